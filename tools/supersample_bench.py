"""Cost of supersampling (mirt_frame.supersample) on one GPU.

Times mirt_trace_tiles_async of the whole screen into device buffers with HIP events on one
stream: the BASELINE configs[1] scene (tests/golden/example/scene.json) at 1920x1080, planes
rgb8 + valid.  Modes (the rounds run them one after the other, so they share the machine's
state; per mode the median and the spread over the rounds are reported):

  ss1, ss2, ss4   supersample 1, 2, 4 (ss4 takes several bands at the default scratch cap)
  plain4k         the plain trace of the 2W x 2H screen with the same camera producing
                  rgb + valid: the kernel and the bytes of the s = 2 sample pass.  With
                  MIRT_LIB=<an older libmirt.so> this is the parent build's figure
  copy            a device-to-device hipMemcpyAsync of the s = 2 scratch size (25 bytes a
                  sample): reads and writes all of it, where the resolve reads it once and
                  writes a quarter of the pixels, so an upper model of the resolve

usage: python tools/supersample_bench.py [--modes ss1,ss2,ss4,plain4k,copy] [--rounds 60]
                                         [--warmup 10] [--width 1920] [--height 1080]
One JSON line per mode (with mirt_build_id) on stdout.
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENE = os.path.join(ROOT, "tests", "golden", "example", "scene.json")


def hip_runtime():
    """The HIP runtime this process already loaded (one per process, _lib.py)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="ss1,ss2,ss4,plain4k,copy")
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("supersample_bench needs a GPU: nothing is measured without one")
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L

    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    ctx = rt.Context(0)
    env = rt.Environment.from_file(SCENE, ctx)
    build_id = L.lib().mirt_build_id().decode()
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def trace_call(s, w, h, planes):
        """One mirt_trace_tiles_async of the whole w x h screen at supersample s."""
        fr, keep = dataclasses.replace(env.mutable(), supersample=s).to_frame()
        bufs = {"valid": torch.empty(w * h, dtype=torch.uint8, device=dev)}
        if "rgb8" in planes:
            bufs["rgb8"] = torch.empty(w * h * 3, dtype=torch.uint8, device=dev)
        if "rgb" in planes:
            bufs["rgb"] = torch.empty(w * h * 3, dtype=torch.float64, device=dev)
        out = L.Outputs(bufs["rgb"].data_ptr() if "rgb" in bufs else None,
                        bufs["rgb8"].data_ptr() if "rgb8" in bufs else None, bufs["valid"].data_ptr(), None, None, None)
        tile = (L.Tile * 1)(L.Tile(0, 0, w, h))

        def call():
            L.check(L.lib().mirt_trace_tiles_async(ctx.handle, C.byref(fr), w, h, tile, 1, C.byref(out), sp, None))
        call.keep = (fr, keep, bufs, out, tile)
        call.valid = bufs["valid"]
        return call

    scratch2 = 25 * 4 * W * H
    calls = {}
    for m in a.modes.split(","):
        if m in ("ss1", "ss2", "ss4"):
            calls[m] = trace_call(int(m[2:]), W, H, ("rgb8",))
        elif m == "plain4k":
            calls[m] = trace_call(1, 2 * W, 2 * H, ("rgb",))
        elif m == "copy":
            src = torch.zeros(scratch2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)

            def copy(src=src, dst=dst):
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), scratch2, 3, sp)  # device to device
                if rc != 0:
                    raise SystemExit(f"hipMemcpyAsync: {rc}")
            calls[m] = copy
        else:
            raise SystemExit(f"unknown mode {m}")

    ev = {m: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.rounds)]
          for m in calls}
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for m, f in calls.items():
                f()
        stream.synchronize()
        for k in range(a.rounds):
            for m, f in calls.items():
                ev[m][k][0].record(stream)
                f()
                ev[m][k][1].record(stream)
            stream.synchronize()  # a round at a time: the host never runs ahead of what is timed
    for m in calls:
        ms = np.array([s.elapsed_time(e) for s, e in ev[m]])
        line = {"tool": "supersample_bench", "mode": m, "mirt_build_id": build_id, "lib": os.path.basename(L.LIB_PATH),
                "W": W, "H": H, "rounds": a.rounds, "warmup": a.warmup,
                "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                "ms_p10": round(float(np.percentile(ms, 10)), 4), "ms_p90": round(float(np.percentile(ms, 90)), 4)}
        if m.startswith("ss"):
            s = int(m[2:])
            line["supersample"] = s
            line["planes"] = "rgb8+valid"
            if s > 1 and hasattr(L.lib(), "mirt_plan_supersample_bands"):
                tile = (L.Tile * 1)(L.Tile(0, 0, W, H))
                line["bands"] = L.lib().mirt_plan_supersample_bands(tile, 1, s, 0, 256 << 20, None, 0)
            line["hit_pixels"] = int(calls[m].valid.sum().item())
        elif m == "plain4k":
            line["planes"] = "rgb+valid"
            line["screen"] = [2 * W, 2 * H]
            line["hit_pixels"] = int(calls[m].valid.sum().item())
        else:
            line["bytes"] = scratch2
            line["GBps_read_plus_write"] = round(2 * scratch2 / (float(np.median(ms)) * 1e-3) / 1e9, 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
