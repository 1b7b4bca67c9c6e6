"""Supersampling on the GPU (mirt_frame.supersample = s), bit for bit.

Sample (a, b) of pixel (i, j) of a W x H screen is the reference's Trace(s i + a, s j + b, s W,
s H), so the oracle's frame at s W x s H holds every sample in fp64 and a fixed-order mean of
them is the exact expected value: every comparison here is array_equal, never a tolerance."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_REF = {}


def hires(py_scene, s, W, H, bounces=0):
    """The oracle's s W x s H frame (computed once per shape, never modified)."""
    key = (id(py_scene), s * W, s * H, bounces)
    if key not in _REF:
        from oracle.oracle import Oracle
        o = Oracle(py_scene)
        o.set_bounces(bounces)
        r = o.frame(s * W, s * H, nthreads=8)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = (py_scene, r)  # the scene stays alive with its key
    return _REF[key][1]


def expected(ref, s, W, H, tile):
    """The planes of tile (x, y, w, h) from the s W x s H oracle frame `ref`: per channel
    acc = +0.0, then acc += S[a][b] for a outer, b inner (a missed sample's colour is zero), then
    acc / (s s); rgb8 = uint8(255 rgb); valid = any sample; face / object = the first valid
    sample's, -1 without one.  Column-major, pixel (x + i, y + j) at i h + j.  count: valid
    samples per pixel."""
    x, y, w, h = tile
    sW, sH = s * W, s * H
    rgb = ref["rgb"].reshape(sW, sH, 3)
    valid = ref["valid"].reshape(sW, sH) != 0
    face = ref["face"].reshape(sW, sH)
    obj = ref["obj"].reshape(sW, sH)
    acc = np.zeros((w, h, 3), np.float64)
    seen = np.zeros((w, h), bool)
    count = np.zeros((w, h), np.int64)
    oface = np.full((w, h), -1, np.int32)
    oobj = np.full((w, h), -1, np.int32)
    for a in range(s):
        for b in range(s):
            sel = (slice(s * x + a, s * (x + w), s), slice(s * y + b, s * (y + h), s))
            v = valid[sel]
            acc += np.where(v[..., None], rgb[sel], 0.0)
            first = v & ~seen
            oface[first] = face[sel][first]
            oobj[first] = obj[sel][first]
            seen |= v
            count += v
    out = acc / float(s * s)
    return dict(rgb=out.reshape(w * h, 3), rgb8=(255 * out).astype(np.uint8).reshape(w * h, 3),
                valid=seen.astype(np.uint8).reshape(w * h), face=oface.reshape(w * h), obj=oobj.reshape(w * h),
                count=count.reshape(w * h), hits=int(valid[s * x:s * (x + w), s * y:s * (y + h)].sum()))


def assert_planes(got, exp, planes=("valid", "face", "obj", "rgb", "rgb8")):
    for k in planes:
        g = getattr(got, k)
        assert np.array_equal(g, exp[k]), f"{k}: {(g != exp[k]).reshape(len(g), -1).any(axis=1).sum()} pixels differ"


@pytest.mark.parametrize("W,H,s", [(64, 48, 2), (40, 30, 3), (32, 24, 4)])
def test_whole_frame_matches_the_oracle_mean(env, py_scene, W, H, s):
    import distributed_raytracer_amd as rt
    exp = expected(hires(py_scene, s, W, H), s, W, H, (0, 0, W, H))
    partial = (exp["count"] >= 1) & (exp["count"] <= s * s - 1)
    assert partial.any(), "no partly covered pixel: 'any sample' and 'all samples' would not differ"
    fb = rt.draw(env, W, H, supersample=s)
    assert_planes(fb, exp)
    assert fb.stats["primary_rays"] == W * H * s * s and fb.stats["hits"] == exp["hits"]
    # a miss stays all zero
    miss = exp["count"] == 0
    assert miss.any() and not fb.rgb[miss].any() and not fb.rgb8[miss].any() and (fb.face[miss] == -1).all()


@pytest.mark.parametrize("tile", [(5, 7, 13, 11), (17, 11, 13, 11)], ids=["background", "silhouette"])
def test_off_origin_odd_tile(env, py_scene, tile):
    """(5, 7, 13, 11) lies beside the object (every sample misses); the same shape at (17, 11)
    crosses its silhouette."""
    import distributed_raytracer_amd as rt
    exp = expected(hires(py_scene, 2, 64, 48), 2, 64, 48, tile)
    if tile[0] == 17:
        assert exp["valid"].any() and not exp["valid"].all() and ((exp["count"] > 0) & (exp["count"] < 4)).any()
    mut = dataclasses.replace(env.mutable(), supersample=2)
    r = rt.trace_tile(env, *tile, 64, 48, mut)
    assert_planes(r, exp)
    assert r.stats["primary_rays"] == 13 * 11 * 4 and r.stats["hits"] == exp["hits"]


def test_bands_change_nothing(ctx, env, py_scene):
    """The scratch cap cuts the frame into bands of 21 columns (not a multiple of the 8-pixel
    blocks), then into single columns: the planes and the statistics stay those of one band."""
    import distributed_raytracer_amd as rt
    from test_supersample_cpu import plan
    W, H, s = 64, 48, 2
    exp = expected(hires(py_scene, s, W, H), s, W, H, (0, 0, W, H))
    whole = rt.draw(env, W, H, supersample=s)
    col = s * s * H * 33  # draw asks for face and object: 33 bytes per sample
    try:
        for cap, widths in [(21 * col + 100, [21, 21, 21, 1]), (col - 1, [1] * W)]:
            assert [b[2] for b in plan([(0, 0, W, H)], s, True, cap)] == widths
            ctx.set_supersample_scratch(cap)
            fb = rt.draw(env, W, H, supersample=s)
            assert_planes(fb, exp)
            for k in ("rgb", "rgb8", "valid", "face", "obj"):
                assert getattr(fb, k).tobytes() == getattr(whole, k).tobytes(), k
            for k in ("primary_rays", "hits", "shadow_rays", "reflection_rays"):
                assert fb.stats[k] == whole.stats[k], k
    finally:
        ctx.set_supersample_scratch(256 << 20)
    with pytest.raises(rt.MirtError) as e:
        ctx.set_supersample_scratch(0)
    assert e.value.code == rt._lib.MIRT_E_INVALID


def test_reflections_compose(env, py_scene):
    import distributed_raytracer_amd as rt
    W, H, s = 32, 24, 2
    ref = hires(py_scene, s, W, H, bounces=2)
    assert ref["stats"]["reflection_rays"] > 0
    exp = expected(ref, s, W, H, (0, 0, W, H))
    plain = expected(hires(py_scene, s, W, H), s, W, H, (0, 0, W, H))
    assert not np.array_equal(exp["rgb"], plain["rgb"])  # the bounces show
    mut = dataclasses.replace(env.mutable(), max_bounces=2)
    fb = rt.draw(env, W, H, mut, supersample=s)
    assert_planes(fb, exp)
    assert fb.stats["reflection_rays"] == ref["stats"]["reflection_rays"]


def test_box_order_and_bulk_trace(ctx, env, py_scene):
    """An order served by a box of 8 entries (one GPU standing in for each), strips of 5
    columns, device copies: the planes of a one-context trace_tile and of the oracle mean; and
    Tracer(..., supersample=2).bulk_trace of the same order with its diff as wire bytes."""
    import distributed_raytracer_amd as rt
    from conftest import SCENE
    from test_gob import read, scenes, wire_scene
    W, H, s, order = 64, 48, 2, (3, 0, 41, 48)
    exp = expected(hires(py_scene, s, W, H), s, W, H, order)
    one = rt.trace_tile(env, *order, W, H, dataclasses.replace(env.mutable(), supersample=s))
    box = rt.Box([0] * 8)
    try:
        box.set_transport(rt._lib.MIRT_BOX_COPY)
        box.set_strip(5)
        box.set_supersample_scratch(64 << 20)
        benv = rt.Environment.from_file(SCENE, box)
        r = rt.trace_tile(benv, *order, W, H, dataclasses.replace(benv.mutable(), supersample=s))
        assert_planes(r, exp)
        for k in ("rgb8", "valid"):
            assert np.array_equal(getattr(r, k), getattr(one, k)), k
        assert r.stats["primary_rays"] == 41 * 48 * 4
        # the wire: the scene a Go worker holds after the same bytes
        sc, _ = scenes()["example"]
        wexp = expected(hires(wire_scene(sc), s, W, H), s, W, H, order)
        genv = rt.Environment.from_gob(read("example_state.gob"), box)
        res = rt.Tracer(genv, W, H, supersample=s).bulk_trace(rt.WorkOrder(*order, read("example_diff.gob")))
        assert np.array_equal(res.results, wexp["rgb8"]) and res.results.any()
        plain = rt.Tracer(genv, W, H).bulk_trace(rt.WorkOrder(*order, read("example_diff.gob")))
        assert not np.array_equal(plain.results, res.results)
    finally:
        box.close()


def test_c_worker_flag(tmp_path, py_scene):
    """worker_c/mirt_worker --supersample 2: the master's partition of a 64x48 screen into 4
    orders, served by a context and by a box of 2 entries; the assembled frame (rgb8, then
    valid, column-major) is the oracle mean."""
    import subprocess

    from conftest import ROOT, SCENE
    W, H, s = 64, 48, 2
    exp = expected(hires(py_scene, s, W, H), s, W, H, (0, 0, W, H))
    out = tmp_path / "fb.bin"
    r = subprocess.run([os.path.join(ROOT, "worker_c", "mirt_worker"), "--box", "2", "--supersample", str(s), SCENE,
                        str(W), str(H), str(out), "4"], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if not k.startswith("PYTHON")})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orders equal: yes" in r.stdout
    raw = np.fromfile(out, np.uint8)
    assert np.array_equal(raw[:W * H * 3].reshape(W * H, 3), exp["rgb8"])
    assert np.array_equal(raw[W * H * 3:], exp["valid"])


@pytest.mark.parametrize("s", [0, 1])
def test_plain_path_unchanged(env, s):
    import distributed_raytracer_amd as rt
    g = np.load(os.path.join(GOLDEN, "suzanne_64x48.npz"))
    fb = rt.draw(env, 64, 48, supersample=s)
    for k in ("valid", "face", "obj", "rgb", "rgb8"):
        assert np.array_equal(getattr(fb, k), g[k]), k
    assert fb.stats["primary_rays"] == 64 * 48


def test_errors_leave_the_context_usable(ctx, env):
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    from distributed_raytracer_amd.framebuffer import NativeFrameGroup
    g = np.load(os.path.join(GOLDEN, "suzanne_64x48.npz"))

    def plain_tile_ok():
        r = rt.trace_tile(env, 0, 0, 64, 48, 64, 48)
        assert np.array_equal(r.rgb8, g["rgb8"]) and np.array_equal(r.valid, g["valid"])

    with pytest.raises(rt.MirtError) as e:
        rt.draw(env, 64, 48, supersample=9)
    assert e.value.code == L.MIRT_E_INVALID
    plain_tile_ok()
    with pytest.raises(rt.MirtError) as e:
        rt.trace_tile(env, 0, 0, 8, 8, 40000, 48, dataclasses.replace(env.mutable(), supersample=2))
    assert e.value.code == L.MIRT_E_LIMIT
    plain_tile_ok()
    grp = NativeFrameGroup(ctx, 64, 48, tile=None, inflight=1)
    try:
        with pytest.raises(rt.MirtError) as e:
            grp.render(dataclasses.replace(env.mutable(), supersample=2).to_frame())
        assert e.value.code == L.MIRT_E_INVALID and "supersample" in str(e.value)
        grp.render(env.mutable().to_frame())  # one ray per pixel is still served
        grp.wait()
    finally:
        grp.close()
    plain_tile_ok()
