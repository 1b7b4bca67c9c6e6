"""k_trace's ring chunks keep their light state in LDS (kernels.hip ChunkLights: one lit ballot
per light and a done count per ring position) while chunks past the ring keep the device-scope
words.  The frame group's fused host copy, which k_trace runs ahead of
the same work loop, is covered at odd heights and on a single workgroup.

Every frame is compared with the oracle on valid, rgb8 and the fp64 rgb plane with
np.array_equal (suzanne's material has an integer Ns, for which go_pow is bit-exact with Go).
The oracle frames are computed once per (camera, light count, size) and left unchanged."""
import copy
import math

import numpy as np
import pytest

from scenes import with_camera

gpu = pytest.mark.gpu

_REFS = {}
# the close camera of test_hit_chunk_ring_many_batches_per_workgroup (more hit blocks) and a
# second one, for launches and bursts whose frames differ; "edge" looks past the object, which
# then covers the frame's last columns and rows
CAMS = {"default": None, "close": 0.55, "side": ((2.2, 0.4, 4.0), (-0.3, 0.1, -1.0), 1.1),
        "edge": ((0.55, 0.55, 2.75), (0.3, 0.3, -1.0), None)}


def scene_of(py_scene, cam="default", n_lights=3):
    """suzanne under `n_lights` lights (its own three first, then a seeded ring of dim ones: the
    frame must not saturate, or a lost lit bit would not show)
    from camera `cam`."""
    sc = copy.copy(py_scene)
    lights = list(py_scene.lights)
    rng = np.random.default_rng(7)
    for k in range(len(lights), n_lights):
        a = 2 * math.pi * k / 13
        pos = (1.0 + 6.0 * math.cos(a), 1.0 + 6.0 * math.sin(a), 4.0 + float(rng.uniform(-1, 1)))
        lights.append((pos, tuple(float(x) * 0.04 for x in rng.uniform(0.2, 1.0, 3))))
    sc.lights = lights[:n_lights]
    c = CAMS[cam]
    if isinstance(c, float):
        sc = with_camera(sc, tuple(np.asarray(py_scene.cam_pos) * c), py_scene.cam_dir)
    elif c is not None:
        sc = with_camera(sc, *c)
    return sc


def reference(py_scene, cam, n_lights, w, h):
    key = (cam, n_lights, w, h)
    if key not in _REFS:
        from oracle.oracle import Oracle
        r = Oracle(scene_of(py_scene, cam, n_lights)).frame(w, h, nthreads=8)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def mutables(env, sc):
    import distributed_raytracer_amd as rt
    return rt.EnvMutables(env.mutable().objects, [rt.Light(tuple(p), tuple(c)) for p, c in sc.lights],
                          rt.Camera.new(sc.cam_pos, sc.cam_dir, sc.fov))


def assert_planes(valid, rgb8, rgb, ref, what):
    for k, g in (("valid", valid), ("rgb8", rgb8), ("rgb", rgb)):
        assert np.array_equal(g, ref[k]), f"{what}: {k} differs in {int((g != ref[k]).reshape(len(g), -1).any(axis=1).sum())} px"


# --------------------------------------------------------------------------- part 1
@gpu
@pytest.mark.parametrize("n_lights", [0, 1, 3, 16])
@pytest.mark.parametrize("max_wg", [1, 3])
def test_ring_and_fallback_chunks_by_light_count(ctx, env, py_scene, max_wg, n_lights):
    """192x144 from the close camera on 1 or 3 workgroups (432 blocks: one workgroup takes two
    256-block batches), where eight waves trace hit blocks faster than their chunks are
    shaded, so more than 8 chunks are live: the ring's chunks (LDS ballots and count) and
    the chunks past it (device words) in one launch, with 0 (one shading pass), 1, 3 and 16
    lights per chunk."""
    import distributed_raytracer_amd as rt
    W, H = 192, 144
    ref = reference(py_scene, "close", n_lights, W, H)
    hit = ref["valid"] == 1
    assert int(hit.sum()) > 5000
    if n_lights:  # most hit pixels below the clamp: every light's bit shows
        assert 2 * int((ref["rgb"][hit] < 1.0).all(axis=1).sum()) > int(hit.sum())
    mut = mutables(env, scene_of(py_scene, "close", n_lights))
    ctx.set_grid(1, max_wg)
    try:
        fb = rt.draw(env, W, H, mut)
    finally:
        ctx.set_grid()
    assert_planes(fb.valid, fb.rgb8, fb.rgb, ref, f"{n_lights} lights, {max_wg} workgroups")
    assert fb.stats["hits"] == int(ref["valid"].sum())
    assert fb.stats["shadow_rays"] == fb.stats["hits"] * n_lights


@gpu
def test_partial_blocks_stay_out_of_the_ballots(env, py_scene):
    """70x50 from a camera that puts the object on the frame's right and bottom edges: the last
    block column is 6 wide and the last row 2 high; a lane outside the frame is never lit and
    never shaded."""
    import distributed_raytracer_amd as rt
    W, H = 70, 50
    ref = reference(py_scene, "edge", 3, W, H)
    edge = ref["valid"].reshape(W, H)
    assert edge[64:, :].any() and edge[:, 48:].any(), "no hit in the partial blocks"
    fb = rt.draw(env, W, H, mutables(env, scene_of(py_scene, "edge")))
    assert_planes(fb.valid, fb.rgb8, fb.rgb, ref, "70x50")
    assert fb.stats["hits"] == int(ref["valid"].sum())


@gpu
def test_two_frames_per_launch_share_the_ring(ctx, env, py_scene):
    """Two cameras alternating through launches of two frames (inflight 4, batch 2), 64x48, 5
    frames: a workgroup's ring positions carry chunks of both frames of its launch."""
    import torch
    from distributed_raytracer_amd.framebuffer import NativeFrameGroup
    W, H, F = 64, 48, 4
    cams = ["default", "close"]
    refs = [reference(py_scene, c, 3, W, H) for c in cams]
    assert not np.array_equal(refs[0]["valid"], refs[1]["valid"])
    muts = [mutables(env, scene_of(py_scene, c)) for c in cams]
    g = NativeFrameGroup(ctx, W, H, 0, 1, None, inflight=F, batch=2, with_rgb=True)
    try:
        for base in (0, F):
            idx = [g.render(muts[k % 2].to_frame()) for k in range(base, min(base + F, 5))]
            g.wait()
            torch.cuda.synchronize()
            for k in idx:
                got = g.frames[k % F]
                assert_planes(got.valid.cpu().numpy(), got.rgb8.cpu().numpy(), got.rgb.cpu().numpy(), refs[k % 2],
                              f"frame {k}")
    finally:
        g.close()
        ctx.set_grid()


# --------------------------------------------------------------------------- fused host copy
def _host_copy_run(ctx, env, py_scene, W, H, every, one_wg):
    """2 * inflight + 1 frames of two alternating cameras through a group of 8 frames in flight
    with host output (the fused copies: each launch copies its stream's previous batch);
    host_frame after every render (`every`) or only after the last, for the frames whose
    slots still hold them."""
    import torch
    from distributed_raytracer_amd.framebuffer import NativeFrameGroup
    F = 8
    cams = ["default", "side"]
    refs = [reference(py_scene, c, 3, W, H) for c in cams]
    assert refs[1]["valid"].sum() > 50 and not np.array_equal(refs[0]["valid"], refs[1]["valid"])
    muts = [mutables(env, scene_of(py_scene, c)) for c in cams]
    n = 2 * F + 1
    g = NativeFrameGroup(ctx, W, H, 0, 1, None, inflight=F, with_rgb=True, host_output=True)
    try:
        if one_wg:
            ctx.set_grid(1, 1)  # the launch's only workgroup copies every column
        for k in range(n):
            i = g.render(muts[k % 2].to_frame())
            assert i == k
            if every:
                rgb8, valid = g.host_frame(k)
                assert np.array_equal(valid, refs[k % 2]["valid"]), f"frame {k}: host valid differs"
                assert np.array_equal(rgb8, refs[k % 2]["rgb8"]), f"frame {k}: host rgb8 differs"
        g.wait()
        torch.cuda.synchronize()
        for k in range(n - F, n):
            rgb8, valid = g.host_frame(k)
            dev = g.frames[k % F]
            assert_planes(valid, rgb8, dev.rgb.cpu().numpy(), refs[k % 2], f"frame {k} (host planes, device rgb)")
            assert np.array_equal(dev.valid.cpu().numpy(), valid) and np.array_equal(dev.rgb8.cpu().numpy(), rgb8)
    finally:
        g.close()
        ctx.set_grid()


@gpu
@pytest.mark.parametrize("every", [True, False], ids=["read_each", "read_last"])
@pytest.mark.parametrize("W,H", [(64, 47), (200, 101)])
def test_fused_host_copy_odd_heights(ctx, env, py_scene, W, H, every):
    """Odd heights: a column's spans end off the 16-byte words of the copy."""
    _host_copy_run(ctx, env, py_scene, W, H, every, one_wg=False)


@gpu
@pytest.mark.parametrize("every", [True, False], ids=["read_each", "read_last"])
def test_fused_host_copy_by_a_single_workgroup(ctx, env, py_scene, every):
    _host_copy_run(ctx, env, py_scene, 200, 101, every, one_wg=True)
