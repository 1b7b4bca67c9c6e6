"""Frames at the ends of what mirt_frame allows (include/mirt.h): 0, 1, 15 and 16 lights, 0 and
16 objects, 8 bounces, supersample 5..8, through every kernel family, the frame group, the
emulated world and the box.

Every frame is compared with the oracle's rtreego restatement (Oracle(sc, use_rtree=True)) on
every plane the path produces, with np.array_equal: the scenes' materials have integer Ns, for
which go_pow is bit-exact with Go (gomath.hpp), so no comparison needs a tolerance.  The first
test (CPU only) checks on the oracle alone that the scenes can show what the GPU tests look for
(a lost light, a wrong clamp order, a lost object); the GPU tests mean little unless it passes."""
import copy
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN
from scenes import CLAMP_LIGHT_SCALE, limit_scene

gpu = pytest.mark.gpu

W, H = 64, 48
PLANES = ("valid", "face", "obj", "rgb", "rgb8")
# (n_lights, clamp): clamp is the 16-light variant with colours at CLAMP_LIGHT_SCALE
LIGHT_CASES = [(0, False), (1, False), (15, False), (16, False), (16, True)]
LIGHT_IDS = ["0", "1", "15", "16", "16clamp"]
# name -> (n_objects, big)
KINDS = {"resident": (1, False), "big": (1, True), "three": (3, False), "sixteen": (16, False), "empty": (0, False)}

_SCENES, _REFS, _MESH_IDS = {}, {}, {}


def scene(kind, n_lights, clamp=False):
    key = (kind, n_lights, clamp)
    if key not in _SCENES:
        n_objects, big = KINDS[kind]
        _SCENES[key] = limit_scene(n_lights, n_objects, big=big, light_scale=CLAMP_LIGHT_SCALE if clamp else None)
    return _SCENES[key]


def oracle_frame(sc, w=W, h=H, bounces=0, tile=None):
    """The oracle's frame (or tile) of `sc`, computed once and left unchanged."""
    key = (id(sc), w, h, bounces, tile)
    if key not in _REFS:
        from oracle.oracle import Oracle
        o = Oracle(sc, use_rtree=True)
        o.set_bounces(bounces)
        r = o.trace_tiles(w, h, [tile or (0, 0, w, h)], nthreads=8)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = (sc, r)
    return _REFS[key][1]


def mutables(mesh_ids, sc, **kw):
    import distributed_raytracer_amd as rt
    cam = rt.Camera.new(sc.cam_pos, sc.cam_dir, sc.fov)
    return rt.EnvMutables([rt.SceneObject(mesh_ids[mi], pos) for mi, pos in sc.objects],
                          [rt.Light(tuple(p), tuple(c)) for p, c in sc.lights], cam, **kw)


def env_of(ctx, sc, big=False, **kw):
    """An Environment of `sc` on `ctx`; the two meshes (the same for every limit_scene of one
    `big`) are uploaded once per context."""
    import distributed_raytracer_amd as rt
    key = (id(ctx), big)
    if key not in _MESH_IDS:
        _MESH_IDS[key] = (ctx, [ctx.upload_mesh(m.vertices, m.normals, m.face_v, m.face_n, m.face_mat, m.materials)
                                for m in sc.meshes])
    ids = _MESH_IDS[key][1]
    return rt.Environment(ctx, ids, mutables(ids, sc, **kw), [])


def assert_frame(got, ref, n_lights, what, planes=PLANES, shadow=True):
    for k in planes:
        g = getattr(got, k)
        assert np.array_equal(g, ref[k]), f"{what}: {k} differs in {(g != ref[k]).reshape(len(g), -1).any(axis=1).sum()} px"
    st, rs = got.stats, ref["stats"]
    assert st["primary_rays"] == rs["primary_rays"]
    assert st["hits"] == rs["hits"] == int(ref["valid"].sum()), what
    assert st["shadow_rays"] == rs["shadow_rays"], what
    if shadow:  # one bounce-free frame: a shadow ray per hit and light, none without lights
        assert st["shadow_rays"] == st["hits"] * n_lights, what


def assert_ambient_only(got, sc, what):
    """No lights: tracer.go's phong adds nothing to Ka, so every hit pixel is exactly its
    material's Ka, and rgb8 its truncation (colour.go:59-61)."""
    hit = np.flatnonzero(got.valid)
    assert len(hit) > 0
    ka = np.zeros((len(hit), 3))
    for n, p in enumerate(hit):
        m = sc.meshes[sc.objects[got.obj[p]][0]]
        ka[n] = m.materials[m.face_mat[got.face[p]]][:3]
    assert np.array_equal(got.rgb[hit], ka), what
    assert np.array_equal(got.rgb8[hit], (255.0 * ka).astype(np.uint8)), what


# --------------------------------------------------------------------------- the scenes (CPU)
def test_limit_scenes_can_show_the_faults_on_the_oracle():
    """Conditions on the oracle alone, at 64x48, for every scene of the GPU tests below that
    has more than one light and at least one object:
    1. removing any single light changes at least one hit pixel (a lost light shows);
    2. at least half of the hit pixels have every channel below 1.0 (not saturated away);
    3. the 16-object scenes have pairwise distinct object-camera distances (Go's sort is not
       stable: ties have no defined reference order) and object 15 wins a pixel;
    4. in the 16-light variants at CLAMP_LIGHT_SCALE some but not all hit pixels reach 1.0
       (colour.Add clamps after every light: the clamp order stays under test)."""
    used = [("resident", 3, False), ("three", 3, False), ("sixteen", 3, False), ("sixteen", 16, False)]
    used += [(kind, nl, clamp) for kind in ("resident", "big", "three") for nl, clamp in LIGHT_CASES if nl > 1]
    for kind, nl, clamp in used:
        sc = scene(kind, nl, clamp)
        what = f"{kind}, {nl} lights" + (" (clamp)" if clamp else "")
        assert len(sc.lights) == nl and len(sc.objects) == KINDS[kind][0]
        for m in sc.meshes:
            assert np.array_equal(m.materials[:, 9], np.floor(m.materials[:, 9])), "go_pow is exact for integer Ns only"
        ref = oracle_frame(sc)
        hit = ref["valid"] == 1
        assert hit.sum() > 100, what
        for k in range(nl):
            less = copy.copy(sc)
            less.lights = sc.lights[:k] + sc.lights[k + 1:]
            r = oracle_frame(less)
            assert np.array_equal(r["valid"], ref["valid"])
            assert (r["rgb"][hit] != ref["rgb"][hit]).any(), f"{what}: light {k} changes no hit pixel"
        below = (ref["rgb"][hit] < 1.0).all(axis=1)
        if clamp:
            reach = (ref["rgb"][hit] >= 1.0).any(axis=1)
            assert reach.any() and not reach.all(), f"{what}: {reach.sum()} of {hit.sum()} hit pixels reach 1.0"
        else:
            assert 2 * below.sum() >= hit.sum(), f"{what}: {below.sum()} of {hit.sum()} hit pixels below 1.0"
        if kind == "sixteen":
            d = [float(np.linalg.norm(np.subtract(pos, sc.cam_pos))) for _, pos in sc.objects]
            assert len(set(d)) == 16, "two objects at the same camera distance"
            assert (ref["obj"][hit] == 15).any(), "object 15 wins no pixel"
            assert len(np.unique(ref["obj"][hit])) >= 8
    big = scene("big", 16)
    assert len(big.meshes[0].face_v) == 3200  # more than kLdsTris: the HBM kernels


# --------------------------------------------------------------------------- 1. light counts
def _light_case(ctx, kind, n_lights, clamp, options):
    """One scene under each of `options`; returns the number of frames compared."""
    import distributed_raytracer_amd as rt
    sc = scene(kind, n_lights, clamp)
    ref = oracle_frame(sc)
    assert ref["valid"].sum() > 100
    env = env_of(ctx, sc, KINDS[kind][1])
    try:
        for opts in options:
            ctx.set_options(opts)
            before = ctx.light_cache_stats()
            fb = rt.draw(env, W, H)
            after = ctx.light_cache_stats()
            assert_frame(fb, ref, n_lights, f"{kind}, {n_lights} lights, options {opts}")
            if n_lights == 0:
                assert fb.stats["shadow_rays"] == 0
                assert_ambient_only(fb, sc, f"{kind}, options {opts}")
                for k in ("builds", "hits", "no_room", "tables", "bytes"):  # no table, no fallback counted
                    assert after[k] == before[k], (k, before, after)
    finally:
        ctx.set_options(0)
    return len(options)


@gpu
@pytest.mark.parametrize("n_lights,clamp", LIGHT_CASES, ids=LIGHT_IDS)
def test_light_counts_one_resident_object(ctx, n_lights, clamp):
    """0, 1, 15 and 16 lights on one LDS-resident object through the fused kernel with and
    without the light table, brute force, the split kernels, the shadow rays as full rays and
    the view tables (6 frames per light count)."""
    from distributed_raytracer_amd import _lib as L
    _light_case(ctx, "resident", n_lights, clamp,
                (0, L.MIRT_OPT_NO_LIGHT_TABLE, L.MIRT_OPT_BRUTE_FORCE, L.MIRT_OPT_SPLIT_KERNELS, L.MIRT_OPT_NO_SEGMENT,
                 L.MIRT_OPT_VIEWS))


@gpu
@pytest.mark.parametrize("n_lights,clamp", LIGHT_CASES, ids=LIGHT_IDS)
def test_light_counts_one_big_object(ctx, n_lights, clamp):
    """The same light counts on a 3,200-face sphere (more than kLdsTris): the two HBM1 kernels."""
    from distributed_raytracer_amd import _lib as L
    _light_case(ctx, "big", n_lights, clamp, (0, L.MIRT_OPT_NO_LDS_STREAM))


@gpu
@pytest.mark.parametrize("n_lights,clamp", LIGHT_CASES, ids=LIGHT_IDS)
def test_light_counts_three_objects(ctx, n_lights, clamp):
    """The same light counts on three objects: the general kernel."""
    _light_case(ctx, "three", n_lights, clamp, (0,))


# --------------------------------------------------------------------------- 2. view tables
def _group_frames(ctx, muts, refs, what, **kw):
    """Render `muts` through one whole-screen frame group (as many frames in flight as it
    has slots at a time) and compare every framebuffer with its oracle frame."""
    import torch
    from distributed_raytracer_amd.framebuffer import NativeFrameGroup
    g = NativeFrameGroup(ctx, W, H, 0, 1, None, with_rgb=True, **kw)
    try:
        for base in range(0, len(muts), g.F):
            idx = [g.render(m.to_frame()) for m in muts[base:base + g.F]]
            g.wait()
            torch.cuda.synchronize()
            for n, i in enumerate(idx):
                got, ref = g.frames[i % g.F], refs[base + n]
                for k in ("valid", "rgb", "rgb8"):
                    a = getattr(got, k).cpu().numpy()
                    assert np.array_equal(a, ref[k]), f"{what}: frame {i}: {k} differs"
    finally:
        g.close()
        ctx.set_grid()
    return len(muts)


@gpu
def test_view_table_budget_edge(ctx):
    """MIRT_OPT_VIEWS builds tables only while frames x (1 + lights) <= 16 (mirt.cpp
    kMaxViewTables) and walks the BVH otherwise: single frames with 15 lights (16 tables) and 16
    lights (17: the walk), a launch of 4 frames with 3 lights (16 tables) and one of 5 frames
    (20: the walk), each bit-exact (valid, rgb and rgb8 from a group, which has no face or
    object plane).  No public counter tells whether tables were used (mirt_debug_counters
    needs a diagnostic build), so both sides of the edge are checked for their results only."""
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    from scenes import with_camera
    ctx.set_options(L.MIRT_OPT_VIEWS)
    try:
        for nl in (15, 16):
            sc = scene("resident", nl)
            assert_frame(rt.draw(env_of(ctx, sc), W, H), oracle_frame(sc), nl, f"views, {nl} lights")
        sc = scene("resident", 3)
        if ("resident", 3, "camera 2") not in _SCENES:
            _SCENES[("resident", 3, "camera 2")] = with_camera(sc, (1.2, -0.6, 4.0), (-0.25, 0.15, -1.0), 1.1)
        cams = [sc, _SCENES[("resident", 3, "camera 2")]]
        ids = env_of(ctx, sc).mesh_ids
        for inflight in (4, 5):
            order = [cams[k % 2] for k in range(inflight)]
            refs = [oracle_frame(s) for s in order]
            assert refs[1]["valid"].sum() > 100 and not np.array_equal(refs[0]["valid"], refs[1]["valid"])
            _group_frames(ctx, [mutables(ids, s) for s in order], refs, f"views, {inflight} frames x 4 tables",
                          inflight=inflight, batch=inflight)
    finally:
        ctx.set_options(0)


# --------------------------------------------------------------------------- 3. object counts
@gpu
def test_no_objects(ctx):
    import distributed_raytracer_amd as rt
    sc = scene("empty", 3)
    ref = oracle_frame(sc)
    assert ref["valid"].sum() == 0
    ctx.profile_enable(True)
    try:
        fb = rt.draw(env_of(ctx, sc), W, H)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert_frame(fb, ref, 3, "no objects")
    assert not fb.valid.any() and not fb.rgb.any() and not fb.rgb8.any()
    assert (fb.face == -1).all() and (fb.obj == -1).all()
    assert fb.stats["primary_rays"] == W * H and fb.stats["hits"] == 0 and fb.stats["shadow_rays"] == 0
    assert prof["primary_rays"] == W * H and prof["hits"] == 0 and prof["stack_overflows"] == 0


@gpu
@pytest.mark.parametrize("n_lights", [3, 16])
def test_sixteen_objects(ctx, n_lights):
    """The reference's camera-distance object order at full length, object 15 among the
    winners (the CPU test above), under the fused kernel, brute force and the split kernels."""
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    sc = scene("sixteen", n_lights)
    ref = oracle_frame(sc)
    env = env_of(ctx, sc)
    try:
        for opts in (0, L.MIRT_OPT_BRUTE_FORCE, L.MIRT_OPT_SPLIT_KERNELS):
            ctx.set_options(opts)
            assert_frame(rt.draw(env, W, H), ref, n_lights, f"16 objects, {n_lights} lights, options {opts}")
    finally:
        ctx.set_options(0)


@gpu
def test_one_past_the_limits_is_rejected(ctx, env):
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    sc = scene("sixteen", 16)
    mut = env_of(ctx, sc).mutable()
    assert len(mut.objects) == L.MIRT_MAX_OBJECTS and len(mut.lights) == L.MIRT_MAX_LIGHTS
    for bad in (dataclasses.replace(mut, objects=mut.objects + mut.objects[:1]),
                dataclasses.replace(mut, lights=mut.lights + mut.lights[:1])):
        with pytest.raises(rt.MirtError) as e:
            rt.draw(env_of(ctx, sc), W, H, bad)
        assert e.value.code == L.MIRT_E_LIMIT
    g = np.load(os.path.join(GOLDEN, "suzanne_64x48.npz"))
    fb = rt.draw(env, 64, 48)
    for k in PLANES:
        assert np.array_equal(getattr(fb, k), g[k]), k


# --------------------------------------------------------------------------- 4. bounces
@gpu
@pytest.mark.parametrize("kind,n_lights,bounces", [("three", 3, 8), ("resident", 16, 8), ("sixteen", 3, 8),
                                                   ("three", 0, 2), ("resident", 0, 2)])
def test_bounce_limit(ctx, kind, n_lights, bounces):
    """max_bounces = MIRT_MAX_BOUNCES on three objects and under 16 lights, and bounces without
    lights, at 48x36: the level waves and the chains (MIRT_OPT_REFLECT_CHAINS) against the
    oracle, ray counts included.  A lone sphere reflects into nothing and the three objects' chains
    end after two bounces, so the 16-object scene is added: there the oracle's eighth bounce still
    adds rays and changes a pixel, and a chain cut one level short would show."""
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    w, h = 48, 36
    sc = scene(kind, n_lights)
    ref = oracle_frame(sc, w, h, bounces)
    assert ref["valid"].sum() > 50 and ref["stats"]["reflection_rays"] >= ref["stats"]["hits"]
    if kind != "resident":
        assert not np.array_equal(ref["rgb"], oracle_frame(sc, w, h)["rgb"])  # the bounces show
    if kind == "sixteen":
        seven = oracle_frame(sc, w, h, bounces - 1)
        assert seven["stats"]["reflection_rays"] < ref["stats"]["reflection_rays"]
        assert not np.array_equal(seven["rgb"], ref["rgb"])
    env = env_of(ctx, sc, max_bounces=bounces)
    try:
        for opts in (0, L.MIRT_OPT_REFLECT_CHAINS):
            ctx.set_options(opts)
            fb = rt.draw(env, w, h)
            assert_frame(fb, ref, n_lights, f"{kind}, {n_lights} lights, {bounces} bounces, options {opts}",
                         shadow=False)
            assert fb.stats["reflection_rays"] == ref["stats"]["reflection_rays"]
            if n_lights == 0:
                assert fb.stats["shadow_rays"] == 0
    finally:
        ctx.set_options(0)


@gpu
def test_nine_bounces_are_rejected(ctx):
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    with pytest.raises(rt.MirtError) as e:
        rt.draw(env_of(ctx, scene("resident", 3), max_bounces=9), 8, 8)
    assert e.value.code == L.MIRT_E_LIMIT


# --------------------------------------------------------------------------- 5. frames in flight
@gpu
def test_frames_in_flight_with_changing_light_counts(ctx):
    """Three frames in flight whose light lists have 0, 16, 1, 16, 0 and 15 entries: frames
    with different counts never share a launch (frames_batchable), and the second 16-light
    frame finds the first one's table in the light cache."""
    counts = [0, 16, 1, 16, 0, 15]
    scs = [scene("resident", nl) for nl in counts]
    ids = env_of(ctx, scs[0]).mesh_ids
    before = ctx.light_cache_stats()
    n = _group_frames(ctx, [mutables(ids, s) for s in scs], [oracle_frame(s) for s in scs], "light counts in flight",
                      inflight=3)
    after = ctx.light_cache_stats()
    assert n == 6
    # four frames have lights: each builds its table or finds it; the second 16-light frame finds it
    assert (after["builds"] - before["builds"]) + (after["hits"] - before["hits"]) == 4
    assert after["hits"] > before["hits"] and after["no_room"] == before["no_room"]


# --------------------------------------------------------------------------- 6. group and box
GROUP_SCENES = [("resident", 0), ("resident", 16), ("empty", 3), ("sixteen", 3)]


@gpu
def test_emulated_world_at_the_limits(ctx):
    """A 2-way deal of 8-px strips on one GPU (tests/test_group_emulated.py): no lights, 16
    lights, no objects and 16 objects (the last two have no frustum pre-test, so their hit
    rectangle is the whole screen: with no objects every transferred pixel is a miss)."""
    import torch
    from distributed_raytracer_amd.framebuffer import NativeFrameGroup
    scs = [scene(kind, nl) for kind, nl in GROUP_SCENES]
    ids = env_of(ctx, scs[0]).mesh_ids
    g = NativeFrameGroup(ctx, W, H, 0, 1, 8, inflight=4, emulate=2)
    try:
        for sc in scs:
            g.render(mutables(ids, sc).to_frame())
        g.wait()
        torch.cuda.synchronize()
        for k, sc in enumerate(scs):
            ref = oracle_frame(sc)
            assert np.array_equal(g.frames[k].valid.cpu().numpy(), ref["valid"]), f"{GROUP_SCENES[k]}: valid differs"
            assert np.array_equal(g.frames[k].rgb8.cpu().numpy(), ref["rgb8"]), f"{GROUP_SCENES[k]}: rgb8 differs"
    finally:
        g.close()
        ctx.set_grid()


@gpu
def test_box_orders_at_the_limits():
    """One order for each of the same scenes served by a box of 8 entries on device 0 (device
    copies, strips of 5 columns): every plane equals the oracle's."""
    import distributed_raytracer_amd as rt
    order = (3, 0, 41, 48)
    box = rt.Box([0] * 8)
    try:
        box.set_transport(rt._lib.MIRT_BOX_COPY)
        box.set_strip(5)
        for kind, nl in GROUP_SCENES:
            sc = scene(kind, nl)
            ref = oracle_frame(sc, tile=order)
            assert ref["valid"].any() or kind == "empty"
            r = rt.trace_tile(env_of(box, sc), *order, W, H)
            for k in PLANES:
                assert np.array_equal(getattr(r, k), ref[k]), f"{kind}, {nl} lights: {k} differs"
            assert r.stats["primary_rays"] == 41 * 48 and r.stats["hits"] == ref["stats"]["hits"]
            assert r.stats["shadow_rays"] == ref["stats"]["hits"] * nl
    finally:
        _MESH_IDS.pop((id(box), False), None)
        box.close()


# --------------------------------------------------------------------------- 7. supersample 5..8
@gpu
@pytest.mark.parametrize("w,h,s", [(16, 12, 5), (16, 12, 6), (12, 10, 7), (12, 8, 8)])
def test_supersample_5_to_8(env, py_scene, w, h, s):
    """k_resolve<5> .. k_resolve<8>: the odd-S 8-byte loads above the unroll, the 16-byte colour
    loads with 16-bit valid loads (6), two 32-bit valid words (8)."""
    import distributed_raytracer_amd as rt
    from test_supersample_gpu import assert_planes, expected, hires
    exp = expected(hires(py_scene, s, w, h), s, w, h, (0, 0, w, h))
    partial = (exp["count"] >= 1) & (exp["count"] <= s * s - 1)
    assert partial.any(), "no partly covered pixel: 'any sample' and 'all samples' would not differ"
    assert (exp["count"] == s * s).any() and (exp["count"] == 0).any()
    fb = rt.draw(env, w, h, supersample=s)
    assert_planes(fb, exp)
    assert fb.stats["primary_rays"] == w * h * s * s and fb.stats["hits"] == exp["hits"]
    miss = exp["count"] == 0
    assert not fb.rgb[miss].any() and not fb.rgb8[miss].any() and (fb.face[miss] == -1).all()


@gpu
@pytest.mark.parametrize("s", [6, 7])
def test_supersample_off_origin_odd_tile(env, py_scene, s):
    import distributed_raytracer_amd as rt
    from test_supersample_gpu import assert_planes, expected, hires
    w, h, tile = 16, 12, (3, 1, 7, 5)
    exp = expected(hires(py_scene, s, w, h), s, w, h, tile)
    assert exp["valid"].any() and not exp["valid"].all() and ((exp["count"] > 0) & (exp["count"] < s * s)).any()
    r = rt.trace_tile(env, *tile, w, h, dataclasses.replace(env.mutable(), supersample=s))
    assert_planes(r, exp)
    assert r.stats["primary_rays"] == 7 * 5 * s * s and r.stats["hits"] == exp["hits"]


@gpu
def test_supersample_5_under_sixteen_lights(ctx):
    import distributed_raytracer_amd as rt
    from test_supersample_gpu import assert_planes, expected, hires
    w, h, s = 16, 12, 5
    sc = scene("resident", 16)
    exp = expected(hires(sc, s, w, h), s, w, h, (0, 0, w, h))
    assert ((exp["count"] >= 1) & (exp["count"] <= s * s - 1)).any()
    fb = rt.draw(env_of(ctx, sc), w, h, supersample=s)
    assert_planes(fb, exp)
    assert fb.stats["hits"] == exp["hits"] and fb.stats["shadow_rays"] == 16 * exp["hits"]
