"""Supersampling (mirt_frame.supersample), the parts that need no GPU: the
band planner (mirt_plan_supersample_bands, host only) and the Python plumbing of the field."""
import ctypes as C

import numpy as np
import pytest

ONE = [(0, 0, 64, 48)]
THREE = [(0, 0, 13, 48), (13, 0, 8, 48), (21, 5, 1, 11)]


def plan(tiles, s, with_ids, cap):
    from distributed_raytracer_amd import _lib as L
    tl = (L.Tile * len(tiles))(*[L.Tile(*t) for t in tiles])
    n = L.lib().mirt_plan_supersample_bands(tl, len(tiles), s, int(with_ids), cap, None, 0)
    if n < 0:
        return n
    out = (L.Tile * max(n, 1))()
    assert L.lib().mirt_plan_supersample_bands(tl, len(tiles), s, int(with_ids), cap, out, n) == n
    return [(b.x, b.y, b.w, b.h) for b in out[:n]]


def caps(tiles, s, with_ids):
    """From below one output column of the shortest tile up to everything at once."""
    per = 33 if with_ids else 25
    col = [s * s * h * per for (_, _, _, h) in tiles]
    whole = sum(s * s * w * h * per for (_, _, w, h) in tiles)
    return sorted({1, min(col) - 1, min(col), max(col), max(col) + 1, 3 * max(col) + 7, 5 * max(col), 21 * max(col) + 100,
                   whole - 1, whole, 10 * whole})


@pytest.mark.parametrize("tiles", [ONE, THREE], ids=["one", "three"])
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("with_ids", [False, True])
def test_bands_partition_the_tiles(tiles, s, with_ids):
    per = 33 if with_ids else 25
    counts = []
    for cap in caps(tiles, s, with_ids):
        bands = plan(tiles, s, with_ids, cap)
        counts.append(len(bands))
        k = 0
        for (x, y, w, h) in tiles:  # list order, left to right, full height, inside one tile
            at = x
            while at < x + w:
                bx, by, bw, bh = bands[k]
                assert (bx, by, bh) == (at, y, h) and bw >= 1 and bx + bw <= x + w, (cap, bands[k])
                if bw > 1:
                    assert s * s * bw * h * per <= cap, (cap, bands[k])
                at += bw
                k += 1
        assert k == len(bands)  # every pixel in exactly one band, and no band besides
    assert counts[0] == sum(w for (_, _, w, _) in tiles)  # below one column: one band per column
    assert counts[-1] == len(tiles)                        # everything fits: one band per tile
    assert counts == sorted(counts, reverse=True)


def test_band_widths_fill_the_cap():
    """A band is as wide as the cap allows: 21 columns of 64x48 at s = 2 with ids."""
    col = 2 * 2 * 48 * 33
    assert [b[2] for b in plan(ONE, 2, True, 21 * col + 100)] == [21, 21, 21, 1]
    assert [b[2] for b in plan(ONE, 2, True, 21 * col - 1)] == [20, 20, 20, 4]


def test_planner_rejects_bad_arguments():
    from distributed_raytracer_amd import _lib as L
    assert plan(ONE, 2, False, 0) == L.MIRT_E_INVALID
    assert plan(ONE, 9, False, 1 << 20) == L.MIRT_E_INVALID
    assert plan(ONE, 0, False, 1 << 20) == L.MIRT_E_INVALID
    assert plan([(0, 0, 0, 4)], 2, False, 1 << 20) == L.MIRT_E_INVALID
    assert L.lib().mirt_plan_supersample_bands(None, 0, 2, 0, 1 << 20, None, 0) == L.MIRT_E_INVALID


def test_env_mutables_carry_supersample():
    import distributed_raytracer_amd as rt
    from distributed_raytracer_amd import _lib as L
    cam = rt.Camera.new((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), 1.0)
    fr, _keep = rt.EnvMutables(cam=cam, supersample=3).to_frame()
    assert fr.supersample == 3 and fr.max_bounces == 0
    fr, _keep = rt.EnvMutables(cam=cam).to_frame()
    assert fr.supersample == 1
    # the field took the place of `reserved`: the struct keeps its size and the field its offset
    assert C.sizeof(L.Frame) == 152
    assert L.Frame.supersample.offset == 148 and L.Frame.max_bounces.offset == 144


def test_tracer_and_draw_take_supersample():
    import inspect

    import distributed_raytracer_amd as rt
    assert inspect.signature(rt.Tracer.__init__).parameters["supersample"].default == 1
    assert inspect.signature(rt.draw).parameters["supersample"].default is None
    assert hasattr(rt.Context, "set_supersample_scratch") and hasattr(rt.Box, "set_supersample_scratch")
