"""The HIP occupancy-grid mapper (csrc/grid_kernels.hip) against the oracle on
the hand-placed cases of tests/grid_cases.py.  No tolerance anywhere: grids,
origins, shapes, bounds and global points are compared with ``array_equal``.

Cases (tests/test_grid_cases.py proves on the CPU what each contains, with
counts; the figures below are cells or beams):

* ``star-24x40`` / ``star-40x24``  437 beams of one scan from one cell: rings 3, 7
  and 4 (every octant, axis, diagonal and slope; 24 error-term ties), the
  zero-length beam, 324 beams that leave through all four borders and the four
  corners; 89 cells end on a hit, 24 on a miss, 847 see misses only.  The two
  shapes catch a swapped row stride.
* ``ragged``  scans of 0, 1, 63, 64, 65, 0, 255, 256, 257, 1, 0 beams (962), robots
  at the centre, in the four corners and outside (1 beam, contributes nothing);
  start grid of all nine start values, odds (5, 2); 85 contested cells, 8 of
  them across a 256-beam block, 9 across scans; 141 saturate below.
* ``count-P``  P = 1, 255, 256, 257, 512 beams; the last beam alone touches a corner.
* ``s300`` (produce)  300 scans of 1, 2, 0, 3 beams; the four extreme points sit
  in scans 260, 269, 281 and in the last beam of scan 299.
* ``duels``  six cells decided by two named beams: neighbouring lanes (10|11,
  12|13), block boundaries (255|256, 511|512), scans 1|3 around an empty one,
  and one beam's own miss and hit one step apart.
* ``long-row``  1 x 32,800: a step >= 2^15 of beam 0 against beam 1's hit.
* ``saturation-*``  130 misses of 1, 2 of 127, hits of 1 and 127, on 1 x 17 and 17 x 1.
* ``start-(kh,km)``  the five odds pairs; untouched / miss-only / last-hit /
  last-miss each meet each of the nine start values.
* ``tiny-*``  1 x 1, 1 x 17, 17 x 1 with results known by hand.
* ``borders``  endpoints on, one ulp below and one ulp above min, two interior
  borders and min + W w (H w), in x and y.
* ``produce-*``  one point (1 x 1), collinear points (1 x 10, 7 x 1), minimum
  extents larger / equal / smaller / mixed, a robot outside the produced grid.

No cell of any case has a hit without a miss, so grid_finalize_kernel's
hit-only branch never runs from this entry point.

Found: the device agreed with the oracle on every case.  One wrapper fault:
``produce_occupancy_grid`` on scans without a single point raised SlamHipError
(a 0 x 0 grid refused by the library) and, with positive minimum extents,
RETURNED a zero grid with a NaN origin; it now raises ValueError like the
reference's ``np.min`` of no points (test_no_points_raise here,
tests/test_grid_cases.py::test_no_points_is_a_value_error on the CPU).
"""
import numpy as np
import pytest

import grid_cases as gc
import grid_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", gc.UPDATE_NAMES)
def test_update_vs_oracle(name):
    import src.produce_occupancy_grid as pog
    c = gc.case(name)
    grid = c.start.copy()
    out = pog.update_occupancy_grid(grid, c.poses, c.scans, c.w, c.geo.min_x, c.geo.min_y, c.k_hit, c.k_miss)
    assert out is grid and grid.dtype == np.int8 and grid.shape == c.ref[0].shape
    assert np.array_equal(grid, c.ref[0])
    if name.startswith("tiny-"):
        assert grid.tolist() == gc.TINY_EXPECTED[name[5:]]
    for _, ((x, y), _, _, value) in c.named.items():
        assert grid[y, x] == value


@pytest.mark.parametrize("name", gc.PRODUCE_NAMES)
def test_produce_vs_oracle(name):
    import src.produce_occupancy_grid as pog
    c = gc.case(name)
    grid, origin = pog.produce_occupancy_grid(c.poses, c.scans, c.w, min_width=c.produce[0], min_height=c.produce[1],
                                              kHitOdds=c.k_hit, kMissOdds=c.k_miss)
    ref, ref_origin = c.ref
    assert tuple(origin) == tuple(ref_origin)
    assert grid.shape == ref.shape and grid.dtype == np.int8
    assert np.array_equal(grid, ref)


@pytest.mark.parametrize("name", ["star-24x40", "s300", "ragged"])
def test_bounds(name):
    """Device bounds == min / max of the exact global points (S = 1, 300, 11)."""
    from slamhip.grid import OccupancyMapper
    c = gc.case(name)
    gp, b = OccupancyMapper(c.poses, c.scans).global_points()
    assert np.array_equal(b, c.bounds())
    assert np.array_equal(gp.cpu().numpy()[:c.P], np.concatenate(c.gpts))


def _fixture_case(g, k):
    off, pts = g[f"off_{k}"], g[f"pts_{k}"]
    return g[f"poses_{k}"], [pts[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_global_points_vs_reference_fixtures(golden):
    import src.produce_occupancy_grid as pog
    g = golden("grid_ref.npz")
    for k in range(int(g["n_cases"])):
        poses, scans = _fixture_case(g, k)
        got = pog.construct_global_points(poses, scans)
        assert [len(a) for a in got] == [len(s) for s in scans]
        assert np.array_equal(np.concatenate(got), g[f"gpts_{k}"]), k


def test_global_points_rotated():
    """Headings +-0.1, pi / 2, 3, ... and coordinates up to 1e3: the device's
    fma(c, x, -s y) + px equals the rational restatement bit for bit."""
    import src.produce_occupancy_grid as pog
    poses, scans = gc.rotated()
    got = pog.construct_global_points(poses, scans)
    want = grid_ref.global_points_exact(poses, scans)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_mapper_reuse():
    """One mapper: a 40 x 24 grid, a 5 x 7 grid (the work buffer stays the larger
    one; counters and keys move inside stale memory), then the 40 x 24 grid again."""
    import occupancy_oracle as oo
    from slamhip.grid import OccupancyMapper
    c, small = gc.case("star-40x24"), gc.case("borders").geo
    m = OccupancyMapper(c.poses, c.scans)
    big = c.start.copy()
    m.update(big, c.w, c.geo.min_x, c.geo.min_y, c.k_hit, c.k_miss)
    assert np.array_equal(big, c.ref[0])
    n_work = m._work.numel()
    # the small grid sits where the star's robot is: beams cross all of it
    sx, sy = c.geo.min_x + 9 * c.w, c.geo.min_y + 17 * c.w
    little = gc.tiled_start(small.H, small.W)
    want = oo.update(little.copy(), c.poses, c.scans, c.w, sx, sy, 5, 2)
    m.update(little, c.w, sx, sy, 5, 2)
    assert m._work.numel() == n_work and np.array_equal(little, want) and np.any(want != gc.tiled_start(5, 7))
    m.update(big, c.w, c.geo.min_x, c.geo.min_y, c.k_hit, c.k_miss)
    twice = oo.update(c.ref[0].copy(), c.poses, c.scans, c.w, c.geo.min_x, c.geo.min_y, c.k_hit, c.k_miss)
    assert np.array_equal(big, twice) and not np.array_equal(twice, c.ref[0])


def test_run_to_run():
    """The atomics only count and take maxima: two runs give identical bytes."""
    import src.produce_occupancy_grid as pog
    c = gc.case("ragged")
    runs = []
    for _ in range(2):
        g = c.start.copy()
        pog.update_occupancy_grid(g, c.poses, c.scans, c.w, c.geo.min_x, c.geo.min_y, c.k_hit, c.k_miss)
        runs.append(g.tobytes())
    assert runs[0] == runs[1] == c.ref[0].tobytes()


def test_no_points_raise():
    """Scans that hold no point: ValueError (the reference's np.min of an empty
    array), never a grid; update_occupancy_grid leaves the grid as it was."""
    import src.produce_occupancy_grid as pog
    poses, scans = np.zeros((3, 3)), [np.zeros((0, 2))] * 3
    for kw in ({}, {"min_width": 2.0, "min_height": 1.0}):
        with pytest.raises(ValueError):
            pog.produce_occupancy_grid(poses, scans, 0.25, **kw)
    g = gc.tiled_start(5, 7)
    pog.update_occupancy_grid(g, poses, scans, 0.25, 0.0, 0.0)
    assert np.array_equal(g, gc.tiled_start(5, 7))
