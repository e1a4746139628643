"""CPU checks of the inputs of tests/test_loc_paths_gpu.py (tests/loc_cases.py).

The GPU tests compare the localisation kernels with their NumPy restatement on
hand-placed cases; here every case is shown to be what it claims: (1) the
single-cell fields equal ``min(d_cap^2, dr^2 + dc^2)`` and the definition
(``loc_ref.field_brute``), and sit on the rows and columns the band and block
edges need; (2) each search window selects the (passes, R) it is named for, the
byte-table guard's query holds cells at exactly d_cap^2 and beyond the map, the
big table's cells lie past the first sweep of its fill; (3) each refinement case
ends with the status, iterations and inliers it is built for, the pivot cases
fail the pivot they name, and the cell a point falls in is exact (rational
arithmetic gives the same doubles); (4) no refinement case hangs on the order of
its sums; (5) the restatement's own linearisation is within its rounding bound
of a 50-digit evaluation.
"""
from fractions import Fraction

import numpy as np
import pytest

import loc_cases as lc
import loc_ref

# ------------------------------------------------------------------------------ field


@pytest.mark.parametrize("d_cap", lc.EDGE_CAPS)
def test_single_cell_fields_are_their_closed_form(d_cap):
    for cases, n in ((lc.band_cells(d_cap), lc.BAND_H), (lc.block_cells(d_cap), lc.BLOCK_W)):
        for c in cases:
            assert int((c.grid > 0).sum()) == 1 and c.grid[c.cell] > 0
            want = c.closed_form()
            assert np.array_equal(c.ref, want) and np.array_equal(loc_ref.field_brute(c.grid, d_cap), want)
            assert c.ref[c.cell] == 0 and c.ref.max() == d_cap * d_cap
        at = {c.cell[0] if n == lc.BAND_H else c.cell[1] for c in cases}
        assert len(at) == len(cases)
        e1, e2 = (lc.BAND, 2 * lc.BAND) if n == lc.BAND_H else (lc.BLOCK, 2 * lc.BLOCK)
        need = {0, e1 - 1, e1, e2 - 1, e2, n - 1}                  # both sides of the edges, and the grid's ends
        for k in (d_cap - 1, d_cap, d_cap + 1):
            need |= {e - 1 - k for e in (e1, e2)} | {e - k for e in (e1, e2)}
            need |= {e - 1 + k for e in (e1, e2)} | {e + k for e in (e1, e2)}
        assert at == {p for p in need if 0 <= p < n}
        # for every d_cap, cells exactly d_cap - 1, d_cap and d_cap + 1 outside a band / block on either side
        for k in (d_cap - 1, d_cap, d_cap + 1):
            assert e2 - k - 1 in at and (e1 + k in at or e2 + k in at)
    assert lc.BAND_H > 2 * lc.BAND and lc.BLOCK_W > 2 * lc.BLOCK


def test_shape_cases_cover_the_band_and_block_counts():
    shapes = [c.grid.shape for c in lc.shape_cases()]
    assert shapes == [(127, 3), (128, 3), (129, 3), (256, 3), (257, 3),
                      (3, 255), (3, 256), (3, 257), (3, 511), (3, 513)]
    assert sorted({-(-H // lc.BAND) for H, _ in shapes}) == [1, 2, 3]
    assert sorted({-(-W // lc.BLOCK) for _, W in shapes}) == [1, 2, 3]
    for c in lc.shape_cases():
        occ = c.grid > 0
        assert occ.any()
        assert np.array_equal(c.ref, loc_ref.field_brute(c.grid, c.d_cap))
        assert c.ref.min() == 0 and c.ref.max() == c.d_cap ** 2


def test_halo_case_spans_two_neighbouring_blocks():
    c = lc.halo_case()
    cols = np.nonzero(c.grid[0] > 0)[0]
    assert tuple(cols) == lc.HALO_COLS and c.d_cap == 255 and c.grid.shape == (1, 800)
    gaps = np.diff(cols)
    assert (gaps > 255).sum() == 1 and (gaps < 255).sum() == 2
    assert lc.BLOCK - 255 >= 0 and 2 * lc.BLOCK - 1 + 255 >= 2 * lc.BLOCK     # block 1 reads blocks 0 and 2
    assert np.array_equal(c.ref, loc_ref.field_brute(c.grid, 255))
    assert c.ref[0, 151] == 148 ** 2 and c.ref[0, 152] == 148 ** 2 and c.ref.max() < 255 ** 2
    # between the cells 297 apart the nearer one decides on each side; the cap is never reached (148 < 255)
    assert c.ref[0, 3 + 148] == 148 ** 2 and c.ref[0, 300 - 148] == 148 ** 2


# ----------------------------------------------------------------------------- search

def test_windows_select_every_instantiation():
    assert sorted(r for p, r in lc.R_SHAPES.values() if p == 1) == list(range(1, 9))
    for (nx, ny), (passes, r) in lc.R_SHAPES.items():
        assert lc.search_host_shape(nx, ny) == (passes, r), (nx, ny)
        if passes == 1:
            assert 256 * (r - 1) < nx * ny <= 256 * r
    assert 16 * 16 == 256 and 64 * 32 == 2048 and 3 * 683 == 2049
    assert lc.R_SHAPES[(16, 16)] == (1, 1) and lc.R_SHAPES[(64, 32)] == (1, 8) and lc.R_SHAPES[(3, 683)] == (2, 5)
    # the windows of tests/test_loc_gpu.py select R = 1, 2, 3 and 5 only
    assert {lc.search_host_shape(nx, ny)[1] for nx, ny in ((7, 5), (8, 6), (25, 23), (47, 47), (21, 21), (1, 1))} \
        == {1, 2, 3, 5}
    c = lc.r_case(16, 16)
    assert len(c.scans[0]) == 61 and c.grid.shape == (37, 53) and c.ref[0].shape == (2, 2, 16, 16)


@pytest.mark.parametrize("d_cap", lc.GUARD_CAPS)
def test_guard_query_holds_cells_at_the_cap_and_beyond_the_map(d_cap):
    c = lc.guard_case(d_cap)
    H, W = c.grid.shape
    cx, cy = c.cells(0)
    pts = c.scans[0]
    for p, (x, y) in enumerate(pts):    # heading 0, cell centres of 0.25 m cells: the cell is exact
        fx = (Fraction(float(x)) - Fraction(float(c.origin[0]))) / Fraction(c.cw)
        fy = (Fraction(float(y)) - Fraction(float(c.origin[1]))) / Fraction(c.cw)
        assert (fx.__floor__(), fy.__floor__()) == (cx[p], cy[p]) and fx - fx.__floor__() == Fraction(1, 2)
    inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    vals = c.F[cy[inside], cx[inside]].astype(int)
    assert (~inside).sum() == 6 and (vals == d_cap * d_cap).sum() >= 4 and (vals == 0).sum() == 3
    assert ((vals > 0) & (vals < d_cap * d_cap)).sum() >= 3
    # exactly d_cap from the nearest occupied cell along a row or column: the first cell at the cap
    assert c.F[2, 3 + d_cap] == d_cap * d_cap and c.F[2, 2 + d_cap] == (d_cap - 1) ** 2
    assert int(c.F.max()) == d_cap * d_cap
    # the host's choice with slam_loc_set_table(1): bytes iff d_cap^2 <= 255
    assert (d_cap * d_cap <= 255) == (d_cap == 15) and 15 * 15 == 225 and 16 * 16 == 256 and 256 % 256 == 0
    costs = c.ref[0]
    assert costs.shape == (1, 1, 3, 3) and len({int(v) for v in costs.reshape(-1)}) > 1


def test_big_table_is_read_past_its_first_sweep():
    c = lc.big_case()
    H, W = c.grid.shape
    w = c.window
    px, py = w["nx"] * w["step"], w["ny"] * w["step"]
    wp, hp = W + 2 * px, H + 2 * py
    assert (H, W) == (1000, 1100) and wp * hp == 1106 * 1006 and wp * hp > lc.TABLE_SWEEP == 1048576
    assert wp * hp <= 2 * lc.TABLE_SWEEP            # the second trip is the last
    lowest = None
    for k in range(w["n_theta"]):
        cx, cy = c.cells(0, k)
        assert np.all((cx >= 0) & (cx < W) & (cy >= 0) & (cy < H))
        at = (cy - (w["ny"] // 2) * w["step"] + py) * wp + (cx - (w["nx"] // 2) * w["step"] + px)
        lowest = int(at.min()) if lowest is None else min(lowest, int(at.min()))
    assert lowest > lc.TABLE_SWEEP
    costs, index, cost = c.ref
    n = len(c.scans[0])
    assert n == 18 and costs.shape == (1, 3, 3, 3) and costs.min() < costs.max() <= n * c.d_cap ** 2
    assert len(np.unique(costs)) >= 9 and not np.array_equal(costs[0, 0], costs[0, 1])
    assert (c.grid[:900] > 0).sum() == 1 and c.grid[3, 4] > 0 and c.F[3, 4] == 0


def test_tile_and_extreme_and_wide_cases():
    c = lc.tile_case()
    assert tuple(len(s) for s in c.scans) == lc.TILE_SIZES == (lc.TILE - 1, lc.TILE, lc.TILE + 1, 2 * lc.TILE + 1)
    cx, cy = c.cells(3)
    outside = (cx < 0) | (cx >= 53) | (cy < 0) | (cy >= 37)
    assert 0 < outside.sum() < len(cx) // 4 and c.window["nx"] == c.window["ny"] == 3
    e = lc.extreme_case()
    assert np.all(np.isfinite(e.scans[0])) and len(e.scans[0]) == len(e.scans[1]) + 3 == 33
    assert np.array_equal(e.scans[0][20:23], lc.EXTREMES)
    for k in range(e.window["n_theta"]):
        cx, cy = e.cells(0, k)
        assert np.all(np.abs(cx[20:23]) >= 2 ** 30) and np.all(np.abs(cy[20:23]) >= 2 ** 30)
    # the three points count d_cap^2 in every bin: the volume is that of the scan without them plus 3 d_cap^2
    assert np.array_equal(e.ref[0][0], e.ref[0][1] + 3 * e.d_cap ** 2)
    # a rotated coordinate that is inf - inf = NaN is outside the map too (the device's fmax gives the low end)
    with np.errstate(all="ignore"):
        cx, cy = loc_ref.cells(np.array([[np.inf, np.inf], [-np.inf, np.inf]]), 0.5, 0.5, 0.0, 0.0, (0.0, 0.0), 0.2)
    assert cx[0] == -2 ** 40 and cy[1] == -2 ** 40 and np.all(np.abs(cx) >= 2 ** 40) and np.all(np.abs(cy) >= 2 ** 40)
    for step, nx, ny in lc.WIDE_WINDOWS:
        w = lc.wide_case(step, nx, ny)
        assert nx * step > w.grid.shape[1] and ny * step > w.grid.shape[0]
    assert {(s, nx % 2, ny % 2) for s, nx, ny in lc.WIDE_WINDOWS} == {(1, 0, 0), (1, 1, 1), (4, 0, 0), (4, 1, 1)}
    assert lc.search_host_shape(54, 38)[0] == 2


# ------------------------------------------------------------------------- refinement

def _exact_uv(c, q):
    """(u, v) of every point at the start pose, heading 0, in rational arithmetic; asserts
    that the restatement's doubles are exactly these."""
    assert q.start[2] == 0.0
    ox, oy, cw = (Fraction(float(v)) for v in (c.origin[0], c.origin[1], c.cw))
    out = []
    for px, py in q.pts:
        u = (Fraction(float(px)) + Fraction(float(q.start[0])) - ox) / cw - Fraction(1, 2)
        v = (Fraction(float(py)) + Fraction(float(q.start[1])) - oy) / cw - Fraction(1, 2)
        if abs(px) < 1e6 and abs(py) < 1e6:
            fu = (((1.0 * px) - (0.0 * py)) + q.start[0] - c.origin[0]) / c.cw - 0.5
            fv = (((0.0 * px) + (1.0 * py)) + q.start[1] - c.origin[1]) / c.cw - 0.5
            assert Fraction(float(fu)) == u and Fraction(float(fv)) == v
        out.append((u, v))
    return out


def _corners(c, u, v):
    """The four field values around (u, v), or None outside the inclusive cell bounds."""
    H, W = c.F.shape
    i0, j0 = u.__floor__(), v.__floor__()
    if not (0 <= i0 <= W - 2 and 0 <= j0 <= H - 2):
        return None
    return [int(c.F[j0, i0]), int(c.F[j0, i0 + 1]), int(c.F[j0 + 1, i0]), int(c.F[j0 + 1, i0 + 1])]


def _pivots(H):
    """(d0, d1, d2) of loc_ref.solve's LDL^T, None from the first pivot that fails on."""
    tol = loc_ref.REFINE_DEFAULTS["pivot_tol"]
    with np.errstate(all="ignore"):
        d0 = H[0, 0]
        if not np.isfinite(d0) or d0 <= tol * H[0, 0]:
            return (d0, None, None)
        l10, l20 = H[0, 1] / d0, H[0, 2] / d0
        d1 = H[1, 1] - l10 * H[0, 1]
        if not np.isfinite(d1) or d1 <= tol * H[1, 1]:
            return (d0, d1, None)
        u = H[1, 2] - l20 * H[0, 1]
        return (d0, d1, (H[2, 2] - l20 * H[0, 2]) - (u / d1) * u)


def test_scan_sizes_cross_the_block_of_256():
    c = lc.size_case()
    assert tuple(len(q.pts) for q in c.queries) == lc.SIZES == (1, 2, 255, 256, 257, 511, 513, 1000)
    assert len(lc.cloud()) == 1110 and len(np.unique(lc.cloud(), axis=0)) == 1110
    _, _, _, _, _, truth = loc_ref.refine_case()
    for q, r in zip(c.queries, c.ref):
        d = q.start - truth
        assert np.hypot(d[0], d[1]) < 0.1 and abs(d[2]) < 0.03
        if len(q.pts) <= 2:
            assert (r["status"], r["iters"], r["inliers"]) == (loc_ref.SINGULAR, 0, len(q.pts))
        else:
            assert (r["status"], r["inliers"]) == (loc_ref.CONVERGED, len(q.pts)) and 2 <= r["iters"] <= 5
            ep, et = loc_ref.pose_error(r["pose"], truth)
            assert ep[0] < 0.01 and et[0] < 0.002      # the sub-cell offsets keep it off the truth itself
    # the first two points of the cloud lie on a wall along x, away from the others: jx = 0 exactly, the dd0 exit
    for n in (0, 1):
        assert c.linearise(c.queries[n])[1][0, 0] == 0.0


def test_iteration_limit_case():
    c = lc.limit_case()
    n = lc.size_case().ref[lc.SIZES.index(257)]["iters"]
    full, short = c.ref
    assert c.queries[0].params == dict(max_iters=n) and c.queries[1].params == dict(max_iters=n - 1) and n >= 2
    assert (full["status"], full["iters"]) == (loc_ref.CONVERGED, n)        # converged ON the last allowed iteration
    assert (short["status"], short["iters"]) == (loc_ref.MAX_ITERS, n - 1)


def test_pivot_cases_fail_the_pivot_they_name():
    dd0, dd1, dd2 = lc.pivot_case()
    for c, inl in ((dd0, 5), (dd1, 5), (dd2, 2)):
        r = c.ref[0]
        assert (r["status"], r["iters"], r["inliers"]) == (loc_ref.SINGULAR, 0, inl)
        assert np.array_equal(r["pose"], c.queries[0].start)
        _exact_uv(c, c.queries[0])
    m, H, g, e = dd0.linearise(dd0.queries[0])
    assert H[0, 0] == 0.0 and H[0, 1] == 0.0 and H[0, 2] == 0.0 and H[1, 1] > 0 and _pivots(H) == (0.0, None, None)
    m, H, g, e = dd1.linearise(dd1.queries[0])
    d = _pivots(H)
    assert H[0, 0] > 0 and H[1, 1] == 0.0 and H[0, 1] == 0.0 and d[0] > 0 and d[1] == 0.0 and d[2] is None
    m, H, g, e = dd2.linearise(dd2.queries[0])
    d = _pivots(H)
    assert H[0, 0] > 0 and H[1, 1] > 0 and d[0] > 0 and d[1] > 0 and d[2] == 0.0
    assert np.array_equal(H, np.diag([H[0, 0], H[1, 1], 0.0]))
    # the two points are (a, 0) and (0, b), each within d_cap of one wall only
    (a, zero_y), (zero_x, b) = dd2.queries[0].pts
    assert zero_y == 0.0 and zero_x == 0.0 and a != 0.0 and b != 0.0
    (u0, v0), (u1, v1) = _exact_uv(dd2, dd2.queries[0])
    assert abs(u0 - 16) < 2 and abs(v0 - 12) > dd2.d_cap + 1 and abs(v1 - 12) < 2 and abs(u1 - 16) > dd2.d_cap + 1


def test_cell_bounds_are_exact_and_inclusive():
    c = lc.bounds_case()
    H, W = c.F.shape
    assert (H, W) == (lc.XH, lc.XW) == (24, 32)
    named = {"fu=-1": (-1, None), "fu=0,a=0": (0, None), "fu=0": (0, None), "fu=W-2,a=0": (W - 2, None),
             "fu=W-2": (W - 2, None), "fu=W-1,a=0": (W - 1, None), "fv=-1": (None, -1), "fv=0,b=0": (None, 0),
             "fv=0": (None, 0), "fv=H-2,b=0": (None, H - 2), "fv=H-2": (None, H - 2), "fv=H-1,b=0": (None, H - 1)}
    assert list(named) == list(lc.BOUNDS)
    for q, r in zip(c.queries[:len(named)], c.ref):
        uv = _exact_uv(c, q)
        (u, v), (i0, j0) = uv[0], named[q.name]
        assert i0 is None or u.__floor__() == i0
        assert j0 is None or v.__floor__() == j0
        if "a=0" in q.name:
            assert u == u.__floor__()
        if "b=0" in q.name:
            assert v == v.__floor__()
        inside = lc.BOUNDS[q.name][1]
        corners = _corners(c, u, v)
        assert (corners is not None) == inside
        assert corners is None or min(corners) < c.d_cap ** 2      # in the grid AND on the field: an inlier
        for uu, vv in uv[1:]:                                      # the eight ordinary points
            assert min(_corners(c, uu, vv)) == 0
        assert len(q.pts) == 9 and q.params == dict(max_iters=1)
        assert r["inliers"] == 8 + inside and r["iters"] == 1 and r["status"] in (loc_ref.CONVERGED, loc_ref.MAX_ITERS)
        assert c.linearise(q)[0] == 8 + inside
    assert [r["inliers"] for r in c.ref[len(named):]] == [8 + 8, 8] and len(c.queries[-1].pts) == 12


def test_cap_case_counts():
    c = lc.cap_case()
    q, cap2 = c.queries[0], c.d_cap ** 2
    assert cap2 == 4 and c.F[lc.CAP_CELL] == 0
    kinds = [sum(f == cap2 for f in _corners(c, u, v)) for u, v in _exact_uv(c, q)]
    assert kinds[:4] == [3, 3, 3, 3] and kinds[4:8] == [4, 4, 4, 4] and all(k < 3 for k in kinds[8:])
    assert len(kinds) == 16
    assert c.linearise(q)[0] == 12 and c.ref[0]["inliers"] == 12 and c.ref[0]["iters"] == 1


def test_inlier_fraction_case():
    c = lc.fraction_case()
    for q, r, (f, too_few) in zip(c.queries, c.ref, lc.FRACTIONS):
        assert q.params == dict(min_inlier_frac=f) and len(q.pts) == 8 and c.linearise(q)[0] == 4
        assert np.array_equal(q.pts[4:7], lc.EXTREMES)
        uv = _exact_uv(c, q)
        assert [(_corners(c, u, v) is not None) for u, v in uv] == [True] * 4 + [False] * 3 + [True]
        assert set(_corners(c, *uv[7])) == {c.d_cap ** 2}
        if too_few:
            assert (r["status"], r["iters"], r["inliers"]) == (loc_ref.TOO_FEW, 0, 4)
            assert np.array_equal(r["pose"], q.start)
        else:
            assert r["status"] == loc_ref.CONVERGED and r["iters"] >= 1 and r["inliers"] == 4
    assert 4.0 < 0.5000001 * 8 and not 4.0 < 0.5 * 8 and 4.0 < 0.625 * 8 == 5.0


def test_statuses_after_a_step():
    too_few, singular = lc.after_step_case()
    r, q = too_few.ref[0], too_few.queries[0]
    assert (r["status"], r["iters"], r["inliers"]) == (loc_ref.TOO_FEW, 1, 8) and too_few.linearise(q)[0] == 9
    r, q = singular.ref[0], singular.queries[0]
    assert (r["status"], r["iters"], r["inliers"]) == (loc_ref.SINGULAR, 1, 40) and singular.linearise(q)[0] == 42
    m, H, g, e = singular.linearise(q, r["pose"])
    d = _pivots(H)
    assert m == 40 and H[1, 1] == 0.0 and H[0, 1] == 0.0 and H[0, 0] > 0 and d[1] == 0.0 and d[2] is None
    assert r["pose"][0] - q.start[0] > 1.25 * lc.XCW       # a quarter cell to spare: the two points are out of reach
    for c in (too_few, singular):              # the pose is that of the last linearisation: one step from the start
        one = loc_ref.refine(c.F, c.origin, c.cw, c.d_cap, c.queries[0].pts, c.queries[0].start,
                             **{**loc_ref.REFINE_DEFAULTS, **c.queries[0].params, "max_iters": 1})
        assert np.array_equal(one["pose"], c.ref[0]["pose"]) and not np.array_equal(one["pose"], c.queries[0].start)


def test_every_status_is_reached_and_no_case_hangs_on_the_order_of_its_sums():
    """The precondition of the GPU comparison: under three seeded permutations of the
    order of the eleven sums the restatement gives the same iterations, inliers and
    status and poses within 1e-10.  A difference on the device is then a defect,
    not the order of the sums."""
    seen = set()
    for c in lc.refine_cases():
        for q, r in zip(c.queries, c.ref):
            seen.add((r["status"], r["iters"] > 0))
            for seed in range(3):
                s = c.refine(q, rng=np.random.default_rng(seed))
                assert (s["iters"], s["status"], s["inliers"]) == (r["iters"], r["status"], r["inliers"]), c.name
                assert np.abs(s["pose"] - r["pose"]).max() <= 1e-10, (c.name, q.name)
    assert seen == {(loc_ref.CONVERGED, True), (loc_ref.MAX_ITERS, True), (loc_ref.SINGULAR, False),
                    (loc_ref.SINGULAR, True), (loc_ref.TOO_FEW, False), (loc_ref.TOO_FEW, True)}


def _mp_linearise(c, q):
    """(H (3, 3), g (3,), e) and the sums of the terms' absolute values, at 50 digits,
    at the start pose (heading 0): cells from rational arithmetic, everything else mpmath."""
    import mpmath as mp
    mp.mp.dps = 50

    def f(x):
        return mp.mpf(x.numerator) / mp.mpf(x.denominator)

    cw, cap2 = f(Fraction(c.cw)), c.d_cap ** 2
    S = [mp.mpf(0)] * 10
    A = [mp.mpf(0)] * 10
    n = 0
    for (u, v), (px, py) in zip(_exact_uv(c, q), q.pts):
        corners = _corners(c, u, v)
        if corners is None or all(x == cap2 for x in corners):
            continue
        n += 1
        a, b = f(u - u.__floor__()), f(v - v.__floor__())
        D00, D10, D01, D11 = (mp.sqrt(mp.mpf(x)) * cw for x in corners)
        r = (1 - b) * ((1 - a) * D00 + a * D10) + b * ((1 - a) * D01 + a * D11)
        jx = ((1 - b) * (D10 - D00) + b * (D11 - D01)) / cw
        jy = ((1 - a) * (D01 - D00) + a * (D11 - D10)) / cw
        jt = jx * (-f(Fraction(float(py)))) + jy * f(Fraction(float(px)))        # cos = 1, sin = 0
        for k, t in enumerate((jx * jx, jx * jy, jx * jt, jy * jy, jy * jt, jt * jt, jx * r, jy * r, jt * r, r * r)):
            S[k] += t
            A[k] += abs(t)
    return n, S, A


@pytest.mark.parametrize("which", ["bounds", "cap", "fraction"])
def test_restatement_linearisation_against_50_digits(which):
    """One linearisation (H, g, e) of the restatement against mpmath at 50 digits.

    Bound per entry: |delta| <= 64 n 2^-53 sum |term|.  A term (say jx * jt) is
    reached from exact inputs (u, v and the integer field values are exact here)
    through fewer than 32 rounded operations: four square roots and their products
    with the cell width (8), a1 and b1 (2), the bilinear residual (9), jx and jy (8
    each, sharing the differences), jt (4 at heading 0) and the product itself (1);
    no two of them cancel beyond the term's own size except the differences of the
    D's, whose operands are exact multiples of the cell width for the integer
    distances that dominate.  Each rounding contributes at most 2^-53 of the
    term's size, so a term is within 32 * 2^-53 |term| (first order), and the
    n-term sum adds at most (n - 1) 2^-53 sum |term|: together below
    (32 + n) 2^-53 sum |term| <= 64 n 2^-53 sum |term| for n >= 1."""
    c = {"bounds": lc.bounds_case, "cap": lc.cap_case, "fraction": lc.fraction_case}[which]()
    q = c.queries[{"bounds": 12, "cap": 0, "fraction": 0}[which]]       # bounds: all the inside points together
    m, H, g, e = c.linearise(q)
    n, S, A = _mp_linearise(c, q)
    assert n == m >= 4
    got = [H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2], g[0], g[1], g[2], e]
    for k in range(10):
        delta = abs(S[k] - got[k])
        bound = 64 * n * 2.0 ** -53 * A[k]
        print("%s entry %d: delta %.3e bound %.3e" % (which, k, float(delta), float(bound)))
        assert delta <= bound, (which, k, float(delta), float(bound))
    assert A[9] > 0 and A[0] > 0 and A[3] > 0
