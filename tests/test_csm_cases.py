"""CPU checks of the inputs of tests/test_csm_paths_gpu.py (tests/csm_cases.py).

The GPU tests compare the correlative scan matcher's kernels with the NumPy
restatement (tests/csm_ref.py) on hand-placed cases; here (1) the restatement
itself is pinned to ``plain_volume`` below, a plain-loop evaluation of the
definition in include/slamhip.h (Python floats, ``math.floor``, a set of
occupied cells, a set of neighbour cells, explicit bounds tests), on every case,
and to the hand-written volumes and best bins where a case has them; (2) every
case is shown to be what it claims: the reach cases sit on the kernel's clamp
bounds, the saturation case crosses 2^16 with a 0 in the other half of the
16-bit pair, the contraction points change their cell under either FMA form
(``fractions.Fraction``) while the restatement takes the three-rounding one, the
sweep's windows select every ``csm_score_kernel<R, W>`` at both fill levels and
score in their first and last slots; (3) ``slamhip.csm.check_offsets``, the
host-side check of the scan offsets, refuses every bad offsets array.

No device, no mutation: every case's arrays are read-only.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import csm_cases as cc
import csm_ref

# ------------------------------------------------------------ the definition, in plain loops


def plain_cell(p, o, res):
    return math.floor((p - o) / res)


def plain_volume(query, ref, centre, res, G, n_theta, d_theta, nx, ny):
    """S[k][j][i] as nested lists, and the (cos, sin) of every angle."""
    o = -(G // 2) * res
    occupied, beside = set(), set()
    for x, y in ref:
        occupied.add((plain_cell(float(x), o, res), plain_cell(float(y), o, res)))
    for cx, cy in occupied:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (cx + dx, cy + dy) not in occupied:
                    beside.add((cx + dx, cy + dy))
    th0, tx0, ty0 = (float(v) for v in centre)
    S, cs = [], []
    for k in range(n_theta):
        th = th0 + (k - n_theta // 2) * float(d_theta)
        c, s = float(np.cos(th)), float(np.sin(th))       # the caller's table: np.cos / np.sin of the Python float
        cs.append((c, s))
        cells = []
        for x, y in query:
            x, y = float(x), float(y)
            X = (c * x - s * y) + tx0
            Y = (s * x + c * y) + ty0
            cells.append((plain_cell(X, o, res), plain_cell(Y, o, res)))
        vol = []
        for j in range(ny):
            row = []
            for i in range(nx):
                total = 0
                for ix, iy in cells:
                    cx, cy = ix + i - nx // 2, iy + j - ny // 2
                    if cx < 0 or cx >= G or cy < 0 or cy >= G:
                        continue
                    if (cx, cy) in occupied:
                        total += 2
                    elif (cx, cy) in beside:
                        total += 1
                row.append(total)
            vol.append(row)
        S.append(vol)
    return S, cs


def plain_best(S):
    """(score, (k, j, i)) of the first maximum in the order k, j, i."""
    top, at = -1, None
    for k, vol in enumerate(S):
        for j, row in enumerate(vol):
            for i, v in enumerate(row):
                if v > top:
                    top, at = v, (k, j, i)
    return top, at


def plain_transform(cs, index, centre, res, nx, ny):
    k, j, i = index
    c, s = cs[k]
    return [[c, -s, float(centre[1]) + (i - nx // 2) * res], [s, c, float(centre[2]) + (j - ny // 2) * res],
            [0.0, 0.0, 1.0]]


PLAIN_MAX_POINTS = 8193     # the saturation case's 40,000 copies are left to n x the one-point volume


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", cc.hand_cases(), ids=_ids(cc.hand_cases()))
def test_restatement_equals_the_plain_loops(case):
    vol, index, score, tf = case.ref
    p = case.params
    assert vol.dtype == np.int32 and vol.shape == case.shape
    ran = 0
    for b in range(len(case.src)):
        q, r, c = case.pair(b)
        if len(q) > PLAIN_MAX_POINTS:
            continue
        S, cs = plain_volume(q.tolist(), r.tolist(), c, **p)
        assert np.array_equal(vol[b], np.array(S, np.int64).reshape(case.shape[1:])), case.labels[b]
        top, at = plain_best(S)
        assert (int(score[b]), tuple(int(v) for v in index[b])) == (top, at), case.labels[b]
        assert np.array_equal(tf[b], np.array(plain_transform(cs, at, c, p["res"], p["nx"], p["ny"]))), case.labels[b]
        ran += 1
    assert ran >= len(case.src) - 2


@pytest.mark.parametrize("case", cc.hand_cases(), ids=_ids(cc.hand_cases()))
def test_restatement_equals_the_hand_written_numbers(case):
    vol, index, score, _ = case.ref
    if case.expect is not None:
        for b in range(len(vol)):
            assert np.array_equal(vol[b], case.expect[b]), (case.labels[b], vol[b].tolist())
    if case.expect_index is not None:
        assert np.array_equal(index, case.expect_index), index.tolist()
    if case.expect_score is not None:
        assert np.array_equal(score, case.expect_score), score.tolist()
    if case.expect is not None and case.expect_index is None:
        # the best bin of a hand-written volume is its first maximum
        for b in range(len(vol)):
            assert (int(score[b]), tuple(index[b])) == csm_ref.best(case.expect[b])


def test_every_group_of_cases_carries_hand_written_numbers():
    by_name = {c.name: c for c in cc.hand_cases()}
    for name, c in by_name.items():
        if name in ("empty", "grid"):
            continue
        assert c.expect is not None or c.expect_index is not None, name
    assert len(by_name) == len(cc.hand_cases()) == 25


# ------------------------------------------------------------------- reach and the clamp

def _clamp(nx, G=cc.G16):
    """csrc/csm_kernels.hip: the query cell is clamped to [hx - px, (G - 1 + px) - (nx - 1 - hx)], px = nx."""
    hx = nx // 2
    return hx - nx, (G - 1 + nx) - (nx - 1 - hx)


@pytest.mark.parametrize("n", sorted(cc.REACH_CELLS))
def test_reach_cells_sit_on_the_clamp_bounds(n):
    lo_hit, lo_miss, hi_hit, hi_miss = cc.REACH_CELLS[n]
    h = n // 2
    assert (lo_hit, lo_miss, hi_hit, hi_miss) == (-(n - 1 - h), -(n - 1 - h) - 1, cc.G16 - 1 + h, cc.G16 + h)
    assert _clamp(n) == (lo_miss, hi_miss)                 # one cell beyond is the clamp itself, on both sides
    assert lo_hit + (n - 1) - h == 0 and hi_hit - h == cc.G16 - 1     # the last and the first shift reach the cell
    assert cc.REACH_ROWS[n]["low"] == [0] * (n - 1) + [2] and cc.REACH_ROWS[n]["high"] == [2] + [0] * (n - 1)


def test_reach_cases_are_what_they_claim():
    for n, axis in cc.REACH_1D:
        c = cc.reach_case(n, axis)
        assert c.shape == (8, 1, 1, n) if axis == "x" else c.shape == (8, 1, n, 1)
        assert all(len(s) == 1 for s in c.scans)
        vol = c.ref[0].reshape(8, n)
        hits = [b for b in range(8) if vol[b].any()]
        assert [c.labels[b] for b in hits] == ["low reach", "high reach", "low reach again", "high reach again"]
        # every zero pair has a scoring neighbour in the batch
        assert all(b - 1 in hits or b + 1 in hits for b in range(8) if b not in hits)
        lo, hi = _clamp(n)
        assert np.floor(c.scans[6][0] + 8.0).max() == cc.FAR > hi
        assert np.floor(c.scans[7][0] + 8.0).min() == -cc.FAR < lo
    for nx, ny in cc.CORNER_AT:
        c = cc.corner_case(nx, ny)
        vol = c.ref[0]
        assert c.shape == (12, 1, ny, nx)
        for b in range(12):
            assert vol[b].sum() == (2 if b % 3 == 0 else 0), c.labels[b]
        corners = {(int(j), int(i)) for b in range(0, 12, 3) for _, j, i in np.argwhere(vol[b])}
        assert corners == {(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)}


def test_overhang_cases_are_what_they_claim():
    assert cc.OVERHANG_NX == (1, 2, 3, 5, 6, 7)
    assert sorted({-nx % 4 for nx in cc.OVERHANG_NX}) == [1, 2, 3]         # columns the last dword reads too many
    for nx in cc.OVERHANG_NX:
        c = cc.overhang_case(nx)
        hx = nx // 2
        last = 8 + nx - 1 - hx
        # the reference's cells are those right of the window's last column
        cells = [tuple(np.floor(p + 8.0).astype(int)) for p in c.scans[2]]
        assert cells == [(last + 1, 8), (last + 2, 8), (last + 3, 8)]
        vol = c.ref[0]
        assert vol.max() == 1 and cc.OVERHANG_ROWS[nx] == [0] * (nx - 1) + [1]
        # the query at the right clamp, its window's last column the table's last before the dword's spare four
        assert np.floor(c.scans[3][0, 0] + 8.0) == _clamp(nx)[1] == cc.G16 + hx
        assert tuple(np.floor(c.scans[4][1] + 8.0)) == (0, 9) and not vol[2].any()


def test_raster_case_is_what_it_claims():
    c = cc.raster_case()
    assert len(c.scans[5]) == cc.N_DUP == 600 > cc.BLOCK and len(c.scans[6]) == 600
    assert len(np.unique(c.scans[5], axis=0)) == 1 and len(np.unique(c.scans[6], axis=0)) == 2
    L = csm_ref.lookup_table(c.scans[7], cc.G16, 1.0)
    want = np.zeros((16, 16), np.uint8)
    want[7:10, 0] = want[7:10, 15] = 1
    assert np.array_equal(L, want)
    assert not csm_ref.lookup_table(c.scans[9], cc.G16, 1.0).any()


# ------------------------------------------------------------------------ cell boundaries

@pytest.mark.parametrize("res", [cc.DYADIC, 0.05])
def test_boundary_values_fall_in_the_cells_written_down(res):
    cells = cc.DYADIC_CELLS if res == cc.DYADIC else cc.DEFAULT_CELLS
    o = -(cc.G16 // 2) * res
    for k in cc.BOUNDARY_K:
        vals = cc.boundary_values(res, k)
        assert set(vals) == set(cells[k])
        assert vals["below"] < vals["exact"] < vals["above"]
        assert np.nextafter(vals["below"], np.inf) == vals["exact"] == np.nextafter(vals["above"], -np.inf)
        for name, v in vals.items():
            assert plain_cell(v, o, res) == cells[k][name], (k, name)
            assert abs(cells[k][name] - k) <= 1
        if res == cc.DYADIC:
            # exact arithmetic puts every value below the edge into cell k - 1: the definition's
            # rounded v - o does not, and the literals follow the definition
            assert vals["exact"] == o + k * res == Fraction(o) + k * Fraction(res)
            assert math.floor((Fraction(vals["below"]) - Fraction(o)) / Fraction(res)) == k - 1
    assert math.copysign(1.0, cc.boundary_values(cc.DYADIC, 8)["-0.0"]) == -1.0
    assert cc.row3(0, -1) == [0, 1, 0] and cc.row3(-1, 0) == [0, 0, 2] and cc.row3(15, 14) == [2, 1, 0]
    assert cc.row3(8, 8) == [1, 2, 1] and cc.row3(7, 8) == [0, 1, 2] and cc.row3(15, 15) == [1, 2, 0]


# --------------------------------------------------------------- contraction-sensitive points

def _exact_forms(a, x, b, y, t, sign):
    """The three evaluations of (a x + sign b y) + t from rationals: every rounding explicit."""
    F = Fraction
    three = cc.fl(F(cc.fl(F(cc.fl(F(a) * F(x))) + sign * F(cc.fl(F(b) * F(y))))) + F(t))
    first = cc.fl(F(cc.fl(F(a) * F(x) + sign * F(cc.fl(F(b) * F(y))))) + F(t))
    second = cc.fl(F(cc.fl(F(cc.fl(F(a) * F(x))) + sign * F(b) * F(y))) + F(t))
    return three, first, second


def test_contraction_points_change_their_cell_under_an_fma():
    pts = cc.contraction_points()
    assert len(pts) == 12 >= 8 and pts == cc.contraction_points()
    moved = {("X", 0): 0, ("X", 1): 0, ("Y", 0): 0, ("Y", 1): 0}
    o, res = -1.0, cc.DYADIC
    case = cc.contraction_case()
    for n, (th, x, y, tx0, ty0, coord, (cx, cy), _) in enumerate(pts):
        c, s = float(np.cos(th)), float(np.sin(th))
        X = _exact_forms(c, x, s, y, tx0, -1)
        Y = _exact_forms(s, x, c, y, ty0, 1)
        assert X[0] == (c * x - s * y) + tx0 and Y[0] == (s * x + c * y) + ty0     # Python's floats do not contract
        cells_x = [math.floor((Fraction(cc.fl(Fraction(v) - Fraction(o)))) / Fraction(res)) for v in X]
        cells_y = [math.floor((Fraction(cc.fl(Fraction(v) - Fraction(o)))) / Fraction(res)) for v in Y]
        assert (cells_x[0], cells_y[0]) == (cx, cy)
        mine = cells_x if coord == "X" else cells_y
        assert mine[1] != mine[0] or mine[2] != mine[0], n
        assert all(abs(m - mine[0]) <= 1 for m in mine)            # an FMA moves it to the neighbouring cell
        for f in (0, 1):
            moved[(coord, f)] += mine[f + 1] != mine[0]
        # the restatement takes the three-rounding cell: 2 in the centre, the reference's cell
        q, r, centre = case.pair(n)
        assert tuple(q[0]) == (x, y) and tuple(centre) == (th, tx0, ty0)
        assert (plain_cell(float(r[0, 0]), o, res), plain_cell(float(r[0, 1]), o, res)) == (cx, cy)
        assert case.ref[0][n, 0, 1, 1] == 2 and case.ref[0][n].tolist() == [cc.CONTRACT_VOLUME]
    assert all(v >= 3 for v in moved.values()), moved        # either product kept exact, either coordinate


# ----------------------------------------------------------------------------- saturation

def test_saturation_case_crosses_16_bits_beside_a_zero():
    c = cc.saturation_case()
    vol, _, score, _ = c.ref
    assert cc.SATURATION_N == (1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 40000)
    assert {n - cc.TILE for n in cc.SATURATION_N} >= {-1, 0, 1} and {n - 2 * cc.TILE for n in cc.SATURATION_N} >= {0, 1}
    assert vol.max() == 80000 > 2 ** 16 and 2 * cc.TILE < 2 ** 16
    for b, n in enumerate(np.repeat(cc.SATURATION_N, 2)):
        one = np.array(cc.SATURATION_ONE[3 if b % 2 == 0 else 4])
        assert len(c.pair(b)[0]) == n and np.array_equal(vol[b, 0], n * one) and score[b] == 2 * n
    # the dwords of an 8-column row are columns 0..3 and 4..7; a dword adds columns (0, 2) and (1, 3) as 16-bit pairs
    for one in cc.SATURATION_ONE.values():
        pairs = [(row[d + a], row[d + a + 2]) for row in one for d in (0, 4) for a in (0, 1)]
        assert (2, 0) in pairs or (0, 2) in pairs
        assert (1, 0) in pairs or (0, 1) in pairs
    assert cc.SATURATION_ONE[3][0][:4] == [0, 2, 1, 0] and cc.SATURATION_ONE[4][0][:4] == [2, 1, 0, 0]


# ----------------------------------------------------------------------------------- ties

def test_tie_cases_tie_where_they_claim():
    def maxima(c, b=0):
        vol = c.ref[0][b]
        return [tuple(int(v) for v in a) for a in np.argwhere(vol == vol.max())]
    c = cc.tie_small_case()
    assert maxima(c, 0) == [(0, 2, 1), (0, 2, 5)] and maxima(c, 1) == [(0, 0, 3), (0, 4, 3)]
    assert maxima(c, 2) == [(0, 1, 5), (0, 3, 1)]
    assert maxima(cc.tie_angle_case()) == [(0, 1, 1), (2, 1, 1)]
    c = cc.tie_wave_case()
    assert maxima(c, 0) == [(0, 1, 3), (0, 10, 7)] and maxima(c, 1) == [(0, 3, 4), (0, 9, 12)]
    assert cc.host_shape(32, 16, 1) == (512, 1, 2) and cc.host_shape(32, 16, 4) == (128, 1, 1)
    wave = {1: lambda j, i: (j * 32 + i) % 256 // 64, 4: lambda j, i: (j * 8 + i // 4) // 64}
    assert [wave[1](*m) for m in ((1, 3), (10, 7), (3, 4), (9, 12))] == [0, 1, 1, 0]
    assert [wave[4](*m) for m in ((1, 3), (10, 7), (3, 4), (9, 12))] == [0, 1, 0, 1]
    c = cc.tie_pass_case()
    assert maxima(c) == [(0, 2, 5), (0, 1097, 1)]
    assert cc.host_shape(8, 1100, 1) == (8800, 3, 12) and cc.host_shape(8, 1100, 4) == (2200, 2, 5)
    for w, per_row in ((1, 8), (4, 2)):
        _, passes, R = cc.host_shape(8, 1100, w)
        assert (2 * per_row) // (cc.BLOCK * R) == 0 and (1097 * per_row) // (cc.BLOCK * R) == passes - 1


# ---------------------------------------------------------------------------- empty scans

def test_empty_case_is_what_it_claims():
    c = cc.empty_case()
    pts, off = c.packed()
    assert off.tolist() == [0, 25, 25, 55, 55, 80] and pts.shape == (80, 2)
    vol, index, score, _ = c.ref
    kinds = [k for k, _, _ in cc.EMPTY_PAIRS]
    assert kinds[0] == kinds[-1] == "ordinary" and {"empty query", "empty reference", "both empty"} <= set(kinds)
    for b, (kind, s, d) in enumerate(cc.EMPTY_PAIRS):
        if "empty" in kind:
            assert not vol[b].any() and score[b] == 0 and tuple(index[b]) == (0, 0, 0)
            assert kinds[b - 1] in ("ordinary", "scan against itself") and "empty" not in kinds[b + 1]
        else:
            assert score[b] > 0
        if kind == "scan against itself":
            assert s == d and len(c.scans[s]) > 0


# ------------------------------------------------------------------------- instance sweep

def test_dispatch_restatement():
    assert cc.host_shape(1, 1, 1) == (1, 1, 1) and cc.host_shape(1, 1, 4) == (1, 1, 1)
    assert cc.host_shape(61, 61, 1) == (3721, 1, 15) and cc.host_shape(61, 61, 4) == (976, 1, 4)
    assert cc.host_shape(1, 4096, 1) == (4096, 1, 16) and cc.host_shape(1, 4097, 1) == (4097, 2, 9)
    assert cc.host_shape(1, 2048, 4) == (2048, 1, 8) and cc.host_shape(1, 2049, 4) == (2049, 2, 5)
    assert cc.host_shape(5, 128, 4) == (256, 1, 1) and cc.host_shape(5, 129, 4) == (258, 1, 2)
    assert cc.host_shape(7, 5, 4) == (10, 1, 1) and cc.host_shape(50, 170, 1) == (8500, 3, 12)
    # the windows of tests/test_csm_gpu.py's exact-volume tests: R = 1, 5 (dwords) and 1, 12 (bytes) only
    old = [(7, 5), (8, 6), (50, 170)]
    assert {cc.host_shape(nx, ny, 4)[2] for nx, ny in old} == {1, 5}
    assert {cc.host_shape(nx, ny, 1)[2] for nx, ny in old} == {1, 12}
    for nx, ny in cc.sweep_windows() + cc.MULTI_PASS:
        for w in cc.WIDTHS:
            nslot, passes, R = cc.host_shape(nx, ny, w)
            assert 1 <= R <= cc.MAX_R[w] and cc.BLOCK * R * (passes - 1) < nslot <= cc.BLOCK * R * passes


def test_sweep_covers_every_instance_at_both_fill_levels():
    single, multi = cc.sweep_coverage()
    for w in cc.WIDTHS:
        for R in range(1, cc.MAX_R[w] + 1):
            assert (w, R, "full") in single and (w, R, "barely") in single, (w, R)
        assert (w, 2) in multi and (w, 3) in multi
    assert cc.DEFAULT_WINDOW in cc.sweep_windows() and len(set(cc.sweep_windows())) == len(cc.sweep_windows()) == 52
    c = cc.sweep_case(*cc.DEFAULT_WINDOW)
    assert (c.params["G"], c.params["res"], c.params["n_theta"]) == (512, 0.05, 8)


@pytest.mark.parametrize("nx,ny", cc.sweep_windows(), ids=["%dx%d" % w for w in cc.sweep_windows()])
def test_sweep_window_scores_in_its_first_and_last_slots(nx, ny):
    """The reference volume is non-zero among the shifts of the first 256 slots of the launch
    and among those of the last group (the last pass of a multi-pass window), under both gather
    widths; scans of 100 to 300 points; and the restatement equals the plain loops on a cut of
    the case (one angle, 8 query points: the tall windows cost the loops too much in full)."""
    c = cc.sweep_case(nx, ny)
    assert all(100 <= len(s) <= 300 for s in c.scans)
    vol = c.ref[0]
    for w in cc.WIDTHS:
        for group in (0, -1):
            j0, j1 = cc.slot_rows(nx, ny, w, group)
            assert 0 <= j0 <= j1 < ny
            for b in range(len(vol)):
                assert vol[b, :, j0:j1 + 1].any(), (w, group, b, j0, j1)
        nslot, passes, R = cc.host_shape(nx, ny, w)
        assert (nslot - 1) // cc.BLOCK * cc.BLOCK >= cc.BLOCK * R * (passes - 1)     # the last group: the last pass
    q, r, centre = c.pair(0)
    p = dict(c.params, n_theta=1)
    S, _ = plain_volume(q[:8].tolist(), r.tolist(), centre, **p)
    assert np.array_equal(csm_ref.score_volume(q[:8], r, centre, **p)[0], np.array(S).reshape(1, ny, nx))


# ------------------------------------------------------------------ host-side offset check

def test_check_offsets_accepts_packed_scans():
    from slamhip.csm import check_offsets
    check_offsets(np.array([0, 3, 3, 7]), 7, 3)
    check_offsets(np.array([0, 3, 3, 7]), 9)              # spare points behind the last scan
    check_offsets(np.array([2, 2, 5], np.int32), 5, 2)    # spare points before the first
    check_offsets(np.array([0]), 0, 0)
    check_offsets(cc.empty_case().packed()[1], 80, 5)


@pytest.mark.parametrize("off, n_points, n_scans, word", [
    ([-1, 3, 7], 7, 2, "first"), ([0, 4, 3, 7], 7, 3, "decrease"), ([0, 3, 7, 6], 7, 3, "decrease"),
    ([0, 3, 8], 7, 2, "exceeds"), ([5, 5, 9], 4, 2, "exceeds"), ([0, 3, 7], 7, 3, "offsets for 3 scans"),
    ([0, 3, 7], 7, 1, "offsets for 1 scans"), ([], 0, None, "1-D"), ([[0, 3], [3, 7]], 7, None, "1-D"),
    ([0.0, 3.0, 7.0], 7, 2, "integer"), ([0, 2 ** 40, 7], 7, 2, "decrease")])
def test_check_offsets_refuses(off, n_points, n_scans, word):
    from slamhip.csm import check_offsets
    with pytest.raises(ValueError, match=word):
        check_offsets(np.array(off), n_points, n_scans)


def test_csm_batch_checks_the_offsets_before_any_launch():
    """A scan set whose offsets are bad never reaches the library: ``_abi.lib`` is not asked for."""
    from slamhip.csm import csm_batch
    from slamhip.icp import ScanSet
    for off, word in (([0, 3, 8], "exceeds"), ([0, 4, 3], "decrease"), ([-2, 3, 7], "first"), ([0, 7], "offsets for")):
        ss = ScanSet.__new__(ScanSet)      # as plicp.packed_scans builds one, without the uploads
        ss.off, ss.lens, ss.host_pts = np.array(off, np.int64), np.array([3, 4]), np.zeros((7, 2))
        ss.pts = ss.scan_off = ss.device = None
        with pytest.raises(ValueError, match=word):
            csm_batch(ss, [0], [1])
