"""GPU parity of the localisation kernels (csrc/loc_kernels.hip) on every field,
search and refinement edge, against the NumPy restatement (tests/loc_ref.py).

tests/test_loc_gpu.py runs seeded maps and one 111-point refinement; here the
cases of tests/loc_cases.py put inputs on the positions the kernels distinguish:
one occupied cell on either side of every 128-row band and 256-column block
edge and d_cap - 1, d_cap and d_cap + 1 away from it, the d_cap = 255 halo over
two neighbouring blocks; a window for each of the eight loc_search_kernel<R>,
one and two passes, both table widths and the guard between them (d_cap 15 and
16), a table filled on the second trip of loc_table_kernel's loop, scans on
either side of the LDS tile, points whose coordinates overflow, windows wider
than the map; refinements of 1 to 1,000 points, each of the three pivot exits,
the inclusive cell bounds, the cap skip, the inlier fraction at equality, the
iteration limit, TOO_FEW and SINGULAR after a step; the device-side bounds flag
(g_loc_bad_query) through the C ABI; repeats, batch order and a side stream.
tests/test_loc_cases.py shows on the CPU that the inputs are what they claim.

Bounds: the field, the cost volumes and the best bins bit for bit.  The
refinement's iterations, inliers and statuses equal, its poses and rms to 1e-9
(tests/test_loc_gpu.py's ``_same``); where no step is taken the pose is the start
pose bit for bit.

Measured on an MI355X: the 68 tests of this file take 2.3 to 2.8 s together, the
largest single one (the first to touch the device) 0.16 s, the 1,000 x 1,100
map 0.02 s.  Every refinement case (run with -s for its LOC-DIFF line) gives
the restatement's status, iterations and inliers; the largest pose difference
is 1.7e-16 (SINGULAR after a step), every other one at most 9e-19.

Mutation check (scratch builds, never committed; each value-only edit of
csrc/loc_kernels.hip built and run once, the tests of this file that fail):
  g.cap2 <= 255 -> <= 256              test_search_byte_table_guard[16]
  fu <= umax -> fu < umax              test_refine_inclusive_cell_bounds, test_refine_status_after_a_step
  s[10] < min_inlier_frac n -> <=      test_refine_inlier_fraction_at_equality, test_refine_status_after_a_step
  column sweep from r0 - d_cap -> r0   test_field_one_cell_at_every_band_edge[2, 20, 127, 128, 129],
                                       test_field_grid_shapes[129x3, 257x3]
  table fill: stride loop -> one if    test_search_table_fill_beyond_one_sweep[2, 1]
  cap skip && -> ||                    test_refine_cap_skip_needs_all_four_corners, test_refine_status_after_a_step
"""
import numpy as np
import pytest

import loc_cases as lc
import loc_ref

pytestmark = pytest.mark.gpu
ORIGIN0 = (0.0, 0.0)


# ------------------------------------------------------------------------------ field

def _field_equals(c):
    from slamhip import loc
    got = loc.LikelihoodField(c.grid, ORIGIN0, 0.25, d_cap=c.d_cap).field
    assert got.dtype == np.uint16 and got.shape == c.grid.shape
    assert np.array_equal(got, c.ref), (c.name, np.argwhere(got != c.ref)[:4])


@pytest.mark.parametrize("n", range(len(lc.SHAPES)), ids=["%dx%d" % s for s in lc.SHAPES])
def test_field_grid_shapes(n):
    _field_equals(lc.shape_cases()[n])


@pytest.mark.parametrize("d_cap", lc.EDGE_CAPS)
def test_field_one_cell_at_every_band_edge(d_cap):
    for c in lc.band_cells(d_cap):
        _field_equals(c)


@pytest.mark.parametrize("d_cap", lc.EDGE_CAPS)
def test_field_one_cell_at_every_block_edge(d_cap):
    for c in lc.block_cells(d_cap):
        _field_equals(c)


def test_field_halo_of_255_over_two_blocks():
    _field_equals(lc.halo_case())


# ----------------------------------------------------------------------------- search

def _search_equals(c, width=2):
    """The case's batch with the table's entries ``width`` bytes wide (width 1 is a
    request: the library keeps 2 where d_cap^2 does not fit a byte)."""
    from slamhip import _abi, loc
    f = loc.LikelihoodField(c.grid, c.origin, c.cw, d_cap=c.d_cap)
    assert np.array_equal(f.field, c.F)
    L = _abi.lib()
    assert L.slam_loc_set_table(width) == 0
    try:
        r = loc.search(f, c.scans, c.idx, c.centre, loc.LocParams(**c.window), return_costs=True)
    finally:
        assert L.slam_loc_set_table(2) == 0
    vol, index, cost = c.ref
    assert r.costs.dtype == np.int32 and r.costs.shape == vol.shape
    assert np.array_equal(r.costs, vol), (c.name, width, np.argwhere(r.costs != vol)[:4])
    assert np.array_equal(r.index, index) and np.array_equal(r.cost, cost)
    return r


@pytest.mark.parametrize("width", [2, 1])
@pytest.mark.parametrize("nx,ny", list(lc.R_SHAPES), ids=["%dx%d" % s for s in lc.R_SHAPES])
def test_search_every_instantiation(nx, ny, width):
    _search_equals(lc.r_case(nx, ny), width)


@pytest.mark.parametrize("d_cap", lc.GUARD_CAPS)
def test_search_byte_table_guard(d_cap):
    """d_cap = 15: bytes, the largest entry 225.  d_cap = 16: 256 does not fit; the
    request for bytes must fall back to 16-bit entries."""
    c = lc.guard_case(d_cap)
    _search_equals(c, 1)
    _search_equals(c, 2)


@pytest.mark.parametrize("width", [2, 1])
def test_search_table_fill_beyond_one_sweep(width):
    _search_equals(lc.big_case(), width)


def test_search_scans_around_the_lds_tile():
    _search_equals(lc.tile_case())


def test_search_points_that_overflow_are_outside_the_map():
    c = lc.extreme_case()
    for width in (2, 1):
        r = _search_equals(c, width)
        assert np.array_equal(r.costs[0], r.costs[1] + 3 * c.d_cap ** 2)


@pytest.mark.parametrize("step,nx,ny", lc.WIDE_WINDOWS)
def test_search_window_wider_than_the_map(step, nx, ny):
    _search_equals(lc.wide_case(step, nx, ny))


# ------------------------------------------------------------------------- refinement

def _same(got, b, want):
    assert got.iters[b] == want["iters"] and got.inliers[b] == want["inliers"] and got.status[b] == want["status"]
    assert np.abs(got.poses[b] - want["pose"]).max() <= 1e-9
    assert np.isnan(want["rms"]) and np.isnan(got.rms[b]) or abs(got.rms[b] - want["rms"]) <= 1e-9


def _refine_equals(c):
    """Every query of the case, one launch per set of parameters; {query name: (result, row)}."""
    from slamhip import loc
    f = loc.LikelihoodField(c.grid, c.origin, c.cw, d_cap=c.d_cap)
    assert np.array_equal(f.field, c.F)
    out = {}
    for params, which in c.launches():
        qs = [c.queries[n] for n in which]
        got = loc.refine(f, [q.pts for q in qs], np.arange(len(qs)), np.array([q.start for q in qs]),
                         loc.LocParams(**params))
        for b, n in enumerate(which):
            want = c.ref[n]
            print("\nLOC-DIFF %s %s: status %d/%d iters %d/%d inliers %d/%d pose %.2e" % (
                c.name, qs[b].name, got.status[b], want["status"], got.iters[b], want["iters"], got.inliers[b],
                want["inliers"], np.abs(got.poses[b] - want["pose"]).max()))
            _same(got, b, want)
            if want["iters"] == 0:
                assert got.poses[b].tobytes() == qs[b].start.tobytes()
            out[qs[b].name] = (got, b)
    return out


def test_refine_scan_sizes_around_the_block():
    out = _refine_equals(lc.size_case())
    assert len(out) == len(lc.SIZES)


def test_refine_iteration_limit_converged_wins():
    out = _refine_equals(lc.limit_case())
    (full, b0), (short, b1) = out["N"], out["N-1"]
    assert full.status[b0] == loc_ref.CONVERGED and short.status[b1] == loc_ref.MAX_ITERS
    assert full.iters[b0] == short.iters[b1] + 1


@pytest.mark.parametrize("n", range(3), ids=lc.PIVOTS)
def test_refine_each_pivot_exit(n):
    c = lc.pivot_case()[n]
    got, b = _refine_equals(c)[lc.PIVOTS[n]]
    assert (got.status[b], got.iters[b]) == (loc_ref.SINGULAR, 0)


def test_refine_inclusive_cell_bounds():
    out = _refine_equals(lc.bounds_case())
    for name, (_, inside) in lc.BOUNDS.items():
        got, b = out[name]
        assert got.inliers[b] == 8 + inside, name
    assert out["all-in"][0].inliers[out["all-in"][1]] == 16 and out["all-out"][0].inliers[out["all-out"][1]] == 8


def test_refine_cap_skip_needs_all_four_corners():
    got, b = _refine_equals(lc.cap_case())["cap"]
    assert got.inliers[b] == len(lc.THREE_AT_CAP) + len(lc.CAP_ORDINARY) == 12


def test_refine_inlier_fraction_at_equality():
    out = _refine_equals(lc.fraction_case())
    for f, too_few in lc.FRACTIONS:
        got, b = out["frac=%r" % f]
        assert (got.status[b] == loc_ref.TOO_FEW) == too_few and got.inliers[b] == 4, f


def test_refine_status_after_a_step():
    too_few, singular = lc.after_step_case()
    got, b = _refine_equals(too_few)["too-few"]
    assert (got.status[b], got.iters[b], got.inliers[b]) == (loc_ref.TOO_FEW, 1, 8)
    got, b = _refine_equals(singular)["singular"]
    assert (got.status[b], got.iters[b], got.inliers[b]) == (loc_ref.SINGULAR, 1, 40)


# ----------------------------------------------------------- the device-side bounds flag

class Raw:
    """slam_loc_search and slam_loc_refine_f64 called as slamhip/loc.py calls them, but with
    whatever scan indices, offsets, S, P and max_n the test passes: the Python wrappers
    validate all of them before a launch and cannot reach the device-side check."""

    WINDOW = dict(n_theta=3, d_theta=0.05, nx=5, ny=4, step=1)

    def __init__(self):
        from slamhip import _abi, loc
        from slamhip import device as dv
        self.L, self.dv, self.abi = _abi.lib(), dv, _abi
        g, origin, cw, d_cap, pts, truth = loc_ref.refine_case()
        self.f = loc.LikelihoodField(g, origin, cw, d_cap=d_cap)
        self.truth = truth
        # scan 1 is the longest; scan 2 is used by no query, so the offset between 1 and 2 is free to be wrong
        self.scans = [pts[:40], pts, pts[5:25], pts[30:100], pts[50:111]]
        self.lens = np.array([len(s) for s in self.scans])
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.pts = dv.to_dev(np.concatenate(self.scans), np.float64, self.f.device)
        self.starts = truth + np.array([(0.03, -0.02, 0.01), (0.05, 0.04, -0.02), (-0.04, 0.02, 0.015),
                                        (0.02, 0.05, -0.01)])

    def run(self, q_scan, rows, off=None, S=None, P=None, max_n=None):
        """(search best (B, 4), search costs (B, ...), refinement outputs as one dict) of the
        queries (scan q_scan[b], start pose rows[b]); the status flag is left for the caller."""
        from slamhip import loc
        from slamhip.csm import rotations
        dv, L, f = self.dv, self.L, self.f
        dev = f.device
        B = len(q_scan)
        off = self.off if off is None else np.asarray(off, np.int64)
        S = len(self.scans) if S is None else S
        P = int(self.off[-1]) if P is None else P
        max_n = int(self.lens.max()) if max_n is None else max_n
        assert len(off) == S + 1 or S != len(self.scans)      # the kernel reads scan_off[s] and [s + 1] for s < S only
        p = loc.LocParams(**self.WINDOW)
        starts = self.starts[rows]
        centre = np.ascontiguousarray(starts[:, [2, 0, 1]])
        d_off = dv.to_dev(off, np.int64, dev)
        d_idx = dv.to_dev(np.asarray(q_scan), np.int32, dev)
        d_centre = dv.to_dev(centre, np.float64, dev)
        d_rot = dv.to_dev(rotations(centre, p), np.float64, dev)
        n_work = int(L.slam_loc_search_work_size(B, f.H, f.W, p.n_theta, p.ny, p.nx, p.step))
        assert n_work > 0
        work = dv.empty((n_work,), np.uint8, dev)
        best = dv.empty((B, 4), np.int32, dev)
        costs = dv.empty((B, p.n_theta, p.ny, p.nx), np.int32, dev)
        h = dv.stream_handle(None)
        margs = (dv.ptr(f.dev), f.H, f.W, float(f.origin[0]), float(f.origin[1]), f.cell_width, f.d_cap)
        assert L.slam_loc_search(*margs, dv.ptr(self.pts), dv.ptr(d_off), S, P, dv.ptr(d_idx), dv.ptr(d_centre),
                                 dv.ptr(d_rot), B, max_n, p.n_theta, p.nx, p.ny, p.step, dv.ptr(best), dv.ptr(costs),
                                 dv.ptr(work), h) == 0
        out_pose, out_rms = dv.empty((B, 3), np.float64, dev), dv.empty((B,), np.float64, dev)
        out_inl, out_it, out_st = (dv.empty((B,), np.int32, dev) for _ in range(3))
        assert L.slam_loc_refine_f64(*margs, dv.ptr(self.pts), dv.ptr(d_off), S, P, dv.ptr(d_idx), dv.ptr(d_centre), B,
                                     max_n, 30, 1e-4, 1e-4, 0.5, 1e-9, dv.ptr(out_pose), dv.ptr(out_rms),
                                     dv.ptr(out_inl), dv.ptr(out_it), dv.ptr(out_st), h) == 0
        self.dv.torch().cuda.synchronize()
        ref = dict(pose=out_pose.cpu().numpy(), rms=out_rms.cpu().numpy(), inliers=out_inl.cpu().numpy(),
                   iters=out_it.cpu().numpy(), status=out_st.cpu().numpy(), init=centre)
        return best.cpu().numpy(), costs.cpu().numpy(), ref

    def status(self):
        return self.L.slam_loc_status(self.dv.stream_handle(None))


@pytest.fixture(scope="module")
def raw():
    r = Raw()
    assert r.status() == 0
    return r


def _row_bytes(best, costs, ref, b):
    return b"".join(np.ascontiguousarray(a[b]).tobytes() for a in
                    (best, costs, ref["pose"], ref["rms"], ref["inliers"], ref["iters"], ref["status"]))


def _bad_launches(raw):
    """name -> the arguments of a launch whose query 1 (scan 1) is outside its bounds."""
    S, P = len(raw.scans), int(raw.off[-1])
    descends, past = raw.off.copy(), raw.off.copy()
    descends[2] = raw.off[1] - 1            # scan 1 ends before it begins
    past[2] = P + 1                         # scan 1 ends past the points
    longest_good = int(raw.lens[[0, 3, 4]].max())
    assert raw.lens[1] > longest_good
    return {"scan index -1": dict(q_scan=[0, -1, 3, 4]), "scan index S": dict(q_scan=[0, S, 3, 4]),
            "offsets descend": dict(q_scan=[0, 1, 3, 4], off=descends),
            "offsets end past P": dict(q_scan=[0, 1, 3, 4], off=past),
            "longer than max_n": dict(q_scan=[0, 1, 3, 4], max_n=longest_good)}


@pytest.mark.parametrize("kind", ["scan index -1", "scan index S", "offsets descend", "offsets end past P",
                                  "longer than max_n"])
def test_bad_query_is_flagged_and_neighbours_are_unaffected(raw, kind):
    kw = _bad_launches(raw)[kind]
    good = raw.run([0, 3, 4], [0, 2, 3], max_n=kw.get("max_n"))
    assert raw.status() == 0
    assert set(good[2]["status"]) <= {loc_ref.CONVERGED, loc_ref.MAX_ITERS} and np.all(good[0] >= 0)
    best, costs, ref = raw.run(rows=[0, 1, 2, 3], **kw)
    assert raw.status() == -1 and b"outside" in raw.L.slam_last_error()       # once ...
    assert raw.status() == 0                                                  # ... and cleared
    assert tuple(best[1]) == (-1, -1, -1, -1)
    assert (ref["status"][1], ref["iters"][1], ref["inliers"][1]) == (-1, 0, 0) and np.isnan(ref["rms"][1])
    assert ref["pose"][1].tobytes() == ref["init"][1].tobytes()
    for b, g in ((0, 0), (2, 1), (3, 2)):
        assert _row_bytes(best, costs, ref, b) == _row_bytes(*good, g), (kind, b)


def test_empty_scan_is_within_bounds(raw):
    """scan_off[2] == scan_off[3]: a scan of no points (the Python wrappers refuse one).  The
    search sums nothing: cost 0, the first bin; the refinement has no inlier: TOO_FEW."""
    off = raw.off.copy()
    off[2] = off[3]
    good = raw.run([0, 3, 4], [0, 2, 3])
    best, costs, ref = raw.run([0, 2, 3, 4], [0, 1, 2, 3], off=off)
    assert raw.status() == 0                                                  # nothing is flagged
    assert tuple(best[1]) == (0, 0, 0, 0) and np.all(costs[1] == 0)
    assert (ref["status"][1], ref["iters"][1], ref["inliers"][1]) == (loc_ref.TOO_FEW, 0, 0) and np.isnan(ref["rms"][1])
    assert ref["pose"][1].tobytes() == ref["init"][1].tobytes()
    for b, g in ((0, 0), (2, 1), (3, 2)):
        assert _row_bytes(best, costs, ref, b) == _row_bytes(*good, g), b
    g, origin, cw, d_cap, pts, truth = loc_ref.refine_case()
    want = loc_ref.refine(loc_ref.field(g, d_cap), origin, cw, d_cap, np.zeros((0, 2)), raw.starts[1])
    assert (want["status"], want["iters"], want["inliers"]) == (loc_ref.TOO_FEW, 0, 0) and np.isnan(want["rms"])


# ------------------------------------------------------------- determinism and streams

def _batch():
    """Twelve queries on the refine_case map: every cut of the cloud from 255 points up,
    two starts each, the windows of the search one pass of R = 2."""
    from slamhip import loc
    g, origin, cw, d_cap, _, truth = loc_ref.refine_case()
    scans = [lc.cloud()[:n] for n in lc.SIZES[2:]]
    idx = np.arange(12) % len(scans)
    rng = np.random.default_rng(17)
    starts = truth + rng.uniform(-1.0, 1.0, size=(12, 3)) * (0.08, 0.08, 0.025)
    p = loc.LocParams(n_theta=5, d_theta=0.02, nx=19, ny=17, step=1)
    return (g, origin, cw, d_cap), scans, idx, starts, p


def _bytes(s, r, rows=slice(None)):
    return b"".join(np.ascontiguousarray(a[rows]).tobytes() for a in
                    (s.costs, s.index, s.cost, s.poses, r.poses, r.iters, r.inliers, r.status, r.rms))


def _run(field, scans, idx, starts, p, stream=None):
    from slamhip import loc
    s = loc.search(field, scans, idx, starts[:, [2, 0, 1]], p, return_costs=True, stream=stream)
    r = loc.refine(field, scans, idx, starts, p, stream=stream)
    return s, r


def test_repeat_and_batch_position():
    from slamhip import loc
    m, scans, idx, starts, p = _batch()
    f = loc.LikelihoodField(*m[:3], d_cap=m[3])
    a = _run(f, scans, idx, starts, p)
    assert set(a[1].status) <= {loc_ref.CONVERGED, loc_ref.MAX_ITERS}
    assert _bytes(*a) == _bytes(*_run(f, scans, idx, starts, p))
    perm = np.random.default_rng(23).permutation(len(idx))
    assert not np.array_equal(perm, np.arange(len(idx)))
    b = _run(f, scans, idx[perm], starts[perm], p)
    assert _bytes(*b) == _bytes(*a, rows=perm)


def test_side_stream_gives_the_default_streams_bytes():
    from slamhip import loc
    from slamhip import device as dv
    t = dv.torch()
    m, scans, idx, starts, p = _batch()
    f = loc.LikelihoodField(*m[:3], d_cap=m[3])
    a = _run(f, scans, idx, starts, p)
    side = t.cuda.Stream()
    assert side.cuda_stream != t.cuda.current_stream().cuda_stream
    f2 = loc.LikelihoodField(*m[:3], d_cap=m[3], stream=side)
    assert f2.field.tobytes() == f.field.tobytes()
    b = _run(f2, scans, idx, starts, p, stream=side)
    side.synchronize()
    assert _bytes(*b) == _bytes(*a)
