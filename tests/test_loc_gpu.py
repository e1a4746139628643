"""Localisation in a finished occupancy grid on the GPU (slamhip.loc,
csrc/loc_kernels.hip) against its NumPy restatement (tests/loc_ref.py): the
field and the search's cost volumes bit for bit, the refinement's iterations,
inliers and statuses equal and its poses to 1e-9, then the end-to-end
experiment, relocalisation with no guess and the opt-in wiring of the scripts.

The end-to-end bound is twice the restatement's own largest error on the same
inputs (loc_ref.E2E_MEASURED, re-measured by tests/test_loc.py)."""
import os
import sys

import numpy as np
import pytest

import loc_ref
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(PKG, "scripts"))


# ------------------------------------------------------------------------------ field

def _edges(H, W, v=7):
    g = np.zeros((H, W), np.int8)
    g[0, W // 3] = g[H - 1, W // 2] = g[H // 2, 0] = g[H // 3, W - 1] = v
    return g


def _corner(H, W):
    g = np.zeros((H, W), np.int8)
    g[H - 1, W - 1] = 1
    return g


def _random(H, W, seed, p=0.03):
    rng = np.random.default_rng(seed)
    g = rng.integers(-128, 1, size=(H, W)).astype(np.int8)
    g[rng.random((H, W)) < p] = rng.integers(1, 128)
    return g


def _occ_values():
    """Cells holding exactly -128, -1, 0, 1, 126 and their neighbours -127, -2, 2, 125, 127."""
    g = np.full((37, 53), -128, np.int8)
    for n, v in enumerate((-128, -127, -2, -1, 0, 1, 2, 125, 126, 127)):
        g[3 + 3 * n, 2 + 5 * n] = v
    return g


FIELD_CASES = {
    "empty": (np.zeros((37, 53), np.int8), 5, 0),
    "corner": (_corner(37, 53), 9, 0),
    "row_1x70": (_edges(1, 70), 4, 0),
    "col_65x1": (_edges(65, 1), 4, 0),
    "odd_37x53": (_random(37, 53, 1), 6, 0),
    "edges": (_edges(37, 53), 12, 0),
    "two_bands_300x270": (_random(300, 270, 2, p=0.002), 20, 0),   # more than one row band and column block
    "d_cap_1": (_random(37, 53, 3), 1, 0),
    "d_cap_above_grid": (_edges(37, 53), 100, 0),
    "d_cap_255": (_corner(300, 270), 255, 0),
    **{"occ_min_%d" % m: (_occ_values(), 7, m) for m in (-128, -1, 0, 1, 126)},
}


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_exact(name):
    from slamhip import loc
    grid, d_cap, occ_min = FIELD_CASES[name]
    got = loc.LikelihoodField(grid, (0.0, 0.0), 0.1, d_cap=d_cap, occ_min=occ_min).field
    want = loc_ref.field(grid, d_cap, occ_min)
    assert got.dtype == np.uint16 and got.shape == grid.shape
    assert np.array_equal(got, want)
    if name == "empty":
        assert np.all(got == d_cap * d_cap)
    if name.startswith("occ_min"):
        assert int((got == 0).sum()) == int((grid.astype(int) > occ_min).sum())


# ----------------------------------------------------------------------------- search

WINDOWS = {
    "odd": dict(n_theta=9, d_theta=0.05, nx=7, ny=5, step=1),
    "even": dict(n_theta=1, d_theta=0.05, nx=8, ny=6, step=3),
}
D_CAP = 6


class SearchCase:
    """Six queries over scans of 61 and 130 points on a 37 x 53 map of 0.2 m cells
    centred on the sensor: windows that hang over every map edge, a query wholly
    outside the map and a scan with a point at 1e12."""

    def __init__(self):
        from slamhip import synthetic
        a = synthetic.make_sequence(3, seed=1, n_beams=61)
        b = synthetic.make_sequence(3, seed=2, n_beams=130)
        far = a.scans[2].copy()
        far[5] = (1e12, -3.0)
        self.scans = a.scans[:2] + b.scans[:2] + [far]
        assert sorted({len(s) for s in self.scans}) == [61, 130]
        self.grid = _random(37, 53, 7, p=0.06)
        self.origin, self.cw = np.array([-5.3, -3.7]), 0.2
        self.idx = np.array([0, 2, 1, 3, 4, 2])
        # (theta0, x0, y0): inside; over the left and bottom edges; over the right edge; over the top edge;
        # the scan with the far point; wholly outside
        self.centre = np.array([[0.10, 0.30, -0.20], [-0.20, -5.25, -3.65], [0.05, 5.2, 0.35], [-0.07, -0.40, 3.6],
                                [0.31, 0.12, 0.52], [-0.33, 500.0, 500.0]])
        self.F = loc_ref.field(self.grid, D_CAP)
        self.ref = {}
        for name, w in WINDOWS.items():
            out = [loc_ref.search(self.F, self.origin, self.cw, D_CAP, self.scans[s], c, **w)
                   for s, c in zip(self.idx, self.centre)]
            vol = np.stack([o[0] for o in out])
            vol.setflags(write=False)
            self.ref[name] = (vol, np.array([o[1][1:] for o in out]), np.array([o[1][0] for o in out]))


@pytest.fixture(scope="module")
def scase():
    return SearchCase()


@pytest.fixture(scope="module")
def sfield(scase):
    from slamhip import loc
    from slamhip.icp import ScanSet
    f = loc.LikelihoodField(scase.grid, scase.origin, scase.cw, d_cap=D_CAP)
    assert np.array_equal(f.field, scase.F)
    return f, ScanSet(scase.scans, f.device)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_search_exact_volumes(scase, sfield, name):
    from slamhip import loc
    f, ss = sfield
    vol, index, cost = scase.ref[name]
    r = loc.search(f, ss, scase.idx, scase.centre, loc.LocParams(**WINDOWS[name]), return_costs=True)
    assert r.costs.dtype == np.int32 and np.array_equal(r.costs, vol)
    assert np.array_equal(r.index, index) and np.array_equal(r.cost, cost)
    # the query wholly outside the map: every cost n d_cap^2, the first bin wins the tie
    n = len(scase.scans[scase.idx[5]])
    assert np.all(r.costs[5] == n * D_CAP ** 2) and tuple(r.index[5]) == (0, 0, 0)
    w = WINDOWS[name]
    for b in range(len(scase.idx)):
        want = loc_ref.assemble(scase.centre[b], index[b], w["n_theta"], w["d_theta"], w["nx"], w["ny"], w["step"],
                                scase.cw)
        assert np.array_equal(r.poses[b], want)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_search_query_alone_equals_its_batch_row(scase, sfield, name):
    from slamhip import loc
    f, ss = sfield
    vol, index, cost = scase.ref[name]
    for b in range(len(scase.idx)):
        r = loc.search(f, ss, scase.idx[b:b + 1], scase.centre[b:b + 1], loc.LocParams(**WINDOWS[name]),
                       return_costs=True)
        assert np.array_equal(r.costs[0], vol[b]) and np.array_equal(r.index[0], index[b]) and r.cost[0] == cost[b]


@pytest.mark.parametrize("name", list(WINDOWS))
def test_search_byte_table_gives_the_same_volumes(scase, sfield, name):
    """d_cap = 6 <= 15: the 1-byte table holds the field; no shape changes the result."""
    from slamhip import _abi, loc
    f, ss = sfield
    L = _abi.lib()
    assert L.slam_loc_set_table(1) == 0
    try:
        r = loc.search(f, ss, scase.idx, scase.centre, loc.LocParams(**WINDOWS[name]), return_costs=True)
    finally:
        assert L.slam_loc_set_table(2) == 0
    assert np.array_equal(r.costs, scase.ref[name][0]) and np.array_equal(r.index, scase.ref[name][1])


def test_search_many_shifts_per_thread(scase, sfield):
    """A window of 23 x 25 shifts: three shifts per thread, the last ones idle."""
    from slamhip import loc
    f, ss = sfield
    w = dict(n_theta=2, d_theta=0.3, nx=25, ny=23, step=2)
    r = loc.search(f, ss, scase.idx[:2], scase.centre[:2], loc.LocParams(**w), return_costs=True)
    for b in range(2):
        vol, best = loc_ref.search(scase.F, scase.origin, scase.cw, D_CAP, scase.scans[scase.idx[b]], scase.centre[b],
                                   **w)
        assert np.array_equal(r.costs[b], vol) and (r.cost[b],) + tuple(r.index[b]) == best


def test_search_empty_map_is_all_ties(scase):
    from slamhip import loc
    f = loc.LikelihoodField(np.zeros((37, 53), np.int8), scase.origin, scase.cw, d_cap=D_CAP)
    for name, w in WINDOWS.items():
        r = loc.search(f, scase.scans, scase.idx, scase.centre, loc.LocParams(**w), return_costs=True)
        n = np.array([len(scase.scans[s]) for s in scase.idx])
        assert np.all(r.costs == (n * D_CAP ** 2)[:, None, None, None])
        assert np.all(r.index == 0) and np.array_equal(r.cost, n * D_CAP ** 2)


def test_score_poses_is_the_single_bin_cost(scase, sfield):
    from slamhip import loc
    f, ss = sfield
    poses = scase.centre[:5][:, [1, 2, 0]]
    cost, mean = loc.score_poses(f, ss, poses)
    for s in range(5):
        _, best = loc_ref.search(scase.F, scase.origin, scase.cw, D_CAP, scase.scans[s], scase.centre[s], 1, 0.0, 1, 1, 1)
        assert cost[s] == best[0] and mean[s] == best[0] / len(scase.scans[s])


def test_scan_too_large_for_int32_costs_is_refused(scase):
    """n d_cap^2 >= 2^31: ValueError from Python, SLAM_EINVAL from the library."""
    from slamhip import _abi, loc
    f = loc.LikelihoodField(scase.grid, scase.origin, scase.cw, d_cap=255)
    big = np.zeros((33027, 2))   # 33,027 x 65,025 = 2^31 + 27
    with pytest.raises(ValueError, match="31 bits"):
        loc.search(f, [big], [0], [[0.0, 0.0, 0.0]])
    L = _abi.lib()
    one = 1   # any non-null pointer: the size check comes before the arrays are touched
    rc = L.slam_loc_search(one, 37, 53, 0.0, 0.0, 0.2, 255, one, one, 1, 33027, one, one, one, 1, 33027, 1, 1, 1, 1,
                           one, None, one, None)
    assert rc == -1 and b"31 bits" in L.slam_last_error()


# ------------------------------------------------------------------------- refinement

def _same(got, b, want):
    assert got.iters[b] == want["iters"] and got.inliers[b] == want["inliers"] and got.status[b] == want["status"]
    assert np.abs(got.poses[b] - want["pose"]).max() <= 1e-9
    assert np.isnan(want["rms"]) and np.isnan(got.rms[b]) or abs(got.rms[b] - want["rms"]) <= 1e-9


def test_refine_statuses_against_the_restatement():
    from slamhip import loc
    grid, origin, cw, d_cap, pts, truth = loc_ref.refine_case()
    F = loc_ref.field(grid, d_cap)
    f = loc.LikelihoodField(grid, origin, cw, d_cap=d_cap)
    one = np.array([[1.0, 0.2]])
    scans = [pts, one]
    starts = np.array([truth + (0.03, -0.02, 0.01), truth + (0.08, 0.06, -0.03), truth + (50.0, 50.0, 0.0), truth])
    idx = np.array([0, 0, 0, 1])
    got = loc.refine(f, scans, idx, starts)
    want = [loc_ref.refine(F, origin, cw, d_cap, scans[s], p) for s, p in zip(idx, starts)]
    assert [w["status"] for w in want] == [loc_ref.CONVERGED, loc_ref.CONVERGED, loc_ref.TOO_FEW, loc_ref.SINGULAR]
    for b, w in enumerate(want):
        _same(got, b, w)
    assert np.array_equal(got.poses[2], starts[2]) and np.array_equal(got.poses[3], starts[3])
    assert loc_ref.pose_error(got.poses[:2], truth)[0].max() < 1e-6
    # the iteration limit
    got1 = loc.refine(f, scans, idx[:2], starts[:2], loc.LocParams(max_iters=1))
    for b in range(2):
        w = loc_ref.refine(F, origin, cw, d_cap, pts, starts[b], max_iters=1)
        assert w["status"] == loc_ref.MAX_ITERS
        _same(got1, b, w)
    # a query alone equals its row of the batch, bit for bit: the order of the sums is fixed
    alone = loc.refine(f, scans, idx[1:2], starts[1:2])
    assert np.array_equal(alone.poses[0], got.poses[1]) and alone.rms[0] == got.rms[1]


# ------------------------------------------------------------------------- end to end

class E2E:
    def __init__(self):
        import src.produce_occupancy_grid as pog
        from slamhip import loc
        from slamhip.icp import ScanSet
        self.seq, map_idx, self.held, self.guess = loc_ref.e2e_inputs()
        cw = loc_ref.E2E["cell_width"]
        grid, origin = pog.produce_occupancy_grid(self.seq.truth[map_idx], [self.seq.scans[i] for i in map_idx], cw)
        with np.load(os.path.join(GOLDEN, "loc_e2e_map.npz")) as z:   # the map the bound was measured on
            assert np.array_equal(grid, z["grid"]) and np.array_equal(np.asarray(origin), z["origin"])
        self.origin, self.cw, self.d_cap = np.asarray(origin), cw, loc_ref.E2E["d_cap"]
        self.field = loc.LikelihoodField(grid, origin, cw, d_cap=self.d_cap)
        self.F = loc_ref.field(grid, self.d_cap)
        assert np.array_equal(self.field.field, self.F)
        self.scans = ScanSet(self.seq.scans[:self.seq.per_lap], self.field.device)
        self.params = loc.LocParams(**{k: loc_ref.E2E[k] for k in ("n_theta", "d_theta", "nx", "ny", "step")})


@pytest.fixture(scope="module")
def e2e():
    return E2E()


def test_end_to_end_tracking(e2e):
    from slamhip import loc
    assert len(e2e.held) == 18
    r = loc.localize(e2e.field, e2e.scans, e2e.held, e2e.guess, e2e.params)
    want = [loc_ref.localize(e2e.F, e2e.origin, e2e.cw, e2e.d_cap, e2e.seq.scans[s], g)[0]
            for s, g in zip(e2e.held, e2e.guess)]
    assert np.array_equal(r.search.index, np.array([w[1:] for w in want]))
    assert np.array_equal(r.search.cost, np.array([w[0] for w in want]))
    ep, et = loc_ref.pose_error(r.poses, e2e.seq.truth[e2e.held])
    print("tracking: largest error %.5f m, %.6f rad; bound %.5f m, %.6f rad" % ((ep.max(), et.max()) + loc_ref.E2E_BOUND))
    assert np.all(np.isin(r.refine.status, (loc.CONVERGED, loc.MAX_ITERS)))   # no scan is left out
    assert np.all(ep <= loc_ref.E2E_BOUND[0]), ep
    assert np.all(et <= loc_ref.E2E_BOUND[1]), et


def test_relocalisation_without_a_guess(e2e):
    from slamhip import loc
    scans = np.array(loc_ref.RELOC_SCANS)
    r = loc.relocalize(e2e.field, e2e.scans, scans, loc.LocParams(**loc_ref.RELOC))
    ep, et = loc_ref.pose_error(r.poses, e2e.seq.truth[scans])
    print("relocalisation: errors", ep, et)
    assert np.all(np.isin(r.refine.status, (loc.CONVERGED, loc.MAX_ITERS)))
    assert np.all(ep <= loc_ref.E2E_BOUND[0]) and np.all(et <= loc_ref.E2E_BOUND[1]), (ep, et)


def test_relocalisation_reduced_equals_the_restatement(e2e):
    """One 61-beam scan of the same path at step 4: the best tile, bin and cost."""
    from slamhip import loc, synthetic
    small = synthetic.make_loop_sequence(loc_ref.E2E["n_scans"], seed=loc_ref.E2E["seed"], n_beams=61)
    w = dict(loc_ref.RELOC, step=4)
    cost, tile, kji, pose = loc_ref.relocalize(e2e.F, e2e.origin, e2e.cw, e2e.d_cap, small.scans[151], **w)
    r = loc.relocalize(e2e.field, [small.scans[151]], [0], loc.LocParams(**w))
    assert r.search.cost[0] == cost and r.search.tile[0] == tile and tuple(r.search.index[0]) == kji
    assert np.array_equal(r.search.poses[0], pose)


# ----------------------------------------------------------------------------- wiring

def test_scripts_save_check_and_localize(tmp_path):
    """The map is the odometry map (--produce-odometry-map: 10 mm and 5 mrad of noise per pose, no chain), so it
    lies in the frame of the truth and the localised scans are held against the truth, as in the experiment.  (The
    maps of the later stages are drawn from chained or relaxed poses, whose drift over 40 scans the check's report
    shows but no localiser can undo.)"""
    import localize as lz
    import main_batched as mb
    from slamhip import dataset, loc, synthetic
    mapfile = str(tmp_path / "map.npz")
    rep = mb.run(mb.parse(["synthetic:loop:40:5", "--skip-icp", "--produce-odometry-map", "--program-end",
                           "scan_matching", "--results-dir", str(tmp_path), "--cell-width", "0.05", "--save-map",
                           mapfile, "--map-check"]))
    assert (tmp_path / "map.npz").exists() and (tmp_path / "odometry_map_check.npz").exists()
    assert rep["map_check_odometry"]["scans"] == 40
    grid, origin, cw = loc.load_map(mapfile)
    assert grid.dtype == np.int8 and list(grid.shape) == rep["map_odometry"]["cells"] and cw == 0.05
    assert np.array_equal(origin, rep["map_odometry"]["origin"])
    with np.load(tmp_path / "odometry_map_check.npz") as z:
        assert z["cost"].shape == (40,) and np.array_equal(z["poses"], dataset.load("synthetic:loop:40:5")[0])
        assert np.all(z["mean"] >= 0) and np.all(z["mean"] <= int(z["d_cap"]) ** 2)
        print("wiring: mean squared cell distance per scan %.3f .. %.3f" % (z["mean"].min(), z["mean"].max()))
    rep2 = lz.run(lz.parse(["synthetic:loop:40:5", "--map", mapfile, "--results-dir", str(tmp_path)]))
    assert rep2["scans"] == 40 and rep2["status"][2] == rep2["status"][3] == 0
    truth = synthetic.make_loop_sequence(40, seed=5, n_beams=3).truth     # the path only
    with np.load(tmp_path / "localize.npz") as z:
        assert np.array_equal(z["scans"], np.arange(40))
        ep, et = loc_ref.pose_error(z["poses"], truth)
    print("wiring: largest error %.5f m, %.6f rad" % (ep.max(), et.max()))
    assert np.all(ep <= loc_ref.E2E_BOUND[0]) and np.all(et <= loc_ref.E2E_BOUND[1]), (ep, et)


def test_search_two_passes_and_two_point_tiles(scase, sfield):
    """47 x 47 shifts are more than one pass of 2,048, 4,200 points more than one LDS tile of 4,096."""
    from slamhip import loc
    f, _ = sfield
    rng = np.random.default_rng(3)
    pts = rng.uniform(-4.0, 4.0, size=(4200, 2))
    w = dict(n_theta=1, d_theta=0.1, nx=47, ny=47, step=1)
    centre = np.array([[0.4, 0.3, -0.2]])
    r = loc.search(f, [pts], [0], centre, loc.LocParams(**w), return_costs=True)
    vol, best = loc_ref.search(scase.F, scase.origin, scase.cw, D_CAP, pts, centre[0], **w)
    assert np.array_equal(r.costs[0], vol) and (r.cost[0],) + tuple(r.index[0]) == best
