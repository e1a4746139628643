"""CPU-side checks of the localisation in a finished occupancy grid: the NumPy
restatement (tests/loc_ref.py) against the definition itself and against
SciPy's Euclidean distance transform, the tie rule, parameter validation before
any device call, the map file, the scripts' argument parsing, the hand-made
refinement cases and the end-to-end experiment on the restatement (which pins
the measured error behind the GPU test's bound)."""
import os
import sys

import numpy as np
import pytest

import loc_ref
from conftest import GOLDEN, PKG

sys.path.insert(0, os.path.join(PKG, "scripts"))


def _grid(H, W, seed, p=0.05):
    rng = np.random.default_rng(seed)
    g = rng.integers(-128, 1, size=(H, W)).astype(np.int8)
    g[rng.random((H, W)) < p] = 3
    return g


@pytest.mark.parametrize("H,W,d_cap,seed", [(1, 30, 4, 0), (23, 1, 5, 1), (17, 29, 3, 2), (31, 37, 50, 3), (20, 20, 1, 4)])
def test_field_equals_the_definition(H, W, d_cap, seed):
    g = _grid(H, W, seed)
    assert np.array_equal(loc_ref.field(g, d_cap), loc_ref.field_brute(g, d_cap))
    empty = np.zeros((H, W), np.int8)
    assert np.all(loc_ref.field(empty, d_cap) == d_cap * d_cap)
    assert np.array_equal(loc_ref.field(g, d_cap, occ_min=3), loc_ref.field(empty, d_cap))   # 3 > 3 is false


def test_field_equals_scipy_edt_below_the_cap():
    from scipy import ndimage
    g = _grid(61, 83, 5, p=0.01)
    d_cap = 9
    F = loc_ref.field(g, d_cap)
    edt2 = np.rint(ndimage.distance_transform_edt(~(g > 0)) ** 2).astype(np.int64)
    below = edt2 < d_cap * d_cap
    assert below.any() and (~below).any()
    assert np.array_equal(F[below], edt2[below]) and np.all(F[~below] == d_cap * d_cap)


def test_occ_min_rule():
    g = np.array([[-128, -1, 0, 1, 126, 127]], np.int8)
    for occ_min in (-128, -1, 0, 1, 126):
        assert np.array_equal(loc_ref.field(g, 3, occ_min)[0] == 0, g[0].astype(int) > occ_min)


def test_tie_rule_and_costs_outside_the_map():
    F = loc_ref.field(np.zeros((9, 11), np.int8), 4)
    pts = np.array([[0.1, 0.2], [0.5, -0.3], [1e12, 0.0]])
    costs, best = loc_ref.search(F, (0.0, 0.0), 0.1, 4, pts, (0.2, 0.3, 0.4), n_theta=3, d_theta=0.1, nx=4, ny=5, step=2)
    assert costs.shape == (3, 5, 4) and np.all(costs == 3 * 16) and best == (48, 0, 0, 0)
    # two equal minima: the smaller flat index (k ny + j) nx + i wins
    g = np.zeros((9, 11), np.int8)
    g[4, 3] = g[4, 7] = 1
    F = loc_ref.field(g, 4)
    one = np.array([[0.0, 0.0]])
    costs, best = loc_ref.search(F, (0.0, 0.0), 1.0, 4, one, (0.0, 5.5, 4.5), n_theta=1, d_theta=0.0, nx=7, ny=3, step=1)
    assert costs[0, 1, 1] == 0 and costs[0, 1, 5] == 0 and best == (0, 0, 1, 1)
    pose = loc_ref.assemble((0.0, 5.5, 4.5), best[1:], 1, 0.0, 7, 3, 1, 1.0)
    assert np.array_equal(pose, [3.5, 4.5, 0.0])


def test_parameter_validation_needs_no_device():
    from slamhip import loc
    for kw in (dict(n_theta=0), dict(nx=0), dict(ny=-1), dict(step=0), dict(d_theta=float("nan")), dict(max_iters=0),
               dict(eps_t=-1.0), dict(eps_r=float("inf")), dict(min_inlier_frac=1.5), dict(pivot_tol=-1e-9),
               dict(n_theta=2048, nx=1024, ny=1024)):
        with pytest.raises(ValueError):
            loc.LocParams(**kw)
    g = np.zeros((4, 5), np.int8)
    for args in ((g.astype(np.int16), (0, 0), 0.1, 5, 0), (g[0], (0, 0), 0.1, 5, 0), (g[:0], (0, 0), 0.1, 5, 0),
                 (g, (0, 0, 0), 0.1, 5, 0), (g, (0, np.nan), 0.1, 5, 0), (g, (0, 0), 0.0, 5, 0),
                 (g, (0, 0), -0.1, 5, 0), (g, (0, 0), 0.1, 0, 0), (g, (0, 0), 0.1, 256, 0), (g, (0, 0), 0.1, 2.5, 0),
                 (g, (0, 0), 0.1, 5, 128), (g, (0, 0), 0.1, 5, -129)):
        with pytest.raises(ValueError):
            loc.check_map(*args)
        with pytest.raises(ValueError):     # the constructor checks before it touches the device
            loc.LikelihoodField(*args)
    p = loc.reloc_params(loc.LocParams(d_theta=np.deg2rad(3.0), step=2))
    assert p.n_theta == 120 and p.d_theta == 2 * np.pi / 120 and p.step == 2
    c = loc.reloc_centres(163, 203, np.array([-0.07, -0.06]), 0.05, p)
    n_theta, d, want = loc_ref.reloc_shape(163, 203, np.array([-0.07, -0.06]), 0.05, 21, 21, 2, np.deg2rad(3.0))
    assert (n_theta, d) == (p.n_theta, p.d_theta) and np.array_equal(c, want) and len(c) == 4 * 5
    index = np.array([[3, 0, 20], [0, 7, 1]])
    centre = np.array([[0.1, 2.0, 3.0], [-0.2, 1.0, -1.0]])
    q = loc.LocParams(n_theta=5, d_theta=0.02, nx=21, ny=9, step=3)
    got = loc.assemble(centre, index, q, 0.05)
    for b in range(2):
        assert np.array_equal(got[b], loc_ref.assemble(centre[b], index[b], 5, 0.02, 21, 9, 3, 0.05))


def test_library_refuses_bad_shapes_before_any_launch():
    from slamhip import _abi
    L = _abi.lib()
    assert L.slam_abi_version() >= 109
    p = 16   # any aligned non-null pointer: these calls return before they touch an array

    def search(H=37, W=53, cw=0.2, d_cap=6, B=1, max_n=61, n_theta=1, nx=1, ny=1, step=1, field=p):
        return L.slam_loc_search(field, H, W, 0.0, 0.0, cw, d_cap, p, p, 1, 61, p, p, p, B, max_n, n_theta, nx, ny,
                                 step, p, None, p, None)
    for kw, word in [(dict(B=0), b"B = 0"), (dict(H=0), b"grid"), (dict(cw=0.0), b"cell_width"),
                     (dict(d_cap=0), b"d_cap"), (dict(d_cap=256), b"d_cap"), (dict(step=0), b"positive"),
                     (dict(n_theta=2048, nx=1024, ny=1024), b"31 bits"), (dict(H=50000, W=50000), b"bordered"),
                     (dict(d_cap=255, max_n=33027), b"31 bits"), (dict(field=None), b"null")]:
        assert search(**kw) == -1 and word in L.slam_last_error(), (kw, L.slam_last_error())
    assert L.slam_loc_search_work_size(1, 37, 53, 9, 5, 7, 1) >= 8 + 2 * (37 + 10) * (53 + 14)
    assert L.slam_loc_search_work_size(1, 37, 53, 0, 5, 7, 1) == -1
    assert L.slam_loc_field_work_size(37, 53) >= 37 * 53 and L.slam_loc_field_work_size(0, 53) == -1
    for args, word in [((p, 0, 5, 0, 3, p, p, None), b"grid"), ((p, 5, 5, 0, 0, p, p, None), b"d_cap"),
                       ((p, 5, 5, 200, 3, p, p, None), b"occ_min"), ((p, 70000, 5, 0, 3, p, p, None), b"launch grid"),
                       ((None, 5, 5, 0, 3, p, p, None), b"null")]:
        assert L.slam_loc_field(*args) == -1 and word in L.slam_last_error(), (args, L.slam_last_error())

    def refine(B=1, max_iters=5, eps_t=1e-4, frac=0.5, d_cap=6, init=p):
        return L.slam_loc_refine_f64(p, 37, 53, 0.0, 0.0, 0.2, d_cap, p, p, 1, 61, p, init, B, 61, max_iters, eps_t,
                                     1e-4, frac, 1e-9, p, p, p, p, p, None)
    for kw, word in [(dict(B=-1), b"negative"), (dict(max_iters=0), b"max_iters"), (dict(eps_t=-1.0), b"tolerance"),
                     (dict(frac=1.5), b"min_inlier_frac"), (dict(d_cap=300), b"d_cap"), (dict(init=None), b"null")]:
        assert refine(**kw) == -1 and word in L.slam_last_error(), (kw, L.slam_last_error())
    assert refine(B=0) == 0
    assert L.slam_loc_set_table(3) == -1 and L.slam_loc_set_table(2) == 0


def test_map_file_round_trip(tmp_path):
    from slamhip import loc
    g = _grid(13, 17, 6)
    f = str(tmp_path / "m.npz")
    loc.save_map(f, g, (-1.25, 0.1 + 0.2), 0.05)
    grid, origin, cw = loc.load_map(f)
    assert grid.dtype == np.int8 and np.array_equal(grid, g)
    assert np.array_equal(origin, [-1.25, 0.1 + 0.2]) and cw == 0.05
    with pytest.raises(ValueError):
        loc.save_map(f, g.astype(np.float32), (0, 0), 0.05)


def test_scripts_parse_the_new_flags(tmp_path):
    import localize as lz
    import main_batched as mb
    a = mb.parse(["synthetic:loop:40:5"])
    assert a.save_map is None and a.map_check is False           # opt-in: off by default
    a = mb.parse(["synthetic:loop:40:5", "--save-map", "m.npz", "--map-check", "--save-map-files"])
    assert a.save_map == "m.npz" and a.map_check and a.save_map_files
    for bad in (["--save-map", "m.npz", "--skip-occupancy-grid"], ["--map-check", "--skip-occupancy-grid"],
                ["--map-check-d-cap", "0"]):
        with pytest.raises(SystemExit):
            mb.parse(["synthetic:loop:40:5"] + bad)
    a = lz.parse(["synthetic:loop:40:5", "--map", "m.npz"])
    p = lz.loc_params(a)
    assert (a.guess, p.n_theta, p.nx, p.ny, p.step, p.d_theta) == ("odometry", 41, 21, 21, 1, 0.0125)
    a = lz.parse(["synthetic:loop:40:5", "--map", "m.npz", "--guess", "none", "--window-cells", "15", "--every", "4"])
    p = lz.loc_params(a)
    assert (p.nx, p.ny, p.step, a.every) == (15, 15, 2, 4) and p.d_theta == np.deg2rad(3.0)
    for bad in ([], ["--map", "m.npz", "--step", "0"], ["--map", "m.npz", "--d-cap", "300"],
                ["--map", "m.npz", "--guess", "gps"], ["--map", "m.npz", "--angle-step-deg", "0"],
                ["--map", "m.npz", "--every", "0"]):
        with pytest.raises(SystemExit):
            lz.parse(["synthetic:loop:40:5"] + bad)


def test_refinement_cases_reach_every_status():
    """The hand-made cases of tests/test_loc_gpu.py: their statuses, and that the
    iteration counts do not hang on the order of the sums."""
    grid, origin, cw, d_cap, pts, truth = loc_ref.refine_case()
    assert len(pts) == 111
    F = loc_ref.field(grid, d_cap)
    for start in (truth + (0.03, -0.02, 0.01), truth + (0.08, 0.06, -0.03)):
        r = loc_ref.refine(F, origin, cw, d_cap, pts, start)
        assert r["status"] == loc_ref.CONVERGED and r["inliers"] == 111
        assert loc_ref.pose_error(r["pose"], truth)[0][0] < 1e-6
        for seed in range(3):
            s = loc_ref.refine(F, origin, cw, d_cap, pts, start, rng=np.random.default_rng(seed))
            assert s["iters"] == r["iters"] and np.abs(s["pose"] - r["pose"]).max() < 1e-9
        assert loc_ref.refine(F, origin, cw, d_cap, pts, start, max_iters=1)["status"] == loc_ref.MAX_ITERS
    far = loc_ref.refine(F, origin, cw, d_cap, pts, truth + (50.0, 50.0, 0.0))
    assert far["status"] == loc_ref.TOO_FEW and far["inliers"] == 0 and far["iters"] == 0
    one = loc_ref.refine(F, origin, cw, d_cap, np.array([[1.0, 0.2]]), truth)
    assert one["status"] == loc_ref.SINGULAR and one["inliers"] == 1 and one["iters"] == 0


def test_end_to_end_on_the_restatement():
    """Eleven of the experiment's 18 held-out scans (every second one, and scans 331
    and 391, which set the measured error) must land within that error."""
    seq, map_idx, held, guess = loc_ref.e2e_inputs()
    assert seq.per_lap == 528 and len(map_idx) == 264 and len(held) == 18
    with np.load(os.path.join(GOLDEN, "loc_e2e_map.npz")) as z:
        grid, origin, cw = z["grid"], z["origin"], float(z["cell_width"])
    d_cap = loc_ref.E2E["d_cap"]
    F = loc_ref.field(grid, d_cap)
    pick = [b for b in range(len(held)) if b % 2 == 0 or held[b] in (331, 391)]
    assert len(pick) == 11
    ep, et = [], []
    for b in pick:
        best, r = loc_ref.localize(F, origin, cw, d_cap, seq.scans[held[b]], guess[b])
        assert r["status"] in (loc_ref.CONVERGED, loc_ref.MAX_ITERS)
        p, t = loc_ref.pose_error(r["pose"], seq.truth[held[b]])
        ep.append(p[0])
        et.append(t[0])
    assert max(ep) <= loc_ref.E2E_MEASURED[0] and max(et) <= loc_ref.E2E_MEASURED[1], (max(ep), max(et))
    assert max(ep) > 0.99 * loc_ref.E2E_MEASURED[0] and max(et) > 0.99 * loc_ref.E2E_MEASURED[1]
