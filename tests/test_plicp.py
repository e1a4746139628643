"""CPU tests of the point-to-line refinement's rule (tests/plicp_ref.py, the
restatement of include/slamhip.h): hand-placed normals, the status paths, the
accuracy of a refined odometry chain, the host-side argument checks of the
library and the conditions the fixtures of tests/test_plicp_gpu.py must meet so
that a bit-for-bit comparison of matches, iterations and statuses is fair.
"""
import functools

import numpy as np
import pytest

import plicp_ref as ref

import slamhip.plicp  # noqa: F401  (the feature under test: absent before it)
from slamhip import se2, synthetic


# ---------------------------------------------------------------- hand-placed normals

def wall(n, step=0.05, x0=0.0, y0=1.0):
    return np.stack([x0 + step * np.arange(n), np.full(n, y0)], axis=1)


def corner(n_side=12, step=0.05):
    """A wall along +x that turns by 90 degrees into +y at its last point."""
    a = np.stack([step * np.arange(n_side), np.zeros(n_side)], axis=1)
    b = np.stack([np.full(n_side, a[-1, 0]), step * np.arange(1, n_side + 1)], axis=1)
    return np.concatenate([a, b])


def normals_cases():
    """name -> (points, K, rho, ctol): the hand-placed cases, shared with the GPU test."""
    rho = 0.15
    at = np.array([[0.0, 0.0], [rho, 0.0], [2 * rho, 0.0], [3 * rho, 0.0]])           # neighbours exactly at rho
    beyond = at.copy()
    beyond[:, 0] = np.array([0.0, np.nextafter(rho, 1.0), 2 * np.nextafter(rho, 1.0), 3 * np.nextafter(rho, 1.0)])
    dup = np.array([[1.0, 2.0]] * 5)
    dup_ends = np.array([[0.0, 0.0], [0.05, 0.01], [0.0, 0.0], [0.05, 0.0], [0.1, 0.0]])
    return {
        "wall": (wall(40), 8, rho, 0.03),
        "wall_short_k": (wall(7), 8, rho, 0.03),
        "wall_k1": (wall(9), 1, rho, 0.03),
        "empty": (np.zeros((0, 2)), 8, rho, 0.03),
        "one": (wall(1), 8, rho, 0.03),
        "two": (wall(2), 8, rho, 0.03),
        "three": (wall(3), 8, rho, 0.03),
        "corner": (corner(), 8, rho, 0.03),
        "at_rho": (at, 8, rho, 0.03),
        "beyond_rho": (beyond, 8, rho, 0.03),
        "duplicates": (dup, 8, rho, 0.03),
        "duplicate_ends": (dup_ends, 1, rho, 0.03),
    }


def test_wall_normals_equal_bit_for_bit():
    Q, K, rho, ctol = normals_cases()["wall"]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    assert has.all()
    assert np.all(N == N[0]) and abs(N[0, 1]) == 1.0 and N[0, 0] == 0.0


def test_points_near_the_ends():
    """The support is cut at the scan's ends: rho = 0.15 reaches three
    neighbours of a 0.05 m wall, the first point has only its right ones."""
    Q, K, rho, ctol = normals_cases()["wall_short_k"]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    assert has.all() and np.all(N == N[0])
    # K = 1: the end points have a support of two points and lose their normal
    Q, K, rho, ctol = normals_cases()["wall_k1"]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    assert not has[0] and not has[-1] and has[1:-1].all()


@pytest.mark.parametrize("name, n_has", [("empty", 0), ("one", 0), ("two", 0), ("three", 3)])
def test_tiny_scans(name, n_has):
    Q, K, rho, ctol = normals_cases()[name]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    assert N.shape == (len(Q), 2) and has.sum() == n_has
    assert np.all(N[~has] == 0)


def test_corner_loses_its_normal():
    Q, K, rho, ctol = normals_cases()["corner"]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    n_side = len(Q) // 2
    c = n_side - 1                                  # the corner point
    # the chord of a support across the corner leaves the points nearest to it by more than ctol
    assert not has[c] and not has[c - 1] and not has[c + 1]
    # three or more steps away the support (rho reaches three neighbours) stays on one wall
    assert has[:c - 2].all() and has[c + 3:].all()
    assert np.all(np.abs(N[:c - 2]) == [0.0, 1.0]) and np.all(np.abs(N[c + 3:]) == [1.0, 0.0])
    # ... and with a corner tolerance above the largest offset every point keeps one
    assert ref.scan_normals(Q, K, rho, 1.0)[1].all()


def test_neighbour_at_rho_and_one_ulp_beyond():
    Q, K, rho, ctol = normals_cases()["at_rho"]
    assert (Q[1, 0] - Q[0, 0]) ** 2 == rho * rho      # exactly at the radius: supported
    _, has = ref.scan_normals(Q, K, rho, ctol)
    assert has[1] and has[2]
    Q, K, rho, ctol = normals_cases()["beyond_rho"]
    assert (Q[1, 0] - Q[0, 0]) ** 2 > rho * rho
    _, has = ref.scan_normals(Q, K, rho, ctol)
    assert not has.any()


def test_duplicate_points():
    Q, K, rho, ctol = normals_cases()["duplicates"]
    N, has = ref.scan_normals(Q, K, rho, ctol)
    assert not has.any() and np.all(N == 0)           # L2 = 0
    Q, K, rho, ctol = normals_cases()["duplicate_ends"]
    _, has = ref.scan_normals(Q, K, rho, ctol)
    assert not has[1] and has[3]                      # Q[0] == Q[2]: point 1's chord is empty


def test_bad_offsets_get_no_normals():
    pts = np.concatenate([wall(10), wall(10, y0=2.0)])
    N, flagged = ref.normals_packed(pts, [0, 10, 20])
    assert not flagged and (N != 0).any(axis=1).all()
    N, flagged = ref.normals_packed(pts, [0, 10, 5])
    assert flagged and (N[:10] != 0).any(axis=1).all() and np.all(N[10:] == 0)
    N, flagged = ref.normals_packed(pts, [0, 21])
    assert flagged and np.all(N == 0)


# ---------------------------------------------------------------- status paths

def room(n=200, w=4.0, h=3.0):
    """Points on the four walls of a w x h room, in beam order around it."""
    t = np.linspace(0.0, 1.0, n // 4, endpoint=False)
    return np.concatenate([np.stack([w * t, 0 * t], 1), np.stack([w + 0 * t, h * t], 1),
                           np.stack([w - w * t, h + 0 * t], 1), np.stack([0 * t, h - h * t], 1)])


def test_degenerate_wall_against_itself():
    Q = wall(60)
    N, has = ref.scan_normals(Q)
    assert has.all()
    T0 = se2.pose_to_mat(np.array([0.01, 0.002, 0.0]))
    r = ref.refine(Q, Q, N, T0)
    assert r["status"] == ref.DEGENERATE and r["iters"] == 0
    assert np.array_equal(r["tf"], T0)
    assert r["inliers"] == len(Q)


def test_too_few_and_the_gate():
    Q = room()
    N, _ = ref.scan_normals(Q, rho=0.3)
    far = se2.pose_to_mat(np.array([50.0, 0.0, 0.0]))
    r = ref.refine(Q, Q, N, far)
    assert r["status"] == ref.TOO_FEW and r["iters"] == 0 and r["inliers"] == 0
    assert np.array_equal(r["tf"], far) and np.all(r["match"] == -1)
    # three points at exactly max_dist on an axis (0.5: the square is exact), the others far away
    P = np.array([[0.5, 0.0], [4.0, 0.5], [0.0, 3.5], [30.0, 30.0], [-20.0, 1.0]])
    D = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 3.0], [2.0, 1.5]])
    Nd = np.zeros((4, 2))
    r = ref.refine(P, D, Nd, np.eye(3), max_dist=0.5, min_inliers=3, max_iters=1)
    assert r["inliers"] == 3 and r["status"] != ref.TOO_FEW
    assert np.array_equal(r["match"], [0, 1, 2, -1, -1])
    r = ref.refine(P, D, Nd, np.eye(3), max_dist=0.5, min_inliers=4, max_iters=1)
    assert r["inliers"] == 3 and r["status"] == ref.TOO_FEW and np.array_equal(r["tf"], np.eye(3))
    r = ref.refine(P, D, Nd, np.eye(3), max_dist=np.nextafter(0.5, 0.0), min_inliers=1, max_iters=1)
    assert r["inliers"] == 0 and r["status"] == ref.TOO_FEW


def test_point_fallback_solves_the_rigid_fit():
    """Without normals the rows are the point-to-point ones: matched points of
    a rigid motion give it back in a few steps."""
    Q = room(80)
    T = se2.pose_to_mat(np.array([0.03, -0.02, 0.01]))
    P = (np.linalg.inv(T) @ np.c_[Q, np.ones(len(Q))].T).T[:, :2]
    r = ref.refine(P, Q, np.zeros_like(Q), np.eye(3), eps_t=1e-10, eps_r=1e-10)
    assert r["status"] == ref.CONVERGED and np.abs(r["tf"] - T).max() < 1e-9


def test_apply_refinement_rule():
    from slamhip import plicp
    tf = np.stack([se2.pose_to_mat(np.array([0.1 * k, 0.0, 0.01 * k])) for k in range(5)])
    new = tf.copy()
    new[:, 0, 2] += 1.0
    res = plicp.PlicpResult(new, np.zeros(5), np.array([0.5, 0.5, 0.5, 0.05, 0.5]),
                            np.array([100, 100, 100, 100, 40]), np.full(5, 3),
                            np.array([plicp.CONVERGED, plicp.MAX_ITERS, plicp.TOO_FEW, plicp.CONVERGED,
                                      plicp.CONVERGED]))
    out, take = plicp.apply_refinement(tf, np.full(5, 100), res, min_overlap=0.5, min_observability=0.1)
    assert np.array_equal(take, [True, True, False, False, False])
    assert np.array_equal(out[:2], new[:2]) and out[2:].tobytes() == tf[2:].tobytes()
    out, take = plicp.apply_refinement(tf, np.full(5, 100), res, min_overlap=0.4, min_observability=0.0)
    assert np.array_equal(take, [True, True, False, True, True])
    with pytest.raises(ValueError):
        plicp.PlicpParams(max_iters=0)
    with pytest.raises(ValueError):
        plicp.PlicpParams(max_dist=float("inf"))
    with pytest.raises(ValueError):
        plicp.PlicpParams(normal_k=0)
    with pytest.raises(Exception):
        plicp.PlicpParams().max_dist = 1.0           # frozen


# ---------------------------------------------------------------- accuracy of a refined chain

def pack(scans):
    lens = [len(s) for s in scans]
    off = np.zeros(len(scans) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return np.concatenate(scans).astype(np.float64), off


def chain_errors(seq, tfs):
    """(rms position error, end heading error) of the chain of edges ``tfs``
    started at the true first pose, against ``seq.truth``."""
    X = se2.pose_to_mat(seq.truth[0])
    xs = [X]
    for T in tfs:
        X = X @ T
        xs.append(X)
    c = np.array([[x[0, 2], x[1, 2], np.arctan2(x[1, 0], x[0, 0])] for x in xs])
    d = c[:, :2] - seq.truth[:, :2]
    dh = (c[-1, 2] - seq.truth[-1, 2] + np.pi) % (2 * np.pi) - np.pi
    return float(np.sqrt((d ** 2).sum(axis=1).mean())), float(abs(dh))


@functools.lru_cache(maxsize=None)
def chain_case():
    """The 120-scan sequence, the oracle's point-to-point edges and their
    refinement by the restatement (computed once per session)."""
    import icp_oracle
    seq = synthetic.make_sequence(120, seed=3, n_beams=361)
    tfs = []
    for i in range(1, len(seq.scans)):
        init = se2.pose_to_mat(seq.odometry[i] - seq.odometry[i - 1])
        hist, _ = icp_oracle.icp(synthetic.homogeneous(seq.scans[i]), synthetic.homogeneous(seq.scans[i - 1]),
                                 init.copy(), 0.05, 100)
        tfs.append(np.array(hist[-1]))
    pts, off = pack(seq.scans)
    S = len(seq.scans)
    res = ref.refine_packed(pts, off, np.arange(1, S), np.arange(0, S - 1), np.stack(tfs))
    return seq, np.stack(tfs), res


def test_refined_chain_accuracy():
    """The issue's bound: the refined chain's rms position error and end heading
    error are at most half the point-to-point chain's (measured with the
    prototype: 0.068 against 0.471 m, 0.051 against 0.669 rad)."""
    seq, tfs, res = chain_case()
    assert all(r["status"] == ref.CONVERGED for r in res), [r["status"] for r in res]
    rms0, head0 = chain_errors(seq, tfs)
    rms1, head1 = chain_errors(seq, np.stack([r["tf"] for r in res]))
    print(f"rms position {rms0:.4f} -> {rms1:.4f} m, end heading {head0:.4f} -> {head1:.4f} rad, "
          f"iterations {min(r['iters'] for r in res)}-{max(r['iters'] for r in res)}")
    assert rms1 <= 0.5 * rms0
    assert head1 <= 0.5 * head0


# ---------------------------------------------------------------- fixtures of the GPU comparison

@functools.lru_cache(maxsize=None)
def fixture_pairs():
    """The fifteen pairs of the whole-run comparison on the device: twelve
    consecutive pairs of two ``make_sequence`` streams (361 and 1081 beams, with
    dropout for ragged sizes) from their odometry inits, and three loop-like
    pairs (scans four apart) started 0.1 m and 3 degrees off the truth.
    Returns (pts, off, src, dst, init)."""
    a = synthetic.make_sequence(24, seed=11, n_beams=361, dropout=0.1)
    b = synthetic.make_sequence(12, seed=12, n_beams=1081, dropout=0.05)
    scans = list(a.scans) + list(b.scans)
    nb = len(a.scans)
    src, dst, init = [], [], []
    for i in (1, 4, 7, 10, 13, 16, 19, 22):
        src.append(i), dst.append(i - 1), init.append(se2.pose_to_mat(a.odometry[i] - a.odometry[i - 1]))
    for i in (1, 4, 7, 10):
        src.append(nb + i), dst.append(nb + i - 1), init.append(se2.pose_to_mat(b.odometry[i] - b.odometry[i - 1]))
    off3 = [(0.1, 0.0, np.deg2rad(3.0)), (-0.07, 0.07, -np.deg2rad(3.0)), (0.0, -0.1, np.deg2rad(3.0))]
    for (i, j, seq, base), d in zip(((6, 2, a, 0), (20, 16, a, 0), (9, 5, b, nb)), off3):
        true = np.linalg.inv(se2.pose_to_mat(seq.truth[j])) @ se2.pose_to_mat(seq.truth[i])
        T = se2.pose_to_mat(np.array(d)) @ true
        T[2] = (0.0, 0.0, 1.0)
        src.append(base + i), dst.append(base + j), init.append(T)
    pts, off = pack(scans)
    return pts, off, np.array(src), np.array(dst), np.stack(init)


@functools.lru_cache(maxsize=None)
def fixture_results():
    """(results, traces) of the restatement on ``fixture_pairs`` (once per session)."""
    pts, off, src, dst, init = fixture_pairs()
    traces = []
    res = ref.refine_packed(pts, off, src, dst, init, traces=traces)
    return res, traces


def test_fixture_pairs_are_fair():
    """No decision of a fixture pair sits so close to its threshold that another
    order of the sums could flip it: every step's ratio to eps and every pivot's
    ratio to pivot_tol is 1e-6 away from the threshold, every inlier test 1e-9
    from the gate, and a run with the rows summed in a random order changes no
    match, iteration count, status or inlier count."""
    pts, off, src, dst, init = fixture_pairs()
    res, traces = fixture_results()
    assert len(res) == 15
    sizes = {int(off[s + 1] - off[s]) for s in src}
    assert len(sizes) > 8, sizes                     # ragged
    for b, (r, tr) in enumerate(zip(res, traces)):
        assert r["status"] in (ref.CONVERGED, ref.MAX_ITERS), (b, r["status"])
        assert len(tr) == r["iters"]
        for rec in tr:
            assert abs(max(rec["step"]) - 1.0) >= 1e-6, (b, rec["step"])
            for p in rec["pivots"]:
                assert abs(p / ref.DEFAULTS["pivot_tol"] - 1.0) >= 1e-6, (b, p)
            assert rec["gate_margin"].min() >= 1e-9, (b, rec["gate_margin"].min())
    assert max(r["iters"] for r in res) >= 3
    again = ref.refine_packed(pts, off, src, dst, init, rng=np.random.default_rng(7))
    for b, (r, s) in enumerate(zip(res, again)):
        assert np.array_equal(r["match"], s["match"]) and r["iters"] == s["iters"], b
        assert r["status"] == s["status"] and r["inliers"] == s["inliers"], b
        assert np.abs(r["tf"] - s["tf"]).max() < 1e-11, b


# ---------------------------------------------------------------- host-side argument checks (no GPU)

def _aligned(nbytes):
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, a + (-a) % 64


def test_host_validation():
    """Null arrays, max_iters = 0, bad tolerances and K are refused and B = 0
    succeeds before anything touches a device."""
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 107
    EINVAL, ETOOBIG = -1, -3
    keep, p = _aligned(256)      # never dereferenced: every call below returns before a launch

    def batch(pts=p, B=0, max_dist2=0.25, min_inliers=10, max_iters=50, eps_t=5e-4, eps_r=5e-4, pivot_tol=1e-9,
              max_n1=100, match=None, stride=0):
        return lib.slam_plicp_batch_f64(pts, p, 4, 100, p, p, p, p, B, max_dist2, min_inliers, max_iters, eps_t, eps_r,
                                        pivot_tol, max_n1, p, p, p, p, p, p, match, stride, None)

    assert batch() == 0
    assert batch(pts=None) == EINVAL and b"null" in lib.slam_last_error()
    assert batch(pts=None, B=3) == EINVAL
    assert batch(B=-1) == EINVAL
    assert batch(max_iters=0) == EINVAL and b"max_iters" in lib.slam_last_error()
    for kw in ({"max_dist2": -1.0}, {"max_dist2": float("inf")}, {"eps_t": float("nan")}, {"eps_r": -1e-3},
               {"pivot_tol": float("inf")}):
        assert batch(**kw) == EINVAL and b"tolerance" in lib.slam_last_error(), kw
    assert batch(max_n1=8193) == ETOOBIG
    assert batch(max_n1=8192) == 0
    assert batch(match=p, stride=99) == EINVAL and batch(match=p, stride=100) == 0

    def normals(pts=p, S=0, P=100, K=8, rho2=0.0225, ctol=0.03):
        return lib.slam_plicp_normals_f64(pts, p, S, P, K, rho2, ctol, p, None)

    assert normals() == 0
    assert normals(pts=None) == EINVAL and b"null" in lib.slam_last_error()
    assert normals(K=0) == EINVAL and b"K" in lib.slam_last_error()
    assert normals(S=-1) == EINVAL and normals(P=-1) == EINVAL
    assert normals(rho2=float("nan")) == EINVAL and normals(ctol=-0.1) == EINVAL
    del keep

