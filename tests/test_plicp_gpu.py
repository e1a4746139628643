"""GPU tests of the point-to-line refinement (csrc/plicp_kernels.hip,
slamhip.plicp) and of the stage that uses it.

The yardstick is the NumPy restatement tests/plicp_ref.py, which
tests/test_plicp.py pins to hand-placed cases.  Supports, corner tests, matches,
the gate, pivots and the stopping rule are decided by individually rounded fp64
operations, so ``has`` flags, matches, inlier counts, iteration counts and
statuses are compared with ``np.array_equal``; the transforms, ``err`` and
``obs`` depend on the order of the ten sums of a linearisation (and on cos /
sin), and are compared to 1e-9, the tolerance of ``icp()`` against its fixtures.
tests/test_plicp.py asserts that no fixture pair's decision sits near enough to
its threshold for that difference to flip it.
"""
import functools

import numpy as np
import pytest

import plicp_ref as ref
from test_plicp import chain_errors, fixture_pairs, fixture_results, normals_cases, pack, room, wall

pytestmark = pytest.mark.gpu

TILE = 2048   # kPlTile of csrc/plicp_kernels.hip


def _plicp():
    from slamhip import plicp
    return plicp


def _dev(a):
    from slamhip import device as dv
    return dv.to_dev(np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 2), np.float64)


def _normals(scans, K=8, rho=0.15, ctol=0.03, check=True):
    """(device normals as a host array, the packed offsets) of a list of scans, one launch."""
    pl = _plicp()
    pts, off = pack([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in scans])
    ss = pl.packed_scans(pts, off)
    N = pl.scan_normals(ss, pl.PlicpParams(normal_k=K, normal_rho=rho, corner_tol=ctol), check=check)
    return N.cpu().numpy(), off


def _compare_normals(scans, K=8, rho=0.15, ctol=0.03):
    got, off = _normals(scans, K, rho, ctol)
    want = np.concatenate([ref.scan_normals(s, K, rho, ctol)[0].reshape(-1, 2) for s in scans])
    assert got.shape == want.shape
    assert np.array_equal((got != 0).any(axis=1), (want != 0).any(axis=1))
    print("normals: max |device - restatement| =", np.abs(got - want).max(initial=0.0))
    assert np.abs(got - want).max(initial=0.0) <= 1e-15
    assert np.array_equal(got, want)   # IEEE square root and division on both sides: the same bits


def test_normals_hand_placed():
    cases = normals_cases()
    for K in (8, 1):
        scans = [Q for (Q, k, rho, ctol) in cases.values() if k == K]
        assert scans
        _compare_normals(scans, K=K)
    _compare_normals([cases["corner"][0]], ctol=1.0)


def test_normals_sizes_in_one_launch():
    from slamhip import synthetic
    seq = synthetic.make_sequence(2, seed=4, n_beams=1081)
    s = seq.scans[1]
    assert len(s) == 1081
    _compare_normals([s[:n] for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1081)])


def test_normals_bad_offsets_are_flagged():
    pl = _plicp()
    from slamhip import _abi
    pts = np.concatenate([wall(10), wall(10, y0=2.0)])
    ss = pl.packed_scans(pts, [0, 10, 5])
    N = pl.scan_normals(ss, check=False).cpu().numpy()
    want, flagged = ref.normals_packed(pts, [0, 10, 5])
    assert flagged and np.array_equal(N, want)
    with pytest.raises(_abi.SlamHipError):
        pl.status()
    pl.status()   # read and cleared


# ---------------------------------------------------------------- one linearisation

def _scene(rng, n1, n2):
    """A destination of n2 points on a jittered room outline (in order, so most
    have normals) and n1 source points: most near it, some far outside the gate."""
    Q = room(max(4 * ((n2 + 3) // 4), 4))[:n2] + rng.normal(0, 2e-3, (n2, 2))
    near = Q[rng.integers(0, n2, n1)] + rng.normal(0, 0.03, (n1, 2))
    far = rng.uniform(-3, 8, (n1, 2))
    P = np.where(rng.random((n1, 1)) < 0.8, near, far)
    return P, Q


def _run(scans, src, dst, init, normals, **kw):
    """slamhip.plicp.refine_batch over packed scans with given normals."""
    pl = _plicp()
    pts, off = pack(scans)
    ss = pl.packed_scans(pts, off)
    pk = {k: kw.pop(k) for k in list(kw) if k in ("max_dist", "min_inliers", "max_iters", "eps_t", "eps_r", "pivot_tol")}
    return pl.refine_batch(ss, src, dst, init, pl.PlicpParams(**pk), normals=_dev(normals), return_match=True, **kw)


def _want(scans, src, dst, init, normals, **kw):
    pts, off = pack(scans)
    return ref.refine_packed(pts, off, src, dst, init, normals=normals, **kw)


def _same(got, want):
    for b, w in enumerate(want):
        assert np.array_equal(got.match[b], w["match"]), b
        assert got.inliers[b] == w["inliers"] and got.status[b] == w["status"] and got.iters[b] == w["iters"], \
            (b, got.inliers[b], got.status[b], got.iters[b], w["inliers"], w["status"], w["iters"])
        assert np.abs(got.tf[b] - w["tf"]).max() <= 1e-9, (b, np.abs(got.tf[b] - w["tf"]).max())
        for g, x in ((got.err[b], w["err"]), (got.obs[b], w["obs"])):
            assert (np.isnan(g) and np.isnan(x)) or abs(g - x) <= 1e-9 * max(1.0, abs(x)), (b, g, x)


def _packed_normals(scans):
    return np.concatenate([ref.scan_normals(s)[0].reshape(-1, 2) for s in scans])


N1S = (1, 2, 255, 256, 257, 1081)
N2S = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def test_first_linearisation_block_and_tile_edges():
    """n1 across the workgroup's 256 lanes, n2 across the 2,048-point tile: all
    thirty pairs, one launch per source size (each takes its own instance)."""
    rng = np.random.default_rng(21)
    for n1 in N1S:
        scans, src, dst = [], [], []
        for n2 in N2S:
            P, Q = _scene(rng, n1, n2)
            src.append(len(scans)), scans.append(P)
            dst.append(len(scans)), scans.append(Q)
        N = _packed_normals(scans)
        init = np.broadcast_to(np.eye(3), (len(src), 3, 3)).copy()
        got = _run(scans, src, dst, init, N, max_iters=1, min_inliers=1)
        _same(got, _want(scans, src, dst, init, N, max_iters=1, min_inliers=1))
        assert (np.concatenate(got.match) >= 0).any() or n1 < 3


@pytest.mark.parametrize("n1", [1300, 2049, 4097, 8192])
def test_first_linearisation_large_sources(n1):
    """The instances of 8, 16 and 32 queries per lane (1081 points take 5)."""
    rng = np.random.default_rng(n1)
    P, Q = _scene(rng, n1, 300)
    N = _packed_normals([P, Q])
    got = _run([P, Q], [0], [1], np.eye(3)[None], N, max_iters=1)
    _same(got, _want([P, Q], [0], [1], np.eye(3)[None], N, max_iters=1))
    assert got.inliers[0] > n1 // 2


def test_nearest_at_tile_edges_and_ties():
    """The unique nearest point as the first and as the last entry of a tile, and
    duplicates on two sides of a tile edge: the first index wins."""
    n2 = 2 * TILE + 1
    ang = np.linspace(0, 2 * np.pi, n2, endpoint=False)
    ring = np.stack([6 * np.cos(ang), 6 * np.sin(ang)], axis=1)       # everything else: far from the sources
    P = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    cases = {"first": {TILE: (0.01, 0.0)}, "last": {TILE - 1: (0.01, 0.0), 2 * TILE - 1: (1.0, 0.02)},
             "tie": {TILE - 1: (0.0, 0.99), TILE: (0.0, 0.99), 2 * TILE - 1: (0.98, 0.0), 2 * TILE: (0.98, 0.0)}}
    expect = {"first": [TILE, -1, -1], "last": [TILE - 1, 2 * TILE - 1, -1], "tie": [-1, 2 * TILE - 1, TILE - 1]}
    scans, src, dst = [P], [], []
    for name, put in cases.items():
        Q = ring.copy()
        for k, xy in put.items():
            Q[k] = xy
        src.append(0), dst.append(len(scans)), scans.append(Q)
    N = np.zeros((sum(len(s) for s in scans), 2))
    init = np.broadcast_to(np.eye(3), (3, 3, 3)).copy()
    got = _run(scans, src, dst, init, N, max_iters=1, min_inliers=1, max_dist=0.1)
    for b, name in enumerate(cases):
        assert np.array_equal(got.match[b], expect[name]), (name, got.match[b])
    _same(got, _want(scans, src, dst, init, N, max_iters=1, min_inliers=1, max_dist=0.1))


# ---------------------------------------------------------------- whole runs

@functools.lru_cache(maxsize=None)
def _fixture_device():
    pl = _plicp()
    pts, off, src, dst, init = fixture_pairs()
    ss = pl.packed_scans(pts, off)
    N = ref.normals_packed(pts, off)[0]
    return ss, _dev(N), N


def test_whole_runs_match_the_restatement():
    pl = _plicp()
    pts, off, src, dst, init = fixture_pairs()
    want, _ = fixture_results()
    ss, dN, N = _fixture_device()
    assert np.array_equal(pl.scan_normals(ss).cpu().numpy(), N)
    got = pl.refine_batch(ss, src, dst, init, normals=dN, return_match=True)
    assert len(want) == 15 and len(got.tf) == 15      # no fixture pair is left out
    _same(got, want)
    # ... and with the normals computed on the device (the default path)
    again = pl.refine_batch(ss, src, dst, init, return_match=True)
    assert again.tf.tobytes() == got.tf.tobytes() and again.err.tobytes() == got.err.tobytes()


def test_status_paths():
    pl = _plicp()
    Q = wall(60)
    T0 = np.array([[1.0, 0.0, 0.01], [0.0, 1.0, 0.002], [0.0, 0.0, 1.0]])
    R = room()
    far = np.array([[1.0, 0.0, 50.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    scans = [Q, R]
    N = np.concatenate([ref.scan_normals(Q)[0], ref.scan_normals(R, rho=0.3)[0]])
    init = np.stack([T0, far])
    got = _run(scans, [0, 1], [0, 1], init, N)
    want = _want(scans, [0, 1], [0, 1], init, N)
    assert want[0]["status"] == ref.DEGENERATE and want[1]["status"] == ref.TOO_FEW
    _same(got, want)
    assert np.array_equal(got.iters, [0, 0])
    assert got.tf.tobytes() == init.tobytes()          # T unchanged, bit for bit
    assert got.inliers[0] == 60 and got.inliers[1] == 0 and np.all(got.match[1] == -1)
    # apply_refinement keeps the input row of the pair that ended TOO_FEW (and of the degenerate one)
    other = init + 1e-3
    out, taken = pl.apply_refinement(other, [60, len(R)], got, 0.0, 0.0)
    assert not taken.any() and out.tobytes() == other.tobytes()
    # the gate: points at exactly max_dist are inliers, min_inliers equal to their number passes
    P = np.array([[0.5, 0.0], [4.0, 0.5], [0.0, 3.5], [30.0, 30.0], [-20.0, 1.0]])
    D = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 3.0], [2.0, 1.5]])
    Z = np.zeros((9, 2))
    for mi in (3, 4):
        g = _run([P, D], [0], [1], np.eye(3)[None], Z, max_dist=0.5, min_inliers=mi, max_iters=1)
        _same(g, _want([P, D], [0], [1], np.eye(3)[None], Z, max_dist=0.5, min_inliers=mi, max_iters=1))
        assert g.inliers[0] == 3 and (g.status[0] == pl.TOO_FEW) == (mi == 4)
    # MAX_ITERS: one step of a pair that needs at least three; its transform is the restatement's first step
    pts, off, src, dst, init = fixture_pairs()
    want, _ = fixture_results()
    b = int(np.argmax([w["iters"] for w in want]))
    assert want[b]["iters"] >= 3
    ss, dN, N = _fixture_device()
    one = pl.refine_batch(ss, src[b:b + 1], dst[b:b + 1], init[b:b + 1], pl.PlicpParams(max_iters=1), normals=dN,
                          return_match=True)
    w1 = ref.refine_packed(pts, off, src[b:b + 1], dst[b:b + 1], init[b:b + 1], normals=N, max_iters=1)
    assert w1[0]["status"] == ref.MAX_ITERS
    _same(one, w1)


def test_bad_pair_is_flagged_and_neighbours_are_unaffected():
    pl = _plicp()
    from slamhip import _abi
    pts, off, src, dst, init = fixture_pairs()
    ss, dN, N = _fixture_device()
    good = pl.refine_batch(ss, src[:3], dst[:3], init[:3], normals=dN, return_match=True)
    s2, d2 = src[:3].copy(), dst[:3].copy()
    s2[1] = len(ss)                                     # a scan index outside [0, S)
    got = pl.refine_batch(ss, s2, d2, init[:3], normals=dN, return_match=True, check=False)
    with pytest.raises(_abi.SlamHipError):
        pl.status()
    pl.status()
    assert got.status[1] == -1 and got.iters[1] == 0 and got.tf[1].tobytes() == init[1].tobytes()
    assert np.isnan(got.err[1]) and np.isnan(got.obs[1])
    for b in (0, 2):
        assert got.tf[b].tobytes() == good.tf[b].tobytes() and np.array_equal(got.match[b], good.match[b])
        assert got.status[b] == good.status[b] and got.iters[b] == good.iters[b]
    d3 = dst[:3].copy()
    d3[2] = -1
    got = pl.refine_batch(ss, src[:3], d3, init[:3], normals=dN, check=False)
    with pytest.raises(_abi.SlamHipError):
        pl.status()
    assert got.status[2] == -1 and got.tf[0].tobytes() == good.tf[0].tobytes()
    with pytest.raises(ValueError):
        pl.refine_batch(ss, s2, d2, init[:3], normals=dN)


# ---------------------------------------------------------------- determinism, reuse

def _bytes(r, b=None):
    sl = slice(None) if b is None else slice(b, b + 1)
    return b"".join(np.ascontiguousarray(a[sl]).tobytes() for a in (r.tf, r.err, r.obs, r.inliers, r.iters, r.status)) \
        + b"".join(m.tobytes() for m in (r.match if b is None else r.match[b:b + 1]))


def test_determinism_across_launches_and_slots():
    pl = _plicp()
    pts, off, src, dst, init = fixture_pairs()
    ss, dN, N = _fixture_device()
    # a mixed batch: the fifteen pairs in turn, every fifth one started 40 m off (TOO_FEW)
    idx = np.arange(257) % 15
    ini = init[idx].copy()
    ini[::5, 0, 2] += 40.0
    a = pl.refine_batch(ss, src[idx], dst[idx], ini, normals=dN, return_match=True)
    b = pl.refine_batch(ss, src[idx], dst[idx], ini, normals=dN, return_match=True)
    assert _bytes(a) == _bytes(b)
    assert set(a.status) >= {pl.CONVERGED, pl.TOO_FEW}
    for p in (0, 3, 8, 11, 14):                         # 361- and 1081-beam pairs and a loop-like one
        alone = pl.refine_batch(ss, src[p:p + 1], dst[p:p + 1], init[p:p + 1], normals=dN, return_match=True)
        jdx = idx.copy()
        jdx[0] = jdx[-1] = p
        jni = ini.copy()
        jni[0] = jni[-1] = init[p]
        inside = pl.refine_batch(ss, src[jdx], dst[jdx], jni, normals=dN, return_match=True)
        # a lane sums its queries t + 256 q in ascending q whatever instance the batch's largest scan selects
        assert _bytes(alone, 0) == _bytes(inside, 0) == _bytes(inside, 256)


def test_reuse_with_other_scans():
    """A second call with other scans gives what a fresh one gives; the cached
    normals of a scan set are reused."""
    pl = _plicp()
    from slamhip import icp, synthetic
    a = synthetic.make_sequence(4, seed=31, n_beams=361)
    b = synthetic.make_sequence(4, seed=32, n_beams=1081, dropout=0.1)

    def inits(s):
        from slamhip import se2
        return np.stack([se2.pose_to_mat(s.odometry[i] - s.odometry[i - 1]) for i in range(1, 4)])

    sa, sb = icp.ScanSet(a.scans), icp.ScanSet(b.scans)
    pl.refine_batch(sa, [1, 2, 3], [0, 1, 2], inits(a))
    second = pl.refine_batch(sb, [1, 2, 3], [0, 1, 2], inits(b), return_match=True)
    fresh = pl.refine_batch(icp.ScanSet(b.scans), [1, 2, 3], [0, 1, 2], inits(b), return_match=True)
    assert _bytes(second) == _bytes(fresh)
    assert pl.scan_normals(sb) is pl.scan_normals(sb)
    third = pl.refine_batch(sb, [1, 2, 3], [0, 1, 2], inits(b), return_match=True)
    assert _bytes(third) == _bytes(fresh)
    # other normals parameters are another cache entry
    assert pl.scan_normals(sb, pl.PlicpParams(normal_k=2)) is not pl.scan_normals(sb)


# ---------------------------------------------------------------- the stage

def test_scan_matching_refine():
    """Stage 1 with ``refine``: the refined chain meets the CPU accuracy
    condition on the device; without it nothing changes."""
    pl = _plicp()
    from slamhip import pipeline, synthetic
    seq = synthetic.make_sequence(120, seed=3, n_beams=361)
    plain = pipeline.scan_matching(seq.odometry, seq.scans, 100, 0.05)
    none = pipeline.scan_matching(seq.odometry, seq.scans, 100, 0.05, refine=None)
    for f in ("poses", "tf", "err", "iters"):
        assert getattr(plain, f).tobytes() == getattr(none, f).tobytes(), f
    assert none.refine_status is None and none.refine_inliers is None and none.refine_obs is None
    r = pipeline.scan_matching(seq.odometry, seq.scans, 100, 0.05, refine=pl.PlicpParams())
    assert np.all(r.refine_status == pl.CONVERGED) and r.refine_taken.all()
    assert r.err.tobytes() == plain.err.tobytes() and r.iters.tobytes() == plain.iters.tobytes()
    rms0, head0 = chain_errors(seq, plain.tf)
    rms1, head1 = chain_errors(seq, r.tf)
    print(f"rms position {rms0:.4f} -> {rms1:.4f} m, end heading {head0:.4f} -> {head1:.4f} rad")
    assert rms1 <= 0.5 * rms0 and head1 <= 0.5 * head0
    assert r.refine_inliers.min() >= 0.5 * min(len(s) for s in seq.scans) and np.all(r.refine_obs > 0)
    with pytest.raises(TypeError):
        pipeline.scan_matching(seq.odometry[:3], seq.scans[:3], 100, 0.05, refine=True)


def test_loop_closure_stage_refine():
    """A loop-closure stage with ``refine``: acceptance is unchanged, and an
    accepted constraint carries what ``refine_edges`` gives for its transform."""
    pl = _plicp()
    import src.pose_graph as pgm
    from slamhip import icp, pipeline, synthetic
    seq = synthetic.make_loop_sequence(120, seed=5, n_beams=361, step=0.5)
    assert len(seq.loop_pairs) >= 5
    ss = icp.ScanSet(seq.scans)
    pg0, pg1, pg2 = (pgm.PoseGraph(seq.truth.copy()) for _ in range(3))
    ok0 = pipeline.manual_loop_closures(pg0, seq.scans, seq.loop_pairs, scanset=ss)
    ok1 = pipeline.manual_loop_closures(pg1, seq.scans, seq.loop_pairs, scanset=ss, refine=pl.PlicpParams())
    ok2 = pipeline.manual_loop_closures(pg2, seq.scans, seq.loop_pairs, scanset=ss, refine=None)
    assert np.array_equal(ok0, ok1) and np.array_equal(ok0, ok2) and ok0.any()

    def closures(pg):
        want = {frozenset(map(int, p)) for p in seq.loop_pairs[ok0]}
        return {frozenset((i, j)): T for i, j, T in pg.graph.edges(data="object") if frozenset((i, j)) in want}
    e0, e1, e2 = closures(pg0), closures(pg1), closures(pg2)
    assert len(e0) == int(ok0.sum()) == len(e1)
    pairs = seq.loop_pairs[ok0]
    plain = np.stack([e0[frozenset(map(int, p))] for p in pairs])
    assert all(e2[k].tobytes() == e0[k].tobytes() for k in e0)
    tfs, taken, res = pipeline.refine_edges(ss, pairs[:, 0], pairs[:, 1], plain, pl.PlicpParams())
    assert taken.any()
    for p, T, t, old in zip(pairs, tfs, taken, plain):
        assert e1[frozenset(map(int, p))].tobytes() == T.tobytes()
        assert t or T.tobytes() == old.tobytes()
    # a gate nothing passes keeps every point-to-point transform bit for bit
    none, taken, _ = pipeline.refine_edges(ss, pairs[:, 0], pairs[:, 1], plain, pl.PlicpParams(), gates=(1.01, 0.0))
    assert not taken.any() and none.tobytes() == plain.tobytes()
