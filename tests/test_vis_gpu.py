"""GPU tests of the visibility check (csrc/vis_kernels.hip, slamhip.vis) and of
the stages that use it.

The yardstick is the NumPy restatement tests/vis_ref.py, which tests/test_vis.py
pins to plain double loops and hand-placed cases.  Sectors, tables, agreement
and conflict are decided by individually rounded fp64 operations and the counts
are integers, so tables and counts are compared with ``np.array_equal``."""
import functools

import numpy as np
import pytest

import vis_ref as ref
from test_vis import CORNERS, MARGIN, TIE_DIRS, hand_cases, pack, quarter_turn_case

pytestmark = pytest.mark.gpu


def _vis():
    from slamhip import vis
    return vis


def _scanset(scans):
    from slamhip import plicp
    return plicp.packed_scans(*pack(scans))


def _raw(scans, src, dst, tf, dirs, margin, W, tables=None):
    """(tables, counts) through the C-ABI with any table of sector centres
    (``slamhip.vis`` always makes the cos / sin one)."""
    from slamhip import _abi, device as dv
    lib = _abi.lib()
    ss = _scanset(scans)
    n, S, B = len(ss), len(dirs), len(src)
    d_dirs = dv.to_dev(dirs, np.float64)
    tab = dv.empty((n, S), np.float64) if tables is None else dv.to_dev(tables, np.float64)
    h = dv.stream_handle()
    if tables is None:
        _abi.check(lib.slam_vis_tables_f64(dv.ptr(ss.pts), dv.ptr(ss.scan_off), n, len(ss.host_pts), dv.ptr(d_dirs), S,
                                           dv.ptr(tab), h), "tables")
    out = dv.empty((B, 6), np.int32)
    d_src, d_dst = dv.to_dev(src, np.int32), dv.to_dev(dst, np.int32)
    d_tf = dv.to_dev(np.asarray(tf, dtype=np.float64).reshape(B, 9), np.float64)
    _abi.check(lib.slam_vis_check_f64(dv.ptr(ss.pts), dv.ptr(ss.scan_off), n, len(ss.host_pts), dv.ptr(d_dirs), S,
                                      dv.ptr(tab), dv.ptr(d_src), dv.ptr(d_dst), dv.ptr(d_tf), B, float(margin), int(W),
                                      dv.ptr(out), h), "check")
    _abi.check(lib.slam_vis_status(h), "status")
    return tab.cpu().numpy(), out.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- sizes, sector counts, windows

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1081)


@functools.lru_cache(maxsize=None)
def size_case():
    """Prefixes of one 1081-point scan at the workgroup's edges against the next
    scan of the stream, with a transform 0.2 m and 0.05 rad off the truth: points
    that agree, conflict and are unknown in both directions."""
    from slamhip import se2, synthetic
    seq = synthetic.make_sequence(3, seed=4, n_beams=1081)
    a, b = seq.scans[1], seq.scans[2]
    assert len(a) == 1081 and len(b) == 1081
    scans = [a[:n] for n in SIZES] + [b]
    T = np.linalg.inv(se2.pose_to_mat(seq.truth[2])) @ se2.pose_to_mat(seq.truth[1])
    T = se2.pose_to_mat(np.array([0.2, -0.1, 0.05])) @ T
    T[2] = (0.0, 0.0, 1.0)
    B = len(SIZES)
    src = np.arange(B)
    dst = np.full(B, B)
    return scans, src, dst, np.broadcast_to(T, (B, 3, 3)).copy()


@pytest.mark.parametrize("S, windows", [(3, (0, 1)), (8, (0, 1, 2)), (64, (0, 1, 2)), (360, (0, 1, 2)),
                                        (1024, (0, 1, 2))])
def test_tables_and_counts_at_every_size(S, windows):
    vis = _vis()
    scans, src, dst, tf = size_case()
    pts, off = pack(scans)
    ss = _scanset(scans)
    want_tab, flagged = ref.tables_packed(pts, off, ref.dirs(S))
    assert not flagged
    got_tab = vis.scan_tables(ss, vis.VisParams(sectors=S, window=0)).cpu().numpy()
    assert got_tab.shape == (len(scans), S) and np.isinf(got_tab[0]).all()          # the empty scan
    assert np.array_equal(got_tab, want_tab)
    kinds = np.zeros(2, dtype=np.int64)
    for W in windows:
        got = vis.check_batch(ss, src, dst, tf, vis.VisParams(sectors=S, window=W, margin=0.15))
        want, _ = ref.check_packed(pts, off, src, dst, tf, S, 0.15, W, tables=want_tab)
        assert got.counts.dtype == np.int64 and np.array_equal(got.counts, want), (S, W)
        assert np.array_equal(got.counts[:, 2], SIZES) and np.all(got.counts[:, 5] == 1081)
        assert not got.ok[0] and np.array_equal(got.ok, ref.passes(want))            # an empty scan fails
        a, c = ref.shares(want)
        assert np.array_equal(got.agree, a) and np.array_equal(got.conflict, c)
        kinds += (want[:, [0, 3]].sum(), want[:, [1, 4]].sum())
    assert (kinds > 0).all(), kinds     # agreeing and conflicting points both occur
    # the same edges in the other direction of the pair: the inverse transform swaps the two halves of the counts
    if S == 360:
        inv = np.stack([np.linalg.inv(t) for t in tf])
        inv[:, 2] = (0.0, 0.0, 1.0)
        back = vis.check_batch(ss, dst, src, inv, vis.VisParams(sectors=S, window=1))
        want, _ = ref.check_packed(pts, off, dst, src, inv, S, 0.15, 1, tables=want_tab)
        assert np.array_equal(back.counts, want)


def test_hand_placed_cases():
    """The cases of tests/test_vis.py on the device, with its dyadic table of
    sector centres: points at the margin and one ulp off, ties between two
    sectors, the origin, an unseen entry in the window, a quarter turn."""
    I = np.eye(3)
    for name, (src, dst, T, W, want) in hand_cases().items():
        tab, got = _raw([src, dst], [0], [1], T[None], TIE_DIRS, MARGIN, W)
        w = ref.edge(src, dst, T, TIE_DIRS, MARGIN, W)
        assert np.array_equal(got[0], w), name
        assert want is None or list(got[0]) == want, name
        assert np.array_equal(tab, [ref.table(src, TIE_DIRS), ref.table(dst, TIE_DIRS)]), name
        if name == "one_ulp":
            assert list(got[0][:3]) == [1, 1, 3]
    # ties: the four half-axes go to sectors 0 (not 7), 1, 3 and 5; the origin to 0
    axes = [[2.0, 0.0], [0.0, 2.0], [-2.0, 0.0], [0.0, -2.0]]
    tab, _ = _raw([axes, [[0.0, 0.0]]], [0], [1], I[None], TIE_DIRS, MARGIN, 0)
    assert np.array_equal(np.nonzero(np.isfinite(tab[0]))[0], [0, 1, 3, 5]) and np.all(tab[0][[0, 1, 3, 5]] == 4.0)
    assert tab[1][0] == 0.0 and np.isinf(tab[1][1:]).all()
    # an unseen entry in the window (given tables): blocks the conflict, not the agreement
    R2 = np.full(8, np.inf)
    R2[[7, 0, 1]] = 4.0
    pts = [[1.0, 0.0], [2.0, 0.0]]
    far = [[0.0, 64.0]]                      # the other direction: one point that maps where nothing was seen
    for hole, want in ((None, [1, 1, 2]), (7, [1, 0, 2]), (1, [1, 0, 2]), (0, [1, 0, 2])):
        R = R2.copy()
        if hole is not None:
            R[hole] = np.inf
        tables = np.stack([np.full(8, np.inf), R])
        _, got = _raw([pts, far], [0], [1], I[None], TIE_DIRS, MARGIN, 1, tables=tables)
        assert list(got[0]) == want + [0, 0, 1], hole
        assert list(ref.direction(pts, I, R, TIE_DIRS, MARGIN, 1)[:3]) == want
    R = R2.copy()
    R[1] = 1.0                               # the minimum over the window decides
    tables = np.stack([np.full(8, np.inf), R])
    three = [[0.5, 0.0], [0.875, 0.0], [1.5, 0.0]]
    _, got = _raw([three, far], [0], [1], I[None], TIE_DIRS, MARGIN, 1, tables=tables)
    assert list(got[0]) == [1, 1, 3, 0, 0, 1]
    # a quarter turn: the inverse
    src, dst, T = quarter_turn_case()
    _, got = _raw([src, dst, src + [[1.5, 0.0]]], [0, 2], [1, 1], np.stack([T, T]), TIE_DIRS, MARGIN, 0)
    assert list(got[0]) == [1, 0, 2, 1, 0, 2] and list(got[1][:3]) == [1, 1, 3]
    assert np.array_equal(got[1], ref.edge(src + [[1.5, 0.0]], dst, T, TIE_DIRS, MARGIN, 0))


def test_points_that_are_not_finite():
    vis = _vis()
    a = np.array([[1.0, 0.5], [np.nan, 1.0], [np.inf, 0.0], [1e200, 1e200], [-2.0, 0.25], [0.3, -4.0]])
    b = np.array([[1.0, 0.45], [-2.0, 0.3], [np.nan, np.nan], [0.3, -3.0]])
    pts, off = pack([a, b])
    ss = _scanset([a, b])
    p = vis.VisParams(sectors=8, window=1, margin=0.25)
    assert np.array_equal(vis.scan_tables(ss, p).cpu().numpy(), ref.tables_packed(pts, off, ref.dirs(8))[0])
    got = vis.check_batch(ss, [0, 1], [1, 0], np.stack([np.eye(3)] * 2), p)
    assert np.array_equal(got.counts, ref.check_packed(pts, off, [0, 1], [1, 0], np.stack([np.eye(3)] * 2), 8, 0.25, 1)[0])
    assert got.counts.tolist() == [[2, 0, 6, 2, 0, 4], [2, 0, 4, 2, 0, 6]]     # the two finite pairs agree, no more
    p0 = vis.VisParams(sectors=8, window=0, margin=0.25)                        # the 3 m return in front of the 4 m one
    got = vis.check_batch(ss, [0], [1], np.eye(3)[None], p0)
    assert np.array_equal(got.counts, ref.check_packed(pts, off, [0], [1], np.eye(3)[None], 8, 0.25, 0)[0])
    assert got.counts[0, 4] == 1


# ---------------------------------------------------------------- a stream with its ICP transforms

@functools.lru_cache(maxsize=None)
def stream_case():
    """40 edges of ``make_sequence(41, 5, dropout=0.35)`` (ragged scans) with the
    device's ICP transforms, the scan set and the restatement's counts."""
    from slamhip import icp, pipeline, synthetic
    seq = synthetic.make_sequence(41, 5, dropout=0.35)
    ss = icp.ScanSet(seq.scans)
    r = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    src, dst = np.arange(1, 41), np.arange(0, 40)
    pts, off = pack(seq.scans)
    want, flagged = ref.check_packed(pts, off, src, dst, r.tf)
    assert not flagged and len({len(s) for s in seq.scans}) > 20
    return seq, ss, src, dst, r.tf, want


def test_stream_with_icp_transforms():
    vis = _vis()
    seq, ss, src, dst, tf, want = stream_case()
    got = vis.check_batch(ss, src, dst, tf)
    assert np.array_equal(got.counts, want)
    assert np.array_equal(got.ok, ref.passes(want)) and got.ok.all()
    print("agree share >=", got.agree.min(), "conflict share <=", got.conflict.max())
    from slamhip import pipeline
    again = pipeline.check_edges(ss, src, dst, tf, vis.VisParams())
    assert np.array_equal(again.counts, want)
    import src.icp as host
    ok, info = host.check_visibility(seq.scans[7], seq.scans[6], tf[6])
    assert ok and np.array_equal(info["counts"], want[6])
    ok, info = host.check_visibility(seq.scans[7], seq.scans[6], tf[6], margin=0.01, max_conflict=0.0)
    assert np.array_equal(info["counts"], ref.edge(seq.scans[7], seq.scans[6], tf[6], ref.dirs(360), 0.01, 1))


@pytest.mark.parametrize("B", [0, 1, 257])
def test_batch_sizes(B):
    """No edge, one, and more than a workgroup's threads; an edge's counts do
    not depend on its slot or on the batch around it."""
    vis = _vis()
    seq, ss, src, dst, tf, want = stream_case()
    idx = (np.arange(B) * 7) % 40
    got = vis.check_batch(ss, src[idx], dst[idx], tf[idx])
    assert got.counts.shape == (B, 6) and got.agree.shape == (B, 2) and got.conflict.shape == (B, 2)
    assert got.ok.shape == (B,) and got.ok.dtype == bool
    assert np.array_equal(got.counts, want[idx])


def test_cached_tables_are_reused():
    vis = _vis()
    from slamhip import _abi, icp
    seq = stream_case()[0]
    ss = icp.ScanSet(seq.scans[:6])
    lib = _abi.lib()
    real, calls = lib.slam_vis_tables_f64, []

    def counting(*a):
        calls.append(a[5])
        return real(*a)
    lib.slam_vis_tables_f64 = counting
    try:
        t1 = vis.scan_tables(ss)
        assert calls == [360]
        assert vis.scan_tables(ss) is t1 and vis.scan_tables(ss, vis.VisParams(margin=0.3, window=2)) is t1
        tf = np.stack([np.eye(3)] * 5)
        a = vis.check_batch(ss, np.arange(1, 6), np.arange(0, 5), tf)
        b = vis.check_batch(ss, np.arange(1, 6), np.arange(0, 5), tf, tables=t1)
        assert calls == [360] and np.array_equal(a.counts, b.counts)      # no second table launch
        t2 = vis.scan_tables(ss, vis.VisParams(sectors=64))
        assert calls == [360, 64] and t2 is not t1 and tuple(t2.shape) == (6, 64)
    finally:
        lib.slam_vis_tables_f64 = real
    with pytest.raises(ValueError):
        vis.check_batch(ss, [1], [0], np.eye(3)[None], vis.VisParams(sectors=8), tables=t1)


def test_bad_offsets_and_indices_are_flagged():
    vis = _vis()
    from slamhip import _abi, plicp
    seq, ss, src, dst, tf, want = stream_case()
    scans = [seq.scans[k] for k in range(4)]
    pts, off = pack(scans)
    good = vis.check_batch(_scanset(scans), [1, 2, 3], [0, 1, 2], tf[:3])
    assert np.array_equal(good.counts, want[:3])
    # an offset past the points: scan 1 leaves [0, P] and scan 2 descends; their tables stay +inf and are
    # flagged, the other rows are right
    bad_off = off.copy()
    bad_off[2] = len(pts) + 7
    sb = plicp.packed_scans(pts, bad_off)
    tab = vis.scan_tables(sb, check=False).cpu().numpy()
    with pytest.raises(_abi.SlamHipError):
        vis.status()
    vis.status()   # read and cleared
    want_tab, flagged = ref.tables_packed(pts, bad_off, ref.dirs(360))
    assert flagged and np.array_equal(tab, want_tab) and np.isinf(tab[1]).all() and np.isinf(tab[2]).all()
    assert np.isfinite(tab[0]).any() and np.isfinite(tab[3]).any()
    # an edge over such a scan is not computed; the others of the launch are unaffected
    got = vis.check_batch(sb, [1, 3, 0], [0, 2, 3], tf[[0, 2, 0]], check=False)
    with pytest.raises(_abi.SlamHipError):
        vis.status()
    vis.status()
    w, flagged = ref.check_packed(pts, bad_off, [1, 3, 0], [0, 2, 3], tf[[0, 2, 0]], tables=want_tab)
    assert flagged and np.array_equal(got.counts, w)
    assert np.all(got.counts[0] == -1) and np.all(got.counts[1] == -1) and np.all(got.counts[2] >= 0)
    assert not got.ok[0] and not got.ok[1]
    # scan indices outside [0, n_scans)
    s4 = _scanset(scans)
    for s, d in (([1, 4, 3], [0, 1, 2]), ([1, 2, 3], [0, -1, 2])):
        got = vis.check_batch(s4, s, d, tf[:3], check=False)
        with pytest.raises(_abi.SlamHipError):
            vis.status()
        vis.status()
        assert np.all(got.counts[1] == -1) and not got.ok[1]
        assert np.array_equal(got.counts[[0, 2]], want[[0, 2]])
        with pytest.raises(ValueError):
            vis.check_batch(s4, s, d, tf[:3])
    assert np.array_equal(vis.check_batch(s4, [1, 2, 3], [0, 1, 2], tf[:3]).counts, want[:3])


# ---------------------------------------------------------------- stage 1: verify and repair

def chain_rms(seq, tfs):
    """The rms position error of the chain of edges ``tfs`` started at the true
    first pose, against ``seq.truth``."""
    from slamhip import se2
    X = se2.pose_to_mat(seq.truth[0])
    xy = [X[:2, 2]]
    for T in tfs:
        X = X @ T
        xy.append(X[:2, 2])
    d = np.array(xy) - seq.truth[:, :2]
    return float(np.sqrt((d ** 2).sum(axis=1).mean()))


@functools.lru_cache(maxsize=None)
def loop600_runs():
    from slamhip import icp, pipeline, synthetic
    vis = _vis()
    seq = synthetic.make_loop_sequence(600, 3)
    ss = icp.ScanSet(seq.scans)
    plain = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    none = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, verify=None)
    fixed = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, verify=vis.VisParams())
    return seq, ss, plain, none, fixed


def test_scan_matching_verify_and_repair():
    """The four corner edges of the 600-scan loop fail, are re-matched from
    their odometry inits and then pass; every other row is the ICP's; the chain
    is four times nearer the truth at least (CPU: 0.80 against 6.57 m)."""
    vis = _vis()
    from slamhip import pipeline, se2
    seq, ss, plain, none, fixed = loop600_runs()
    for f in ("poses", "tf", "err", "iters"):
        assert getattr(plain, f).tobytes() == getattr(none, f).tobytes(), f
    assert none.verify_ok is None and none.verify_counts is None and none.repaired is None \
        and none.repair_source is None
    bad = np.nonzero(~fixed.verify_ok)[0] + 1
    assert list(bad) == CORNERS
    assert fixed.verify_counts.shape == (599, 6)
    want = ref.check_packed(*pack(seq.scans), np.arange(1, 600)[bad - 1], np.arange(0, 599)[bad - 1],
                            plain.tf[bad - 1])[0]
    assert np.array_equal(fixed.verify_counts[bad - 1], want)
    assert list(np.nonzero(fixed.repaired)[0] + 1) == CORNERS and np.all(fixed.repair_source[bad - 1] == 1)
    assert np.all(fixed.repair_source[fixed.verify_ok] == 0)
    keep = fixed.verify_ok
    assert fixed.tf[keep].tobytes() == plain.tf[keep].tobytes()
    assert fixed.err.tobytes() == plain.err.tobytes() and fixed.iters.tobytes() == plain.iters.tobytes()
    after = pipeline.check_edges(ss, bad, bad - 1, fixed.tf[bad - 1], vis.VisParams())
    assert after.ok.all()
    print("repaired edges: conflict share", after.conflict.max(), "agree share", after.agree.min())
    rms0, rms1 = chain_rms(seq, plain.tf), chain_rms(seq, fixed.tf)
    print(f"chain rms position error {rms0:.3f} -> {rms1:.3f} m")
    assert rms1 < 0.25 * rms0
    assert np.array_equal(fixed.poses, se2.compose_chain(seq.odometry[0], fixed.tf))


def test_scan_matching_flag_only_and_with_refine():
    vis = _vis()
    from slamhip import pipeline, plicp
    seq, ss, plain, none, fixed = loop600_runs()
    flag = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, verify=vis.VisParams(), repair="none")
    for f in ("poses", "tf", "err", "iters"):
        assert getattr(plain, f).tobytes() == getattr(flag, f).tobytes(), f
    assert np.array_equal(flag.verify_ok, fixed.verify_ok) and np.array_equal(flag.verify_counts, fixed.verify_counts)
    assert not flag.repaired.any() and not flag.repair_source.any()
    # refine= runs afterwards, on the repaired transforms
    both = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, verify=vis.VisParams(),
                                  refine=plicp.PlicpParams())
    tfs, taken, _ = pipeline.refine_edges(ss, np.arange(1, 600), np.arange(0, 599), fixed.tf, plicp.PlicpParams())
    assert both.tf.tobytes() == tfs.tobytes() and np.array_equal(both.refine_taken, taken)
    assert np.array_equal(both.repair_source, fixed.repair_source)


# ---------------------------------------------------------------- the signature stage

class _Graph:
    def __init__(self, poses):
        self.poses = poses
        self.added = []

    def add_constraint(self, i, j, T, convention=None):
        self.added.append((i, j, T))


def test_signature_stage_rejects_an_aliased_closure(monkeypatch):
    """The stage's candidate list is given by hand: true loop pairs (the same
    place a lap on) and one aliased pair, a scan against the scan half a lap on,
    all from the identity.  Every candidate is below the stage's default error
    threshold (the aliased pair's ICP error is 105.6 against 110), so only the
    check stands between the aliased pair and the graph."""
    vis = _vis()
    from slamhip import icp, pipeline, sig, synthetic
    seq = synthetic.make_loop_sequence(300, seed=5, step=0.2)
    lap = seq.per_lap
    assert lap == 132
    true = [(i, i + lap, 0) for i in range(20, 160, 20)]
    alias = (10, 10 + lap // 2, 0)
    cand = true[:3] + [alias] + true[3:]
    monkeypatch.setattr(sig, "signature_candidates_device", lambda *a, **k: list(cand))
    ss = icp.ScanSet(seq.scans)
    g0, g1, g2 = (_Graph(seq.odometry.copy()) for _ in range(3))
    c0, ok0 = pipeline.signature_loop_closures(g0, seq.scans, scanset=ss, init="identity")
    c2, ok2 = pipeline.signature_loop_closures(g2, seq.scans, scanset=ss, init="identity", verify=None)
    assert c0 == cand and ok0.all() and np.array_equal(ok0, ok2)              # without the check: today's graph
    assert [(i, j) for i, j, _ in g0.added] == [(i, j) for i, j, _ in cand] == [(i, j) for i, j, _ in g2.added]
    assert all(a[2].tobytes() == b[2].tobytes() for a, b in zip(g0.added, g2.added))
    c1, ok1, rep = pipeline.signature_loop_closures(g1, seq.scans, scanset=ss, init="identity",
                                                    verify=vis.VisParams())
    assert c1 == cand and rep.checked == len(cand) and rep.rejected == 1
    assert list(ok1) == [c != alias for c in cand] and np.array_equal(rep.ok, ok1)
    assert [(i, j) for i, j, _ in g1.added] == [(i, j) for i, j, _ in true]
    kept = {(i, j): T for i, j, T in g0.added}
    assert all(T.tobytes() == kept[(i, j)].tobytes() for i, j, T in g1.added)
    a, c = vis.shares(rep.counts)
    print("aliased pair: agree", a[3], "conflict", c[3], "; true pairs: agree >=", np.delete(a, 3, 0).min(),
          "conflict <=", np.delete(c, 3, 0).max())
    with pytest.raises(TypeError):
        pipeline.signature_loop_closures(g1, seq.scans, scanset=ss, verify=True)
    # the drop-in function reports the count
    import src.loop_closure_detection as host
    g3 = _Graph(seq.odometry.copy())
    assert host.detect_signatures(g3, seq.scans, init="identity", verify=vis.VisParams()) == 1
    assert [(i, j) for i, j, _ in g3.added] == [(i, j) for i, j, _ in true]


# ---------------------------------------------------------------- the driver

def test_cli_edge_check(tmp_path):
    """``--edge-check visibility`` on the 600-scan loop with its ground-truth
    loop pairs: the summary counts the four corner edges flagged and repaired,
    and the closures checked; ``--scan-matching-repair none`` only flags."""
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("main_batched_vis_gpu", os.path.join(PKG, "scripts", "main_batched.py"))
    mb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mb)
    common = ["synthetic:loop:600:3", "--manual-loop-closures", "auto", "--program-end", "loop_closure",
              "--results-dir", str(tmp_path), "--skip-occupancy-grid"]
    plain = mb.run(mb.parse(common))
    assert "edge_check" not in plain and "edge_check" not in plain["loop_closures"]
    rep = mb.run(mb.parse(common + ["--edge-check", "visibility"]))
    ec = rep["edge_check"]
    assert ec == {"method": "visibility", "edges": 599, "flagged": 4, "repair": "refine-from-init", "repaired": 4,
                  "repair_source": [595, 4, 0]}
    lc = rep["loop_closures"]
    assert lc["annotated"] == plain["loop_closures"]["annotated"] == 8
    assert lc["edge_check"]["method"] == "visibility"
    assert lc["edge_check"]["checked"] == plain["loop_closures"]["accepted"]
    assert lc["accepted"] == lc["edge_check"]["checked"] - lc["edge_check"]["rejected"]
    flag = mb.run(mb.parse(common + ["--edge-check", "visibility", "--scan-matching-repair", "none"]))
    assert flag["edge_check"]["flagged"] == 4 and flag["edge_check"]["repaired"] == 0
    assert flag["edge_check"]["repair_source"] == [599, 0, 0]
