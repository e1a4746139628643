"""GPU tests of the scan signatures (csrc/sig_kernels.hip, slamhip.sig) and of
the stage, the drop-in function and the command-line switch that use them.

The yardstick is the NumPy restatement tests/sig_ref.py, which tests/test_sig.py
pins to plain double loops.  Every comparison of signatures and matches is
``np.array_equal``: only integers and individually rounded fp64 comparisons
decide an outcome.
"""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

import sig_ref
from test_sig import edge_case_points, tie_tables, turned

sys.path.insert(0, os.path.join(PKG, "scripts"))

pytestmark = pytest.mark.gpu


def _equal_sets(sg, want):
    got = sg.host()
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _check_match(sg, sig, start, n_rows, frac, K, rows=None, **kw):
    """match_signatures against sig_ref.match (on ``rows`` only when given)."""
    from slamhip import sig as gsig
    got = gsig.match_signatures(sg, start, n_rows, frac, K, **kw)
    want = sig_ref.match(sig, start, n_rows, frac[0], frac[1], K, rows)
    sel = slice(None) if rows is None else rows
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g[sel], w)
    return got


@pytest.mark.parametrize("S", [8, 64, 128])
def test_signatures(S):
    """Scans of 1 to 4,097 points (one lane, around the wave, several strides of
    the 256-thread workgroup), one that is empty after the ring filter, the
    ring-edge, origin and NaN cases, and sector ties from duplicate table rows."""
    from slamhip import icp, sig as gsig
    rng = np.random.default_rng(S)
    params = gsig.SigParams(sectors=S)
    dirs, edges2 = params.tables()
    ref_dirs, ref_edges2 = sig_ref.tables(S)
    assert np.array_equal(dirs, ref_dirs) and np.array_equal(edges2, ref_edges2)
    scans = [rng.uniform(-14, 14, size=(m, 2)) for m in (1, 63, 64, 65, 1081, 4097)]
    scans += [rng.uniform(20, 30, size=(70, 2)), edge_case_points(edges2), np.zeros((3, 2))]
    ss = icp.ScanSet(scans)
    want = sig_ref.signatures(scans, dirs, edges2)
    assert want[2][6] == 0 and want[2][4] > 100
    _equal_sets(gsig.build_signatures(ss, params), want)
    tied = tie_tables(S)
    _equal_sets(gsig.build_signatures(ss, params, tables=tied), sig_ref.signatures(scans, *tied))
    other = gsig.SigParams(sectors=S, r_min=0.5, dr=0.25)
    _equal_sets(gsig.build_signatures(ss, other), sig_ref.signatures(scans, *sig_ref.tables(S, 0.5, 0.25)))


@pytest.fixture(scope="module")
def loop700():
    """make_loop_sequence(700, seed=3, n_beams=181), every frame turned, and
    its reference signatures (64 sectors)."""
    from slamhip import synthetic
    seq = synthetic.make_loop_sequence(700, seed=3, n_beams=181)
    scans = turned(seq.scans, np.random.default_rng(1).uniform(-np.pi, np.pi, 700))
    return seq, scans, sig_ref.signatures(scans, *sig_ref.tables(64))


@pytest.mark.parametrize("n", [1, 2, 65, 257, 700])
def test_match_loop_sequences(loop700, n):
    """The first n scans: built on the device, matched from the path rule's
    starts and from j >= i (the row itself included), at three thresholds."""
    from slamhip import icp, lcd, sig as gsig
    seq, scans, ref = loop700
    sg = gsig.build_signatures(icp.ScanSet(scans[:n]))
    _equal_sets(sg, [r[:n] for r in ref])
    sig = ref[0][:n]
    start, n_rows = lcd.path_starts(seq.odometry[:n], 5)
    for frac in ((0, 1), (1, 4), (1, 1)):
        _check_match(sg, sig, start, n_rows, frac, 4)
        j, d, k, count = _check_match(sg, sig, np.arange(n), n, frac, 4)
        assert (j[:, 0] == np.arange(n)).all() and (d[:, 0] == 0).all() and (k[:, 0] == 0).all()
    if n == 700:
        assert n_rows > 400 and (gsig.match_signatures(sg, start, n_rows)[3] > 0).sum() > 100


def _random_signatures(n, S, seed):
    """Masks of a density that varies from scan to scan, so that the ring-count
    screen drops some pairs and keeps others."""
    rng = np.random.default_rng(seed)
    dens = rng.uniform(0.1, 0.9, size=n)
    return (rng.random((n, S, 32)) < dens[:, None, None]).dot(1 << np.arange(32, dtype=np.uint64)).astype(np.uint32)


def test_many_row_blocks_and_chunks_screen_on_and_off():
    """6,001 signatures: 1,501 workgroups of 4 rows over 16 column chunks of 384
    columns.  Checked on a sample of rows (the block and chunk boundaries among
    them); the screen switched off gives the same arrays."""
    from slamhip import _abi, sig as gsig
    n = 6001
    sig = _random_signatures(n, 64, 0)
    sg = gsig.SignatureSet.from_host(sig)
    start = np.random.default_rng(1).integers(0, n + 1, size=n)
    start[:8] = (0, 383, 384, 385, n, n - 1, 0, 5999)
    rows = np.unique(np.r_[np.arange(8), 383, 384, 3999, 4000, 4001, n - 2, n - 1,
                           np.random.default_rng(2).integers(0, n, 60)])
    got = _check_match(sg, sig, start, n, (2, 5), 4, rows)
    assert 0 < (got[3] > 4).sum() and (got[3] == 0).sum() > 0
    L = _abi.lib()
    try:
        assert L.slam_sig_set_screen(0) == 0
        off = gsig.match_signatures(sg, start, n, (2, 5), 4)
    finally:
        assert L.slam_sig_set_screen(1) == 0
    for a, b in zip(got, off):
        assert np.array_equal(a, b)
    assert L.slam_sig_set_screen(2) == -1


@pytest.mark.parametrize("S", [8, 72, 128])
def test_other_sector_counts(S):
    """Fewer shifts than lanes, and the second pass of shifts 64 and up."""
    from slamhip import sig as gsig
    sig = _random_signatures(300, S, S)
    sig[7] = np.roll(sig[2], S - 1)   # a perfect match at the last shift
    sig[9] = np.roll(sig[3], 5)
    sg = gsig.SignatureSet.from_host(sig)
    j, d, k, _ = _check_match(sg, sig, np.arange(300) + 1, 299, (1, 2), 16)
    assert (j[2, 0], d[2, 0], k[2, 0]) == (7, 0, S - 1) and (j[3, 0], d[3, 0], k[3, 0]) == (9, 0, 5)


def test_ties_few_candidates_and_partial_rows():
    from slamhip import sig as gsig
    rng = np.random.default_rng(4)
    one = rng.integers(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
    same = np.full(64, 0x00F0F00F, np.uint32)   # the same mask in every sector: every shift gives 0
    for sig in (np.tile(one, (10, 1)), np.tile(same, (10, 1)), np.zeros((10, 64), np.uint32)):
        sg = gsig.SignatureSet.from_host(sig)
        for K in (1, 4, 16):   # at most 10 candidates: fewer than K = 16
            j, d, k, count = _check_match(sg, sig, np.zeros(10, np.int64), 10, (0, 1), K)
            assert np.array_equal(j[0, :min(K, 10)], np.arange(min(K, 10))) and (j[:, 10:] == -1).all()
            assert (count == 10).all() and (k[j >= 0] == 0).all() and (d[j >= 0] == 0).all()
        _check_match(sg, sig, np.arange(10) + 1, 10, (1, 4), 16)   # the last row has start == N
        _check_match(sg, sig, np.arange(10), 3, (1, 4), 4)         # n_rows < N
        out = gsig.match_signatures(sg, np.zeros(10, np.int64), 0)
        assert out[0].shape == (0, 1) and out[3].shape == (0,)


def test_repeat_side_stream_and_checks():
    import torch
    from slamhip import _abi, icp, sig as gsig
    sig = _random_signatures(900, 64, 8)
    sg = gsig.SignatureSet.from_host(sig)
    start = np.arange(900) // 2
    a = gsig.match_signatures(sg, start, 900, (2, 5), 4)
    b = gsig.match_signatures(sg, start, 900, (2, 5), 4)
    c = gsig.match_signatures(sg, start, 900, (2, 5), 4, stream=torch.cuda.Stream())
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    ss = icp.ScanSet([np.random.default_rng(0).uniform(-5, 5, size=(200, 2)) for _ in range(5)])
    s0, s1 = gsig.build_signatures(ss), gsig.build_signatures(ss, stream=torch.cuda.Stream())
    for x, y in zip(s0.host(), s1.host()):
        assert np.array_equal(x, y)
    # what only the device sees: a start outside [0, N] is flagged, reported once, and nothing is read through it
    for bad in (-1, 901, 1 << 40):
        st = start.copy()
        st[450] = bad
        with pytest.raises(_abi.SlamHipError, match="status -1.*start"):
            gsig.match_signatures(sg, st, 900, (2, 5), 4)
        again = gsig.match_signatures(sg, start, 900, (2, 5), 4)
        assert np.array_equal(again[0], a[0])
    # argument errors
    for kw in (dict(top_k=0), dict(top_k=17), dict(max_frac=(2, 1)), dict(max_frac=(-1, 1)), dict(max_frac=(0, 0))):
        with pytest.raises(ValueError):
            gsig.match_signatures(sg, start, 900, **kw)
    with pytest.raises(ValueError):
        gsig.match_signatures(sg, start, 901)
    with pytest.raises(ValueError):
        gsig.SigParams(sectors=60)
    L = _abi.lib()
    p = [sg.d_sig.data_ptr(), sg.d_ring.data_ptr(), sg.d_n.data_ptr()]
    o = torch.empty(4 * 900 + 16, dtype=torch.int32, device=sg.device)
    w = torch.empty(int(L.slam_sig_work_size(900, 64, 1)), dtype=torch.uint8, device=sg.device)
    st = torch.zeros(900, dtype=torch.int32, device=sg.device)

    def call(N=900, S=64, n_rows=900, num=1, den=4, K=1, sig_ptr=p[0]):
        return L.slam_sig_match(sig_ptr, p[1], p[2], N, S, st.data_ptr(), n_rows, num, den, K, o.data_ptr(),
                                o[900:].data_ptr(), o[1800:].data_ptr(), o[2700:].data_ptr(), w.data_ptr(), None)
    assert call(n_rows=0) == 0
    for kw in (dict(sig_ptr=None), dict(S=60), dict(S=136), dict(S=0), dict(K=0), dict(K=17), dict(num=5),
               dict(num=-1), dict(n_rows=-1), dict(n_rows=901), dict(N=0)):
        assert call(**kw) == -1, kw
        assert L.slam_last_error() != b""
    assert L.slam_sig_work_size(900, 64, 17) == -1 and L.slam_sig_work_size(0, 64, 1) == -1
    assert L.slam_sig_work_size(900, 12, 1) == -1
    assert L.slam_sig_work_size(50000, 64, 16) <= 16 * 50000 * 196 + 256   # linear in N
    assert L.slam_sig_build(None, None, 5, 10, None, None, 64, None, None, None, None) == -1
    assert L.slam_sig_status(None) == 0
    assert L.slam_abi_version() >= 105


def _truth_tf(seq, i, j, turn):
    """T with pc_i ~ T pc_j for scan j taken in a frame turned by ``turn``."""
    from slamhip import se2
    Xj = se2.pose_to_mat(seq.truth[j]) @ se2.pose_to_mat((0.0, 0.0, turn))
    return np.linalg.inv(se2.pose_to_mat(seq.truth[i])) @ Xj


def test_shift_seeds_icp():
    """The first 12 loop pairs of make_loop_sequence(700, seed=5, n_beams=361),
    the later scan's frame turned at random: ICP seeded by the shift ends at the
    true transform (0.1 m, 0.02 rad, error < 30) on all 12, and from the
    identity it fails on at least 4."""
    from slamhip import icp, sig as gsig, synthetic
    seq = synthetic.make_loop_sequence(700, seed=5, n_beams=361)
    rng = np.random.default_rng(2)
    pc1, pc2, ks, truth = [], [], [], []
    for i, j in seq.loop_pairs[:12]:
        turn = rng.uniform(-np.pi, np.pi)
        later = turned([seq.scans[j]], [turn])[0]
        sg = gsig.build_signatures(icp.ScanSet([seq.scans[i], later]))
        jj, d, k, count = gsig.match_signatures(sg, [1], 1, (1, 1))
        assert jj[0, 0] == 1 and count[0] == 1
        ks.append(k[0, 0])
        pc1.append(later)
        pc2.append(seq.scans[i])
        truth.append(_truth_tf(seq, i, j, turn))

    def good(r):
        ok = []
        for t, e, want in zip(r.tf, r.err, truth):
            dth = np.arctan2(t[1, 0], t[0, 0]) - np.arctan2(want[1, 0], want[0, 0])
            dth = abs(np.arctan2(np.sin(dth), np.cos(dth)))
            ok.append(np.hypot(*(t[:2, 2] - want[:2, 2])) <= 0.1 and dth <= 0.02 and e < 30)
        return np.array(ok)
    seeded = good(icp.icp_pairs(pc1, pc2, gsig.shift_inits(ks, 64), epsilon=0.05, max_iters=100))
    plain = good(icp.icp_pairs(pc1, pc2, np.tile(np.eye(3), (12, 1, 1)), epsilon=0.05, max_iters=100))
    print(f"seeded {int(seeded.sum())} of 12, identity {int(plain.sum())} of 12")
    assert seeded.all()
    assert (~plain).sum() >= 4


class _Graph:
    def __init__(self, poses):
        self.poses = poses
        self.added = []

    def add_constraint(self, i, j, tf):
        self.added.append((i, j, np.array(tf)))


@pytest.fixture(scope="module")
def wiring():
    """Three laps of a small loop (step 0.2 m: 132 scans a lap), frames turned,
    and the constraints of a host replay: sig_ref candidates, the existing
    icp_batch from the shifts' rotations, the greedy pass."""
    from slamhip import icp, lcd, sig as gsig, synthetic
    seq = synthetic.make_loop_sequence(400, seed=5, n_beams=181, step=0.2)
    scans = turned(seq.scans, np.random.default_rng(3).uniform(-np.pi, np.pi, 400))
    sig = sig_ref.signatures(scans, *sig_ref.tables(64))[0]
    start, n_rows = lcd.path_starts(seq.odometry, 5)
    cand = sig_ref.candidates(sig, start, n_rows, 1, 4)
    assert len(cand) > 100
    r = icp.icp_batch(scans, [j for _, j, _ in cand], [i for i, _, _ in cand],
                      gsig.shift_inits([k for _, _, k in cand], 64), epsilon=0.05, max_iters=100)
    used, want = set(), []
    for b, (i, j, _) in enumerate(cand):
        if i in used or j in used or not float(r.err[b]) < 110:
            continue
        want.append((i, j, r.tf[b].copy()))
        used.update((i, j))
    assert len(want) > 20
    return seq, scans, cand, want


def _same_constraints(added, want):
    assert [(i, j) for i, j, _ in added] == [(i, j) for i, j, _ in want]
    for (_, _, a), (_, _, b) in zip(added, want):
        assert np.array_equal(a, b)


def test_pipeline_stage(wiring):
    from slamhip import icp, pipeline
    seq, scans, cand, want = wiring
    g = _Graph(seq.odometry.copy())
    got, accepted = pipeline.signature_loop_closures(g, scans, scanset=icp.ScanSet(scans))
    assert got == cand and accepted.dtype == bool and accepted.sum() == len(want)
    _same_constraints(g.added, want)
    assert [(i, j) for (i, j, _), ok in zip(got, accepted) if ok] == [(i, j) for i, j, _ in want]
    g2 = _Graph(seq.odometry.copy())
    pipeline.signature_loop_closures(g2, scans, init="identity")
    assert len(g2.added) < len(want)   # the frames are turned: most need the shift
    with pytest.raises(ValueError, match="init"):
        pipeline.signature_loop_closures(g, scans, init="bogus")
    with pytest.raises(ValueError, match="init"):
        pipeline.proximity_loop_closures(g, scans, init="signature")   # this stage's init only


def test_detect_signatures(wiring):
    import src.loop_closure_detection as host
    seq, scans, _, want = wiring
    g = _Graph(seq.odometry.copy())
    assert host.detect_signatures(g, scans) is None
    _same_constraints(g.added, want)


def test_cli_signatures(wiring, tmp_path):
    import main_batched as mb
    from slamhip import dataset
    seq, scans, cand, want = wiring
    dataset.save(str(tmp_path / "loop.npz"), seq.odometry, scans)
    rep = mb.run(mb.parse([str(tmp_path / "loop.npz"), "--loop-closure-detection", "signatures", "--skip-icp",
                           "--program-end", "loop_closure", "--results-dir", str(tmp_path),
                           "--skip-occupancy-grid"]))
    det = rep["loop_closure_detection"]
    assert det["method"] == "signatures" and det["candidates"] == len(cand) and det["accepted"] == len(want)
    import src.pose_graph as pose_graph
    pg = pose_graph.PoseGraph(None)
    pg.load(str(tmp_path / "loop_closure_pose_graph.pickle"))
    ea, eb, tf = pg.edge_arrays()
    loops = {(int(a), int(b)): t for a, b, t in zip(ea, eb, tf) if abs(int(a) - int(b)) > 1}
    assert sorted(loops) == sorted((i, j) for i, j, _ in want)
    for i, j, t in want:
        assert np.array_equal(loops[(i, j)], t)
        assert pg.graph.edges[i, j]["convention"] == "relative"
    with pytest.raises(SystemExit):
        mb.parse(["x.npz", "--signature-max-frac", "3/2"])
