"""Correlative scan matcher on the GPU against its NumPy restatement
(tests/csm_ref.py): exact score volumes, the tie rule, independence of the
batch, and the end-to-end experiment — loop pairs seen from a frame turned by
any angle, where ICP from the identity fails and ICP seeded by the matcher
does not.  The opt-in wiring of the loop-closure paths is checked on the same
pairs."""
import numpy as np
import pytest

import csm_ref
from conftest import homog

pytestmark = pytest.mark.gpu

SHAPES = {
    "odd": dict(n_theta=9, d_theta=0.05, nx=7, ny=5, G=128, res=0.1),
    # even windows; at +-8 m many reference and query points fall outside the grid, windows reach over its edge
    "even": dict(n_theta=1, d_theta=0.05, nx=8, ny=6, G=64, res=0.25),
}


class Case:
    """B = 6 pairs over scans of 61 and 130 points, distinct non-zero centres."""

    def __init__(self):
        from slamhip import synthetic
        a = synthetic.make_sequence(4, seed=1, n_beams=61)
        b = synthetic.make_sequence(4, seed=2, n_beams=130)
        self.scans = a.scans + b.scans
        assert sorted({len(s) for s in self.scans}) == [61, 130]
        self.src = np.array([1, 2, 3, 5, 6, 0])
        self.dst = np.array([0, 0, 1, 4, 4, 5])
        self.centre = np.array([[0.10, 0.30, -0.20], [-0.20, -0.15, 0.25], [0.05, 0.45, 0.35],
                                [-0.07, -0.40, -0.30], [0.31, 0.12, 0.52], [-0.33, 0.27, -0.11]])
        self.ref = {}
        for name, kw in SHAPES.items():
            vols = [csm_ref.score_volume(self.scans[s], self.scans[d], c, **kw)[0]
                    for s, d, c in zip(self.src, self.dst, self.centre)]
            self.ref[name] = np.stack(vols)
            self.ref[name].setflags(write=False)


@pytest.fixture(scope="module")
def case():
    return Case()


def _params(name):
    from slamhip.csm import CsmParams
    return CsmParams(**SHAPES[name])


def _expect(ref):
    """(index (B, 3), score (B,)) of reference volumes."""
    bests = [csm_ref.best(S) for S in ref]
    return np.array([b[1] for b in bests]), np.array([b[0] for b in bests])


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_volumes(case, name):
    from slamhip.csm import csm_batch
    kw = SHAPES[name]
    r = csm_batch(case.scans, case.src, case.dst, case.centre, _params(name), return_scores=True)
    assert r.scores.dtype == np.int32 and r.scores.shape == case.ref[name].shape
    assert case.ref[name].max() > 0
    assert np.array_equal(r.scores, case.ref[name])
    index, score = _expect(case.ref[name])
    assert np.array_equal(r.index, index) and np.array_equal(r.score, score)
    assert np.array_equal(r.n_query, [len(case.scans[s]) for s in case.src])
    for b in range(len(case.src)):
        cs = csm_ref.angle_table(case.centre[b, 0], kw["n_theta"], kw["d_theta"])
        want = csm_ref.transform(cs, tuple(index[b]), case.centre[b], kw["res"], kw["nx"], kw["ny"])
        assert np.array_equal(r.tf[b], want)
    # without the volume the answer is the same
    q = csm_batch(case.scans, case.src, case.dst, case.centre, _params(name))
    assert q.scores is None and np.array_equal(q.index, r.index) and np.array_equal(q.score, r.score)
    assert np.array_equal(q.tf, r.tf)


@pytest.mark.parametrize("name", list(SHAPES))
def test_byte_gathers_agree(case, name):
    """The score kernel's byte-gather form (slam_csm_set_gather(1); dword
    gathers are the default the other tests run) gives the same volumes."""
    from slamhip import _abi
    from slamhip.csm import csm_batch
    lib = _abi.lib()
    assert lib.slam_csm_set_gather(1) == 0
    try:
        r = csm_batch(case.scans, case.src, case.dst, case.centre, _params(name), return_scores=True)
    finally:
        assert lib.slam_csm_set_gather(4) == 0
    index, score = _expect(case.ref[name])
    assert np.array_equal(r.scores, case.ref[name])
    assert np.array_equal(r.index, index) and np.array_equal(r.score, score)


def test_wide_window_and_long_scan():
    """More slots than one pass holds (a 170 x 50 window) and more query
    points than one LDS tile (5,000): the multi-pass and multi-tile paths of
    both gather forms against the restatement."""
    from slamhip import _abi
    from slamhip.csm import CsmParams, csm_batch
    rng = np.random.default_rng(7)
    ref = rng.uniform(-3.0, 3.0, size=(400, 2))
    query = np.r_[ref[rng.integers(0, 400, size=5000)] + rng.normal(0, 0.02, size=(5000, 2)) - [0.4, -0.3]]
    kw = dict(n_theta=2, d_theta=0.1, nx=50, ny=170, G=128, res=0.1)
    want, _ = csm_ref.score_volume(query, ref, (0.05, 0.1, -0.1), **kw)
    lib = _abi.lib()
    for width in (1, 4):
        assert lib.slam_csm_set_gather(width) == 0
        try:
            r = csm_batch([query, ref], [0], [1], [[0.05, 0.1, -0.1]], CsmParams(**kw), return_scores=True)
        finally:
            assert lib.slam_csm_set_gather(4) == 0
        assert np.array_equal(r.scores[0], want), width
        assert (int(r.score[0]), tuple(int(v) for v in r.index[0])) == csm_ref.best(want)


def test_ties_every_angle():
    """Reference = query = the single point (0, 0): every angle ties."""
    from slamhip.csm import CsmParams, csm_batch
    kw = dict(n_theta=5, d_theta=0.3, nx=7, ny=5, G=64, res=0.1)
    p = CsmParams(**kw)
    r = csm_batch([np.zeros((1, 2))], [0], [0], params=p, return_scores=True)
    assert r.score[0] == 2 and tuple(r.index[0]) == (0, p.ny // 2, p.nx // 2)
    assert (r.scores[0, :, p.ny // 2, p.nx // 2] == 2).all()
    assert np.array_equal(r.scores[0], csm_ref.score_volume(np.zeros((1, 2)), np.zeros((1, 2)), **kw)[0])


def test_query_outside_the_grid(case):
    """A query entirely outside the grid: all scores 0, index (0, 0, 0)."""
    from slamhip.csm import csm_batch
    q = np.c_[np.full(70, 1e3), np.linspace(-1.0, 1.0, 70)]
    r = csm_batch([q, case.scans[0]], [0], [1], params=_params("odd"), return_scores=True)
    assert not r.scores.any() and r.score[0] == 0 and tuple(r.index[0]) == (0, 0, 0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_far_point_changes_nothing(case, name):
    """One extra query point at (1e12, -1e12) is simply outside: no overflow."""
    from slamhip.csm import csm_batch
    scans = list(case.scans)
    src = []
    for s in case.src:
        scans.append(np.r_[case.scans[s], [[1e12, -1e12]]])
        src.append(len(scans) - 1)
    r = csm_batch(scans, src, case.dst, case.centre, _params(name), return_scores=True)
    assert np.array_equal(r.scores, case.ref[name])
    assert np.array_equal(r.n_query, [len(case.scans[s]) + 1 for s in case.src])


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_independence(case, name):
    from slamhip.csm import csm_batch
    from slamhip.icp import ScanSet
    ss = ScanSet(case.scans)
    p = _params(name)
    full = csm_batch(ss, case.src, case.dst, case.centre, p, return_scores=True)
    for b in range(len(case.src)):
        one = csm_batch(ss, case.src[b:b + 1], case.dst[b:b + 1], case.centre[b:b + 1], p, return_scores=True)
        assert np.array_equal(one.scores[0], full.scores[b])
        assert np.array_equal(one.index[0], full.index[b]) and one.score[0] == full.score[b]
        assert np.array_equal(one.tf[0], full.tf[b])
    perm = np.array([4, 2, 5, 0, 3, 1])
    sh = csm_batch(ss, case.src[perm], case.dst[perm], case.centre[perm], p, return_scores=True)
    assert np.array_equal(sh.scores, full.scores[perm]) and np.array_equal(sh.index, full.index[perm])
    assert np.array_equal(sh.score, full.score[perm]) and np.array_equal(sh.tf, full.tf[perm])


def test_non_finite_points_raise(case):
    from slamhip.csm import csm_batch
    bad = case.scans[0].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        csm_batch([bad, case.scans[1]], [0], [1], params=_params("odd"))
    with pytest.raises(ValueError, match="non-finite"):
        csm_batch(case.scans, [0], [1], centre=[[np.inf, 0, 0]], params=_params("odd"))


# ---- end to end: loop pairs seen from a frame turned by any angle ------------------------------------

def _M(p):
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def loop_seq():
    from slamhip import synthetic
    return synthetic.make_loop_sequence(700, seed=5, n_beams=361)


class Drifted:
    def __init__(self, seq):
        rng = np.random.default_rng(2)
        self.query, self.ref, self.truth = [], [], []
        for a, b in seq.loop_pairs[:12]:
            al = rng.uniform(-np.pi, np.pi)
            dx = rng.uniform(-1.2, 1.2)
            dy = rng.uniform(-1.2, 1.2)
            D = np.array([[np.cos(al), -np.sin(al), dx], [np.sin(al), np.cos(al), dy], [0, 0, 1.0]])
            q = homog(seq.scans[b]) @ np.linalg.inv(D).T
            self.query.append(homog(q[:, :2]))            # the homogeneous coordinate exactly 1 again
            self.ref.append(homog(seq.scans[a]))
            self.truth.append(np.linalg.inv(_M(seq.truth[a])) @ _M(seq.truth[b]) @ D)
        assert len(self.query) == 12


@pytest.fixture(scope="module")
def drifted(loop_seq):
    return Drifted(loop_seq)


def _pose_error(tf, truth):
    d = np.arctan2(tf[1, 0], tf[0, 0]) - np.arctan2(truth[1, 0], truth[0, 0])
    return np.hypot(*(tf[:2, 2] - truth[:2, 2])), abs(np.arctan2(np.sin(d), np.cos(d)))


def test_csm_seeds_loop_closure_icp(drifted):
    from slamhip.csm import csm_batch
    from slamhip.icp import icp_pairs
    scans = [s[:, :2] for s in drifted.query + drifted.ref]
    m = csm_batch(scans, np.arange(12), np.arange(12, 24))
    seeded = icp_pairs(drifted.query, drifted.ref, m.tf, epsilon=0.05, max_iters=100)
    plain = icp_pairs(drifted.query, drifted.ref, np.stack([np.eye(3)] * 12), epsilon=0.05, max_iters=100)
    plain_failures = 0
    for b in range(12):
        raw = _pose_error(m.tf[b], drifted.truth[b])
        fine = _pose_error(seeded.tf[b], drifted.truth[b])
        ident = _pose_error(plain.tf[b], drifted.truth[b])
        print(f"pair {b}: csm {raw[0]:.3f} m {raw[1]:.4f} rad score {m.score[b]}/{2 * m.n_query[b]}; "
              f"csm+icp {fine[0]:.3f} m {fine[1]:.4f} rad err {seeded.err[b]:.3f}; "
              f"identity+icp {ident[0]:.3f} m {ident[1]:.4f} rad err {plain.err[b]:.1f}")
        assert raw[0] <= 0.1 and raw[1] <= 0.05, (b, raw)
        assert seeded.err[b] < 30 and fine[0] <= 0.1 and fine[1] <= 0.02, (b, fine, seeded.err[b])
        plain_failures += not (plain.err[b] < 30 and ident[0] <= 0.1 and ident[1] <= 0.02)
    assert plain_failures >= 4, plain_failures


def _graph_bytes(pg):
    return [(a, b, np.asarray(t).tobytes()) for a, b, t in pg.graph.edges(data="object")]


def test_wiring_manual_loop_closures(drifted):
    """init="csm" accepts all 12 drifted pairs, the default at most 8;
    init="identity" is the default call, byte for byte."""
    import src.pose_graph as pgm
    from slamhip import pipeline
    scans = [s[:, :2] for s in drifted.ref + drifted.query]      # the drifted scans as extra scans 12..23
    pairs = np.stack([np.arange(12, 24), np.arange(12)], axis=1)  # icp(pc_i = query, pc_j = reference)
    graphs = {}
    for key, kw in (("default", {}), ("identity", dict(init="identity")), ("csm", dict(init="csm"))):
        pg = pgm.PoseGraph(np.zeros((24, 3)))
        ok = pipeline.manual_loop_closures(pg, scans, pairs, **kw)
        graphs[key] = (pg, ok)
        assert pg.graph.number_of_edges() == 23 + int(ok.sum())
    assert graphs["csm"][1].sum() == 12
    assert graphs["default"][1].sum() <= 8
    assert np.array_equal(graphs["default"][1], graphs["identity"][1])
    assert _graph_bytes(graphs["default"][0]) == _graph_bytes(graphs["identity"][0])
    pg = graphs["csm"][0]
    for b, (i, j) in enumerate(pairs):
        d, a = _pose_error(pg.graph.edges[int(i), int(j)]["object"], drifted.truth[b])
        assert d <= 0.1 and a <= 0.02, (b, d, a)


def test_wiring_detect_proximity_keyword(loop_seq):
    """The drop-in's trailing keyword: "identity" is the default call byte for
    byte; "csm" runs the matcher (here a small window) on the same candidates."""
    import src.loop_closure_detection as lcd
    import src.pose_graph as pgm
    from slamhip.csm import CsmParams
    seq = loop_seq
    small = CsmParams(n_theta=9, d_theta=0.02, nx=21, ny=21)
    graphs = []
    for kw in ({}, dict(init="identity"), dict(init="csm", csm=small)):
        pg = pgm.PoseGraph(seq.odometry.copy())
        lcd.detect_proximity(pg, seq.scans, min_dist_along_path=2, max_dist=1, err_thresh=110, **kw)
        graphs.append(pg)
    n0 = len(seq.truth) - 1
    assert graphs[0].graph.number_of_edges() > n0
    assert _graph_bytes(graphs[0]) == _graph_bytes(graphs[1])
    assert graphs[2].graph.number_of_edges() > n0
