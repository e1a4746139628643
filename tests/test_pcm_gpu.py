"""GPU tests of the pairwise-consistency check (csrc/pcm_kernels.hip,
slamhip.pcm) and of the stage, the drop-in function and the command-line switch
that use it.

The yardstick is the NumPy restatement tests/pcm_ref.py, which tests/test_pcm.py
pins to plain double loops.  Every comparison is ``np.array_equal``: adjacency
words, degrees, removal order, keep mask and step count are decided by
individually rounded fp64 operations and integers alone.
"""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

import pcm_ref
from test_pcm import TOL, drifting_case, random_case

sys.path.insert(0, os.path.join(PKG, "scripts"))

pytestmark = pytest.mark.gpu


def _params(tol=TOL, min_size=2):
    from slamhip import pcm
    return pcm.PcmParams(trans_tol=tol[0], trans_drift=tol[1], rot_tol=tol[2], rot_drift=tol[3], min_size=min_size)


def _mats(Z):
    """(L, 3, 3) matrices of float64[L][4] elements: the same doubles."""
    T = np.zeros((len(Z), 3, 3))
    T[:, 0, 0], T[:, 1, 0], T[:, 0, 2], T[:, 1, 2] = Z[:, 0], Z[:, 1], Z[:, 2], Z[:, 3]
    T[:, 0, 1], T[:, 1, 1], T[:, 2, 2] = -Z[:, 1], Z[:, 0], 1.0
    return T


def _device(X, a, b, Z, tol=TOL, min_size=2, **kw):
    """slamhip.pcm.consistency on given elements X (float64[N][4]), so that the
    kernels and the restatement see the same bits."""
    from slamhip import pcm
    return pcm.consistency(X, a, b, _mats(Z), _params(tol, min_size), return_adjacency=True, **kw)


def _check(X, a, b, Z, tol=TOL, min_size=2, **kw):
    got = _device(X, a, b, Z, tol, min_size, **kw)
    adj, deg = pcm_ref.adjacency(X, a, b, Z, tol)
    order, keep, steps = pcm_ref.select(adj, deg, min_size)
    assert got.adjacency.dtype == np.uint32 and np.array_equal(got.adjacency, adj)
    assert np.array_equal(got.degree, deg)
    assert np.array_equal(got.order, order)
    assert got.keep.dtype == bool and np.array_equal(got.keep, keep.astype(bool))
    assert got.steps == steps
    return got


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049])
def test_random_closures(L):
    """Word, wave, column-tile (256) and peel-workgroup (1,024) boundaries."""
    X, a, b, Z = random_case(L, 1000 + L, N=60)
    got = _check(X, a, b, Z)
    if L >= 63:
        assert 0 < got.steps < L - 1 and got.keep.any()


@pytest.mark.parametrize("seed", [0, 2])
def test_lap_graphs(seed):
    from slamhip import pcm
    poses, a, b, Z, inlier = drifting_case(seed)
    got = pcm.consistency(poses, a, b, Z, _params(), return_adjacency=True)
    keep, deg, order, steps, adj = pcm_ref.consistency(poses, a, b, Z, TOL)
    assert np.array_equal(got.adjacency, adj) and np.array_equal(got.degree, deg)
    assert np.array_equal(got.order, order) and np.array_equal(got.keep, keep) and got.steps == steps
    assert not got.keep[~inlier].any() and got.keep[inlier].sum() >= 57


def threshold_case():
    """Closures over a chain of identity poses, so that E of the pair (0, k) is
    the pure translation by -d_k and dt = d_k d_k exactly; a_k = n_k makes the
    bound tol^2 + drift^2 n_k.  d_k is chosen among the doubles next to the
    bound's square root so that d_k d_k equals the bound to the last bit (odd k)
    or is the next double above it (even k >= 2).  Returns the number of each."""
    tt0, ttd = np.float64(TOL[0]), np.float64(TOL[1])
    on, over = [], []
    for n in range(0, 400):
        bound = tt0 * tt0 + (ttd * ttd) * np.float64(n)
        d = np.sqrt(bound)
        for _ in range(3):
            d = np.nextafter(d, 0.0)
        for _ in range(7):
            if d * d == bound:
                on.append((n, d))
            elif d * d == np.nextafter(bound, np.inf):
                over.append((n, d))
            d = np.nextafter(d, np.inf)
    m = min(len(on), len(over), 40)
    picks = [p for pair in zip(on[:m], over[:m]) for p in pair]
    N = 401
    X = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
    a = np.array([0] + [n for n, _ in picks])
    b = np.zeros(len(a), dtype=np.int64)
    Z = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (len(a), 1))
    Z[1:, 2] = [-d for _, d in picks]
    return X, a, b, Z, m


def test_verdicts_on_the_threshold():
    X, a, b, Z, m = threshold_case()
    assert m >= 10
    got = _check(X, a, b, Z)
    row0 = pcm_ref.unpack(got.adjacency, len(a))[0]
    assert row0[1::2].all() and not row0[2::2].any()   # dt == bound: consistent; one ulp above: not


def test_duplicates_reversed_pairs_and_nan():
    X, a, b, Z = random_case(130, 5, N=30)
    a[40:80], b[40:80], Z[40:80] = a[:40], b[:40], Z[:40]                   # duplicates
    a[80:120], b[80:120], Z[80:120] = b[:40], a[:40], pcm_ref.inv(Z[:40])   # (b, a) with the inverse measurement
    Z[7, 3] = np.nan
    Z[100, 0] = np.nan
    got = _check(X, a, b, Z)
    assert got.degree[7] == 0 and got.degree[100] == 0 and not got.keep[7] and got.order[7] >= 0
    full = pcm_ref.unpack(got.adjacency, 130)
    assert full[0, 40] and full[1, 41]   # a closure is consistent with its copy


def test_peel_instantiations_give_the_same_result():
    from slamhip import _abi
    X, a, b, Z = random_case(257, 11, N=60)
    want = _check(X, a, b, Z)
    lib = _abi.lib()
    try:
        for slots in (1, 4, 16, 64):
            assert lib.slam_pcm_set_peel_slots(slots) == 0
            got = _check(X, a, b, Z)
            assert np.array_equal(got.order, want.order)
    finally:
        assert lib.slam_pcm_set_peel_slots(0) == 0


def _select(adj, deg, min_size=2):
    """slam_pcm_select on a given packed matrix: ``(order, keep, steps)``."""
    import torch
    from slamhip import _abi
    lib = _abi.lib()
    L = len(deg)
    d_adj = torch.from_numpy(np.ascontiguousarray(adj).view(np.int32)).cuda()
    d_deg = torch.from_numpy(np.ascontiguousarray(deg, dtype=np.int32)).cuda()
    d_order = torch.empty(L, dtype=torch.int32, device="cuda")
    d_keep = torch.empty(L, dtype=torch.uint8, device="cuda")
    d_steps = torch.empty(1, dtype=torch.int32, device="cuda")
    _abi.check(lib.slam_pcm_select(d_adj.data_ptr(), d_deg.data_ptr(), L, min_size, d_order.data_ptr(),
                                   d_keep.data_ptr(), d_steps.data_ptr(), None), "slam_pcm_select")
    assert lib.slam_pcm_status(None) == 0
    assert np.array_equal(d_deg.cpu().numpy(), deg)   # only read
    return d_order.cpu().numpy(), d_keep.cpu().numpy(), int(d_steps.cpu().numpy()[0])


def test_select_alone_4097():
    """16 closures a thread: a random graph of 3,900 mutually consistent closures
    and 197 with few neighbours, against the restatement."""
    L = 4097
    rng = np.random.default_rng(3)
    full = np.zeros((L, L), dtype=bool)
    core = rng.permutation(L)[:3900]
    full[np.ix_(core, core)] = True
    sparse = np.setdiff1d(np.arange(L), core)
    for s in sparse:
        nb = rng.choice(L, int(rng.integers(0, 3000)), replace=False)
        full[s, nb] = full[nb, s] = True
    np.fill_diagonal(full, False)
    adj, deg = pcm_ref.pack(full), full.sum(1).astype(np.int32)
    order, keep, steps = _select(adj, deg)
    want = pcm_ref.select(adj, deg)
    assert np.array_equal(order, want[0]) and np.array_equal(keep, want[1]) and steps == want[2]
    assert steps == 197 and keep.sum() == 3900


def test_select_alone_16385():
    """64 closures a thread, closed forms (tests/test_pcm.py has them at L = 40):
    nothing consistent leaves index 0 after L - 1 removals from the highest index
    down; everything consistent takes no step."""
    L = 16385
    W = (L + 31) // 32
    order, keep, steps = _select(np.zeros((L, W), np.uint32), np.zeros(L, np.int32), min_size=1)
    assert steps == L - 1 and keep[0] == 1 and not keep[1:].any()
    assert np.array_equal(order, np.r_[-1, np.arange(L - 2, -1, -1)])
    adj = np.full((L, W), 0xFFFFFFFF, np.uint32)
    adj[:, -1] = (1 << (L % 32)) - 1
    idx = np.arange(L)
    adj[idx, idx >> 5] &= ~(np.uint32(1) << (idx & 31).astype(np.uint32))
    order, keep, steps = _select(adj, np.full(L, L - 1, np.int32))
    assert steps == 0 and keep.all() and (order == -1).all()


def test_repeat_side_stream_flag_and_edge_cases():
    import torch
    from slamhip import _abi, pcm
    X, a, b, Z = random_case(300, 21, N=50)
    first = _check(X, a, b, Z)
    for kw in ({}, dict(stream=torch.cuda.Stream())):
        again = _device(X, a, b, Z, **kw)
        assert np.array_equal(again.adjacency, first.adjacency) and np.array_equal(again.order, first.order)
        assert np.array_equal(again.keep, first.keep) and again.steps == first.steps
    # what only the device sees: an index outside [0, N) is flagged, reported once, and nothing is read through it
    for arr, bad in ((a, -1), (b, 50), (a, 1 << 40)):
        saved = arr[150]
        arr[150] = bad
        with pytest.raises(_abi.SlamHipError, match="status -1.*index"):
            _device(X, a, b, Z)
        arr[150] = saved
        again = _device(X, a, b, Z)
        assert np.array_equal(again.adjacency, first.adjacency) and np.array_equal(again.order, first.order)
    # no closure; fewer kept than min_size
    none = pcm.consistency(X, [], [], np.zeros((0, 3, 3)), _params(), return_adjacency=True)
    assert none.keep.shape == (0,) and none.steps == 0 and none.adjacency.shape == (0, 0)
    size = int(first.keep.sum())
    assert size >= 2
    big = _check(X, a, b, Z, min_size=size + 1)
    assert not big.keep.any() and np.array_equal(big.order, first.order) and big.steps == first.steps
    assert _check(X, a, b, Z, min_size=size).keep.sum() == size
    with pytest.raises(ValueError):
        pcm.PcmParams(trans_tol=-1.0)
    with pytest.raises(ValueError):
        pcm.consistency(X, a, b[:-1], _mats(Z))


@pytest.fixture(scope="module")
def lap_pose_graph():
    """The 160-node graph of seed 0 as a PoseGraph maker: the inliers in the
    "relative" convention, every other outlier re-expressed in the "icp" one."""
    import src.pose_graph as pose_graph
    poses, a, b, Z, inlier = drifting_case(0)

    def make():
        pg = pose_graph.PoseGraph(poses.copy())
        flip = False
        for i, j, T, good in zip(a, b, Z, inlier):
            if good or not flip:
                pg.add_constraint(int(i), int(j), T.copy(), convention="relative")
            else:
                pg.add_constraint(int(j), int(i), T.copy(), convention="icp")   # X_j' = X_i' T with the ends swapped
            flip = flip != (not good)
        return pg
    inliers = {(int(i), int(j)): T for i, j, T, good in zip(a, b, Z, inlier) if good}
    assert make().graph.number_of_edges() == 159 + len(a) and len(inliers) == 60
    return make, inliers, int((~inlier).sum())


def _loop_edges(pg):
    return {(i, j): d["object"] for i, j, d in pg.graph.edges(data=True) if d.get("constraint")}


def _only_inliers(pg, inliers):
    left = _loop_edges(pg)
    assert sorted(left) == sorted(inliers) and pg.graph.number_of_edges() == 159 + len(inliers)
    for key, T in inliers.items():
        assert np.array_equal(left[key], T) and pg.graph.edges[key]["convention"] == "relative"


def test_verify_loop_closures(lap_pose_graph):
    from slamhip import pipeline
    make, inliers, n_out = lap_pose_graph
    pg = make()
    conv = [pg.graph.edges[i, j]["convention"] for i, j in _loop_edges(pg) if (i, j) not in inliers]
    assert conv.count("icp") >= n_out // 2 - 1 and conv.count("relative") >= n_out // 2 - 1
    ea_before = pg.edge_arrays()[0]
    edges, keep, unverified = pipeline.verify_loop_closures(pg, _params(), remove=False)
    assert len(edges) == 60 + n_out and keep.sum() == 60 and unverified == 0
    assert [(i, j) in inliers for i, j, _ in edges] == keep.tolist()
    assert pg.graph.number_of_edges() == 159 + 60 + n_out            # remove=False: untouched
    edges2, keep2, _ = pipeline.verify_loop_closures(pg, _params())
    assert np.array_equal(keep, keep2)
    _only_inliers(pg, inliers)
    assert len(pg.edge_arrays()[0]) == len(ea_before) - n_out        # the cache was dropped
    # an edge without a convention is counted and left alone; a graph without closures is fine
    pg.add_constraint(3, 90, np.eye(3))
    edges3, keep3, unverified = pipeline.verify_loop_closures(pg, _params())
    assert unverified == 1 and keep3.all() and len(edges3) == 60 and pg.graph.has_edge(3, 90)
    import src.pose_graph as pose_graph
    bare = pose_graph.PoseGraph(pg.poses.copy())
    e, k, u = pipeline.verify_loop_closures(bare, _params())
    assert e == [] and k.shape == (0,) and u == 0
    with pytest.raises(Exception):
        pg.remove_constraint(5, 100)   # no such edge


def test_filter_consistent(lap_pose_graph):
    import src.loop_closure_detection as host
    make, inliers, n_out = lap_pose_graph
    pg = make()
    edges, keep, unverified = host.filter_consistent(pg, _params())
    assert keep.sum() == 60 and len(edges) == 60 + n_out and unverified == 0
    _only_inliers(pg, inliers)


def test_cli_consistency(lap_pose_graph, tmp_path):
    import main_batched as mb
    import src.pose_graph as pose_graph
    from slamhip import dataset
    make, inliers, n_out = lap_pose_graph
    pg = make()
    pg.save(str(tmp_path / "in.pickle"))
    scans = [np.array([[1.0, 0.0], [0.0, 1.0]])] * len(pg.poses)
    dataset.save(str(tmp_path / "lap.npz"), pg.poses, scans)
    base = [str(tmp_path / "lap.npz"), "--program-start", "loop_closure", "--program-end", "loop_closure",
            "--pose-graph", str(tmp_path / "in.pickle"), "--skip-occupancy-grid"]
    tol = ["--consistency-trans-tol", str(TOL[0]), "--consistency-trans-drift", str(TOL[1]),
           "--consistency-rot-tol", str(TOL[2]), "--consistency-rot-drift", str(TOL[3])]
    rep = mb.run(mb.parse(base + ["--results-dir", str(tmp_path / "on"), "--loop-closure-consistency"] + tol))
    block = rep["loop_closure_consistency"]
    assert (block["closures"], block["kept"], block["removed"], block["unverified"]) == (60 + n_out, 60, n_out, 0)
    assert block["steps"] >= n_out and block["seconds"] >= 0
    out = pose_graph.PoseGraph(None)
    out.load(str(tmp_path / "on" / "loop_closure_pose_graph.pickle"))
    _only_inliers(out, inliers)
    # without the flag: no block, and the graph goes through as it came
    rep = mb.run(mb.parse(base + ["--results-dir", str(tmp_path / "off")]))
    assert "loop_closure_consistency" not in rep
    off = pose_graph.PoseGraph(None)
    off.load(str(tmp_path / "off" / "loop_closure_pose_graph.pickle"))
    assert list(off.graph.edges) == list(pg.graph.edges)
    for (_, _, x), (_, _, y) in zip(off.graph.edges(data=True), pg.graph.edges(data=True)):
        assert np.array_equal(x["object"], y["object"]) and x.get("convention") == y.get("convention")
    with pytest.raises(SystemExit):
        mb.parse(["x.npz", "--consistency-trans-tol", "-1"])
