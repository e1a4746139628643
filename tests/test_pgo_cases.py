"""CPU checks of the inputs of tests/test_pgo_paths_gpu.py (tests/pgo_cases.py).

The GPU tests are only as good as their graphs: here every graph is shown to
(1) stay >= 1e-4 rad away from the heading residual's wrap point in both steps
(a condition on the inputs: asserted, never skipped), (2) contain the
structural relations it is named for, computed from (a, b, shift) alone, (3)
exercise both outcomes of the clamp, and the restatement that measures all
this is bit-identical to the oracle.  The relaxation's launch plan is pinned at
every dispatch boundary (host-only query, no GPU).
"""
import ctypes

import numpy as np
import pytest

import pgo_cases as pc
import pgo_oracle as po

KEYS = pc.graph_keys()
IDS = [f"{k}-N{n}-sh{s}" for k, n, s in KEYS]


def _check_steps(c, both_clamp_outcomes):
    for lr in pc.LRS:
        got, margin, clamped, unclamped = pc.residual_margin(c.poses.copy(), c.ea, c.eb, c.tf, lr)
        assert np.array_equal(got, c.ref[lr]), (c.name, lr)           # restatement == oracle, bit for bit
        assert margin >= pc.MARGIN, (c.name, lr, margin)
        assert clamped + unclamped == 3 * len(c.active)
        # beta = 2 (b - a) lr r up to rounding (d = 2 r / sigma, gamma = 1 / sigma):
        # clamped to r exactly when 2 (b - a) lr > 1; at b - a = 25 and lr = 0.02
        # rounding decides, and both outcomes give the same beta to 1e-16
        long_ = sum(2 * (b - a) * lr > 1.001 for a, b in c.active)
        edge_ = sum(0.999 <= 2 * (b - a) * lr <= 1.001 for a, b in c.active)
        assert 3 * long_ <= clamped <= 3 * (long_ + edge_), (c.name, lr, clamped, long_, edge_)
        if lr == 0.02 and both_clamp_outcomes:
            assert clamped > 0 and unclamped > 0, (c.name, clamped, unclamped)
    assert not np.array_equal(c.ref[1.0], c.ref[0.02]) or not c.active


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_graph_steps(key):
    c = pc.case(*key)
    assert len(c.pairs) == len(set(c.pairs)) and all(0 <= a < c.N and 0 <= b < c.N for a, b in c.pairs)
    # an edge longer than 25 nodes needs N >= 28: the tiny graphs cannot clamp at lr = 0.02
    _check_steps(c, both_clamp_outcomes=c.N >= 41)
    assert np.array_equal(c.ref[1.0][:c.first_a() + 1], c.poses[:c.first_a() + 1])


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] == "structural"],
                         ids=[i for i, k in zip(IDS, KEYS) if k[0] == "structural"])
def test_structural_relations(key):
    _, N, shift = key
    c = pc.case(*key)
    have = pc.relations(c.pairs, N, shift)
    want = pc.expected_relations(N, shift)
    assert want <= have, (c.name, sorted(want - have))
    assert c.first_a() == 0 and c.pairs[0] == (0, N - 1)
    if N >= 41:
        assert (N - 1, 4) in c.pairs and (10, 11) in c.pairs          # reversed, odometry-shaped
        act = c.active
        nested = any(a < a2 and b2 < b for a, b in act for a2, b2 in act)
        overlap = any(a < a2 < b < b2 for a, b in act for a2, b2 in act)
        assert nested and overlap


def test_structural_relations_cover_every_name():
    """Over the whole set, every relation the kernel distinguishes appears, and
    the sh >= 9 graphs have more explicit nodes than prefetched slots."""
    seen = set()
    for key in KEYS:
        if key[0] == "structural":
            seen |= pc.relations(pc.case(*key).pairs, key[1], key[2])
    assert seen >= {"a=0", "a>0", "b=N-1", "same block", "adjacent blocks", "b on a block's last node",
                    "a on a block's last node", "b in the partial last block", "whole block inside a ramp",
                    "whole block in a tail", "more than 2 x 256 explicit nodes",
                    "three consecutive edges out of one node", "inactive edges interleaved"}
    for kind, N, shift in KEYS:
        if kind == "structural" and shift >= 9:
            assert "more than 2 x 256 explicit nodes" in pc.relations(pc.case(kind, N, shift).pairs, N, shift)


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] == "islands"],
                         ids=[i for i, k in zip(IDS, KEYS) if k[0] == "islands"])
def test_islands_leave_nodes_uncovered(key):
    _, N, shift = key
    bs = 1 << shift
    c = pc.case(*key)
    cov = pc.covered(c.pairs, N)
    assert c.first_a() == 10 and not cov[:11].any()                   # nodes 0..10
    assert cov[11:41].all()
    assert not cov[N - 3:].any() and max(b for _, b in c.active) <= N - 4
    inside = [(10, 40), (bs + 5, 3 * bs - 7), (4 * bs, 5 * bs - 1)]
    assert all(any(lo <= a and b <= hi for lo, hi in inside) for a, b in c.active)
    assert not cov[41:min(bs + 6, N)].any()                           # the gap before the second island
    assert (np.diff(cov.astype(int)) == 1).sum() >= 2                 # at least two separate covered runs
    # uncovered nodes have M = 0: the oracle leaves their 1 / M out of every ramp
    assert any(not pc.is_active(a, b) for a, b in c.pairs)


@pytest.mark.parametrize("E", pc.DENSE_E)
def test_dense_graph(E):
    c = pc.dense_case(E)
    assert len(c.pairs) == E == len(set(c.pairs))
    adjacent = sum(abs(a - b) == 1 for a, b in c.pairs)
    reverse = sum(a > b + 1 for a, b in c.pairs)
    tol = 3 * np.sqrt(0.1 * 0.9 / E) + 1 / E        # three sigma of the larger share
    assert abs(adjacent / E - 0.05) <= tol and abs(reverse / E - 0.10) <= tol
    assert adjacent > 0 and reverse > 0 and len(c.active) == E - adjacent - reverse
    _check_steps(c, both_clamp_outcomes=True)
    # the inactive edges change nothing: the oracle on the active-only sub-list
    # (same order) gives the same bits, so the GPU may be held to that too
    keep = np.array([pc.is_active(a, b) for a, b in c.pairs])
    for lr in pc.LRS:
        sub = po.sgd_step(c.poses.copy(), c.ea[keep], c.eb[keep], c.tf[keep], lr, pc.SIGMA)
        assert np.array_equal(sub, c.ref[lr])


def test_dense_edge_counts_cross_the_compaction_boundaries():
    """sgd_compact_kernel: 64-lane ballots, 1,024 edges per round."""
    for edge in (64, 1024, 2048):
        assert any(e < edge for e in pc.DENSE_E) and any(e > edge for e in pc.DENSE_E)
    assert 64 in pc.DENSE_E and 1024 in pc.DENSE_E


def test_inactive_graph():
    c = pc.inactive_case()
    assert c.active == [] and len(c.pairs) >= 4
    for lr in pc.LRS:
        assert np.array_equal(c.ref[lr], c.poses)


def _plan(lib, N):
    v = [ctypes.c_int32() for _ in range(4)]
    assert lib.slam_pgo_sgd_plan(N, *[ctypes.byref(x) for x in v]) == 0
    return dict(zip(("in_lds", "rounds", "shift", "threads"), (x.value for x in v)))


def test_plan_flips_exactly_at_the_boundaries():
    from slamhip import _abi, pgo
    lib = _abi.lib()
    for N, fields in pc.PLAN_BOUNDARIES.items():
        lo, hi = _plan(lib, N), _plan(lib, N + 1)
        assert {k for k in lo if lo[k] != hi[k]} == fields, (N, lo, hi)
    # nowhere else: between two boundaries the plan is constant
    edges = [0] + sorted(pc.PLAN_BOUNDARIES) + [524290]
    for lo, hi in zip(edges, edges[1:]):
        ref = _plan(lib, lo + 1)
        for N in {lo + 2, (lo + hi) // 2, hi - 1, hi} - {lo}:
            assert _plan(lib, N) == ref, N
    for N, (in_lds, rounds, shift) in pc.AUTO_PLAN.items():
        p = pgo.sgd_plan(N)
        assert (p["in_lds"], p["rounds"], p["shift"]) == (in_lds, rounds, shift), N
        assert p["threads"] == (64 if in_lds else 256)
    # every case sits on the side of its boundary it is named for
    for N in pc.PLAN_BOUNDARIES:
        if N + 1 in pc.AUTO_PLAN:
            assert N + 1 in pc.AUTO_STRUCTURAL
    assert {4096, 4097, 6144, 6145, 131072, 131073} <= set(pc.AUTO_STRUCTURAL)


def test_forced_plans_hold_their_graphs():
    from slamhip import pgo
    try:
        for path, sh, N in pc.FORCED:
            pgo.force_sgd_path(path, sh)
            p = pgo.sgd_plan(N)
            assert p["in_lds"] == (path < 2) and p["rounds"] == (2 if path == 1 else 1)
            assert p["shift"] == (6 if sh < 0 else sh)
            if p["shift"] >= 9:      # the overflow loop: 2^(sh+1) > kRelaxSlots * 256 explicit-node slots
                assert 2 << p["shift"] > 2 * p["threads"] and N > 2 << p["shift"]
    finally:
        pgo.force_sgd_path()


@pytest.mark.parametrize("N", pc.ORIENT_N)
def test_orient_inputs(N):
    p = pc.orient_case(N)
    assert p.shape == (N, 3)
    runs = pc.zero_runs(N)
    assert len(runs) == (2 if N >= 259 else 1 if N >= 4 else 0)
    for lo, hi in runs:
        assert np.all(p[lo:hi + 1, :2] == p[lo, :2])
    ref = po.orient_from_positions(p.copy())
    zero = np.zeros(N, dtype=bool)
    for lo, hi in runs:
        zero[lo:hi] = True               # node i's step i -> i + 1 has length 0
    inner = np.zeros(N, dtype=bool)
    inner[1:max(N - 1, 1)] = True
    keep = zero | ~inner
    assert np.array_equal(ref[keep, 2], p[keep, 2])                   # zero steps and both ends keep their heading
    assert np.all(np.abs(po.wrap(ref[~keep, 2] - p[~keep, 2])) > 1e-3)    # every other heading really changes
    assert np.array_equal(ref[:, :2], p[:, :2])


@pytest.mark.parametrize("N", pc.ORIENT_TF_N)
def test_orient_tf_inputs(N):
    p, tfs = pc.orient_tf_case(N)
    assert tfs.shape == (max(N - 1, 0), 3, 3)
    ref = pc.orient_from_tf_ref(p.copy(), tfs)
    # the reference's own loop (recompute_orientation with a stand-in ICP) on
    # coincident positions, where its first half changes nothing
    q = p.copy()
    q[:, :2] = 0.0
    it = iter(tfs)
    got = po.recompute_orientation(q, [np.zeros((1, 2))] * N, 1, 0.1, icp_recompute=True,
                                   icp_fn=lambda *a: ([next(it)], 0.0))
    assert np.array_equal(got[:, 2], ref[:, 2])
    # node i >= 2 reading the NEW theta_{i-1} instead of the old one is off by
    # new - old of node i - 1: more than 0.1 rad for every node that is updated
    assert np.all(np.abs(ref[1:N - 1, 2] - p[1:N - 1, 2]) > 0.1)
    assert ref[0, 2] == p[0, 2] and np.array_equal(ref[:, :2], p[:, :2])
