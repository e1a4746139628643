"""CPU checks of tests/pcm_cases.py: every input sits where its docstring says
(indices, slots, words, on-bound counts), and ``select_packed`` and the closed
forms of the cluster inputs equal the restatement tests/pcm_ref.py at small L.
tests/test_pcm_paths_gpu.py runs the same cases on the GPU."""
import numpy as np
import pytest

import pcm_cases as pc
import pcm_ref


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _seeded_graph(L, seed):
    """Named seeded fill: every pair is an edge with probability 0.6, a clique on the first third."""
    rng = np.random.default_rng(seed)
    full = np.triu(rng.random((L, L)) < 0.6, 1)
    full[:L // 3, :L // 3] = np.triu(np.ones((L // 3, L // 3), dtype=bool), 1)
    full = full | full.T
    return full


@pytest.mark.parametrize("L", [1, 2, 33, 70, 300])
def test_select_packed_is_the_restatement(L):
    for seed in (0, 1):
        full = _seeded_graph(L, 10 * L + seed)
        adj, deg = pcm_ref.pack(full), full.sum(1).astype(np.int32)
        assert np.array_equal(pc.pack_rows(full), adj) and np.array_equal(pc.popcounts(adj), deg)
        assert all(np.array_equal(pc.unpack_row(adj[l], L), full[l]) for l in range(0, L, 7))
        for min_size in (0, 1, 2, 5):
            got = pc.select_packed(adj, deg, min_size)
            assert got[0].dtype == np.int32 and got[1].dtype == np.uint8
            assert _same(got, pcm_ref.select(adj, deg, min_size)), (L, seed, min_size)
        if L >= 33:
            assert 0 < got[2] < L - 1
    # a patched row is used in place of the stored one
    if L == 70:
        r = int(np.argmin(pc.select_packed(adj, deg)[0] != 0))
        zero = np.zeros_like(adj[r])
        changed = adj.copy()
        changed[r] = zero
        assert _same(pc.select_packed(adj, deg, 2, patch={r: zero}), pcm_ref.select(changed, deg, 2))


@pytest.mark.parametrize("G", pc.A_GS)
@pytest.mark.parametrize("L", [L for L in pc.A_LS if L <= 513])
def test_cluster_closed_forms_are_the_restatement(L, G):
    g = pc.cluster_ids(L, G)
    X, a, b, Z = pc.cluster_inputs(g)
    adj, deg = pcm_ref.adjacency(X, a, b, Z, pc.CLUSTER_TOL)
    cadj, cdeg = pc.cluster_adjacency(g)
    assert cadj.dtype == np.uint32 and np.array_equal(cadj, adj) and np.array_equal(cdeg, deg)
    assert np.array_equal(pc.cluster_adjacency(g, rows=[0, L - 1])[0], adj[[0, L - 1]])
    for min_size in (1, 2, L):
        assert _same(pc.cluster_peel(g, min_size), pcm_ref.select(adj, deg, min_size)), (L, G, min_size)
    order, keep, steps = pc.cluster_peel(g, 1)
    assert steps == L - np.bincount(g).max() and keep.sum() == np.bincount(g).max()
    if G == "1":
        assert steps == 0 and keep.all()
    if G == "L":
        assert steps == L - 1 and keep[0] == 1 and np.array_equal(order, np.r_[-1, np.arange(L - 2, -1, -1)])


@pytest.mark.parametrize("G", pc.A_GS)
@pytest.mark.parametrize("L", [L for L in pc.A_LS if L > 513])
def test_cluster_closed_forms_against_select_packed(L, G):
    """Above what the L x L restatement does quickly: the packed peel on the closed-form rows."""
    g = pc.cluster_ids(L, G)
    adj, deg = pc.cluster_adjacency(g)
    assert np.array_equal(pc.popcounts(adj), deg)
    assert _same(pc.cluster_peel(g), pc.select_packed(adj, deg))


@pytest.mark.parametrize("G", ["3", "5"])
def test_clusters_are_spread(G):
    """Every cluster has members in every word (a lane half of a pair-kernel wave) and in every peel slot of
    every peel wave."""
    L = 4096
    g = pc.cluster_ids(L, G)
    i = np.arange(L)
    sizes = np.bincount(g)
    assert len(sizes) == int(G) and sizes.min() > L // int(G) - 64
    for c in range(int(G)):
        mine = i[g == c]
        assert len(np.unique(mine >> 5)) == pc.words(L)
        assert len(np.unique((mine >> 10) * 16 + ((mine & 1023) >> 6))) == 4 * 16


def test_capacity_clusters():
    g = pc.capacity_clusters()
    assert len(g) == pc.MAX_L and np.bincount(g).tolist() == [pc.MAX_L - 201, 100, 101]
    for c in (1, 2):
        mine = np.flatnonzero(g == c)
        assert len(np.unique(mine >> 10)) >= 59 and len(np.unique((mine & 1023) >> 6)) == 16
        assert len(np.unique(mine & 32)) == 2
    order, keep, steps = pc.cluster_peel(g)
    assert steps == 201 and keep.sum() == pc.MAX_L - 201
    assert order[17 + 653 * 99] == 0 and order[17] == 99 and order[301 + 601 * 100] == 100 and order[301] == 200
    adj, deg = pc.cluster_adjacency(g, rows=pc.CAP_ROWS)
    assert adj.shape == (len(pc.CAP_ROWS), 2048) and g[pc.CAP_ROWS[-2]] == 1 and g[pc.CAP_ROWS[-1]] == 2
    assert np.array_equal(pc.popcounts(adj), deg[list(pc.CAP_ROWS)])
    assert deg[0] == pc.MAX_L - 202 and deg[17] == 99 and deg[301] == 100
    # the key of closure 65,535 has index field 0 and it is in the big cluster
    assert g[65535] == 0


@pytest.mark.parametrize("name", list(pc.B_ANCHORS))
def test_bounds_are_on_the_bit(name):
    c = pc.bound_case(name)
    L, A = c.L, c.anchor
    probes = np.delete(np.arange(L), A)
    tt0, ttd, tr0, trd = (np.float64(v) for v in c.tol)
    bt = tt0 * tt0 + (ttd * ttd) * c.n.astype(np.float64)
    br = tr0 * tr0 + (trd * trd) * c.n.astype(np.float64)
    up = np.nextafter(bt, np.inf), np.nextafter(br, np.inf)
    # the restatement's own terms for the pairs with the anchor are the stated ones
    dt, dr, n = pcm_ref.pair_terms(c.X, c.a, c.b, c.Z)
    for i in probes:
        lo, hi = min(i, A), max(i, A)
        assert n[lo, hi] == c.n[i] == abs(c.a[i] - c.a[A]) + abs(c.b[i] - c.b[A])
        assert dt[lo, hi] == c.dt[i] == (bt[i] if c.t_on[i] else up[0][i])
        assert dr[lo, hi] == c.dr[i] == (br[i] if c.r_on[i] else up[1][i])
    full = pcm_ref.consistent(c.X, c.a, c.b, c.Z, c.tol)
    assert np.array_equal(full[A, probes], c.t_on[probes] & c.r_on[probes])
    assert np.array_equal(full[probes, A], full[A, probes])
    # at least 10 of each, the four combinations, n = 0, and every sign pattern
    for on in (c.t_on[probes], c.r_on[probes]):
        assert on.sum() >= 10 and (~on).sum() >= 10
    combos = {(bool(t), bool(r)) for t, r in zip(c.t_on[probes], c.r_on[probes])}
    assert len(combos) == 4
    zero = probes[c.n[probes] == 0]
    assert len(zero) >= 8 and c.r_on[zero].any() and not c.r_on[zero].all()
    if A > 0:   # as the low index dt = x x, and x = trans_tol is on the bound; x x + (d x)(d x) need not reach it
        assert c.t_on[zero[zero < A]].any()
    da, db = c.a[probes] - pc.B_CENTRE, c.b[probes] - pc.B_CENTRE
    for sa in (-1, 0, 1):
        for sb in (-1, 0, 1):
            sel = (np.sign(da) == sa) & (np.sign(db) == sb)
            assert sel.sum() >= 4, (sa, sb)
            if sa or sb:   # each sign pattern is seen with the pair consistent and not
                assert full[A, probes[sel]].any() and not full[A, probes[sel]].all()
    # |da| + |db| differs from |da + db| on a consistent pair: the wrong sum would change its bit's bound
    assert ((np.sign(da) * np.sign(db) == -1) & full[A, probes]).any()
    # the four combinations in lanes 0, 31, 32 and 63 of some wave, and on either side of column and row 256
    for lane in (0, 31, 32, 63):
        at = probes[(probes & 63) == lane]
        assert len({(bool(c.t_on[i]), bool(c.r_on[i])) for i in at}) == 4, lane
    for side in (probes[probes < 256], probes[probes >= 256]):
        assert len({(bool(c.t_on[i]), bool(c.r_on[i])) for i in side}) == 4
    assert pc.words(L) % 2 == 1


def test_anchor_is_low_and_high():
    """With the anchor first every probe is the high index of its pair, with the anchor last the low one, and
    in the middle both occur: the same rule is evaluated from both sides."""
    first, mid, last = (pc.bound_case(n) for n in pc.B_ANCHORS)
    assert (first.anchor, mid.anchor, last.anchor) == (0, 259, pc.B_L - 1)
    # as the high index the probe's translation carries the (d x)^2 term, as the low index it does not
    assert (first.dt[1:] > first.Z[1:, 2] ** 2).sum() > 400
    assert np.array_equal(last.dt[:-1], last.Z[:-1, 2] ** 2)
    assert np.array_equal(mid.dt[:259], mid.Z[:259, 2] ** 2) and (mid.dt[260:] > mid.Z[260:, 2] ** 2).sum() > 200


@pytest.mark.parametrize("K,L", pc.SLOT_SHAPES, ids=[pc.slot_name(*s) for s in pc.SLOT_SHAPES])
def test_slot_graphs(K, L):
    gr = pc.slot_graph(K, L)
    S = K + 2
    st = gr.stragglers
    assert pc.auto_slots(L) == K and gr.W == pc.words(L)
    # where the stragglers sit: s_k in slot k, varying waves, both lane halves, ascending after p
    s = st[1:-1]
    assert np.array_equal(s >> 10, np.arange(K)) and st[-1] == L - 2 and (st[-1] >> 10) == K - 1
    if K >= 4:
        assert len(np.unique((s & 1023) >> 6)) >= 4 and len(np.unique(s & 32)) == 2
    if L % pc.PEEL:   # an odd W whose last word is the `lo` word of wave 5 in slot K - 1, with no `hi` word behind it
        assert gr.W % 2 == 1 and gr.W - 1 == 2 * 5 + 32 * (K - 1) and ((L - 1) & 1023) >> 6 == 5
    # symmetric, degrees are the popcounts, padding clear, diagonal clear
    assert np.array_equal(pc.popcounts(gr.adj), gr.deg)
    idx = np.arange(L)
    assert not ((gr.adj[idx, idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).any()
    if L % 32:
        assert not (gr.adj[:, -1] >> np.uint32(L % 32)).any()
    for j, sj in enumerate(st):
        row = pc.unpack_row(gr.adj[sj], L)
        col = ((gr.adj[:, sj >> 5] >> np.uint32(sj & 31)) & 1).astype(bool)
        assert np.array_equal(row, col) and np.array_equal(row, gr.bits[j])
        assert gr.deg[sj] == S - 1 + gr.n0 + j                      # distinct, ascending with the position
        assert row[st].sum() == S - 1                               # all the other stragglers
        nb = np.flatnonzero(row)
        assert len(np.unique(nb >> 10)) == K                        # neighbours in every slot
        assert row[L - 1] and (nb >> 5 == gr.W - 1).any()           # index L - 1, word W - 1
        assert (sj ^ 32) >= L or (sj ^ 32) in st or row[sj ^ 32]    # the same wave's other lane half
    clique = np.setdiff1d(idx, st)
    assert gr.deg[clique].min() >= L - S - 1 > gr.deg[st].max() + 1
    # the peel: position by position, by hand and by the packed reference
    want = pc.select_packed(gr.adj, gr.deg)
    assert _same(want, gr.want) and want[2] == S and want[1].sum() == L - S == gr.kept
    assert np.array_equal(want[0][st], np.arange(S))
    # a decrement lost in any slot swaps that slot's straggler with its successor
    slots = range(K) if K <= 16 else (0, 1, 16, 17, 31, 32, 33, 62, 63)
    for k in slots:
        got = pc.dropped_decrement(gr, k)
        swapped = np.arange(S)
        swapped[[k + 1, k + 2]] = [k + 2, k + 1]
        assert np.array_equal(got[0][st], swapped), (K, L, k)


def test_slot_graph_small_against_the_restatement():
    gr = pc.slot_graph(1, 337)
    assert _same(pcm_ref.select(gr.adj, gr.deg), gr.want)
    gr = pc.slot_graph(4, 3409)
    assert _same(pcm_ref.select(gr.adj, gr.deg), gr.want)


@pytest.mark.parametrize("case", pc.hand_graphs(), ids=[c.name for c in pc.hand_graphs()])
def test_hand_graphs(case):
    assert np.array_equal(pc.popcounts(case.adj), case.deg) and len(case.deg) == case.L
    assert _same(pc.select_packed(case.adj, case.deg, case.min_size), case.want), case.name
    if case.L <= 100:
        assert _same(pcm_ref.select(case.adj, case.deg, case.min_size), case.want), case.name
        full = pcm_ref.unpack(case.adj, case.L)
        assert np.array_equal(full, full.T) and not full.diagonal().any()


def test_tie_graph_positions():
    out = np.array(pc.TIE_OUT)
    assert pc.auto_slots(pc.TIE_L) == 4
    assert (out >> 10).tolist() == [0, 0, 1, 1, 2, 2] and ((out & 1023) >> 6).tolist() == [0, 1, 0, 1, 0, 1]
    assert (out & 1023).tolist() == [5, 70, 5, 76, 2, 64]
    case = pc.hand_graphs()[0]
    assert case.name == "ties-across-slots" and (case.deg[out] == 0).all() and case.want[0][2112] == 0


@pytest.mark.parametrize("case", pc.nonfinite_cases(), ids=[c.name for c in pc.nonfinite_cases()])
def test_nonfinite_bits(case):
    with np.errstate(all="ignore"):
        full = pcm_ref.consistent(case.X, case.a, case.b, case.Z, case.tol)
        adj, deg = pcm_ref.adjacency(case.X, case.a, case.b, case.Z, case.tol)
    assert np.array_equal(full, case.full), (case.name, np.argwhere(full != case.full))
    assert np.array_equal(adj, pc.pack_rows(case.full)) and np.array_equal(deg, case.full.sum(1))
    # the peel follows from those bits: whoever has no consistent partner goes first, from the highest index down
    order, keep, steps = pc.select_packed(adj, deg, 2)
    alone = np.flatnonzero(deg == 0)
    if len(alone) < case.L:
        assert np.array_equal(order[alone[::-1]], np.arange(len(alone))) and not keep[alone].any()
        assert keep.sum() == case.L - len(alone) - (order[deg > 0] >= 0).sum()
