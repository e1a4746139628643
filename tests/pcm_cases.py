"""Hand-placed inputs for the pairwise-consistency check (no GPU; nothing random).

csrc/pcm_kernels.hip writes a bit matrix with one wave per 64 columns and one
workgroup per 256 x 256 tile, and peels it in one workgroup of 1,024 threads,
thread t owning the closures t + 1024 k, k < K, K = 1, 4, 16 or 64 (slot k).  A
removed row reaches slot k of wave w through words 2 w + 32 k (lanes 0-31) and
2 w + 32 k + 1 (lanes 32-63), loaded by lane k.  The cases here put inputs on
those positions by hand and come with references that do not go through an
L x L array of bools:

* ``select_packed``: the peel on packed rows, unpacking the removed row only;
* group A, clusters: identity poses, closure i the pure translation Z = (1, 0,
  10 g(i), 0) with a = b = 0 and the tolerances ``CLUSTER_TOL``: every product is
  exact and two closures are consistent iff g agrees.  g(i) = (i * 7 + (i >> 6))
  % G for G = 1, 3, 5, which puts every cluster into every word, wave, lane half
  and peel slot (the sizes are left as they fall: equal sizes occur and the
  closed form says who goes first); g(i) = i for "G = L".  Closed forms
  ``cluster_adjacency`` / ``cluster_peel``; ``capacity_clusters`` is the L =
  65,536 instance, two clusters of 100 and 101 spread over all 64 slots;
* group B, ``bound_case``: an anchor closure (identity) at index 0, 259 or L - 1
  of L = 520 and 519 probes Z = (1, d, -x, 0) over identity poses.  With the probe
  as the low index E = (1, d, -x, 0), dt = x x and dr = d d exactly; with the
  probe as the high index E = (1, -d, x, -d x), dr = d d and dt = x x + (d x)(d
  x).  d and x are taken among the doubles next to the square roots so that dr
  and dt equal the bound to the last bit or are the next double above it, in
  all four combinations, for chain lengths n = |da| + |db| of either sign;
* group C, ``slot_graph``: a clique and K + 2 stragglers, one in every peel slot
  plus one that goes first and one that goes last, whose removal order changes
  when any one decrement between them is lost;
* group D, ``hand_graphs``: small graphs with the expected order written out;
* group G, ``nonfinite_cases``: NaN and infinities in poses, overflowing
  translations and an infinite tolerance, with the expected bits written out.

Every array is read-only and every case is built once per process.
tests/test_pcm_cases.py checks these inputs on the CPU;
tests/test_pcm_paths_gpu.py runs them on the GPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

from test_pcm import TOL

PEEL = 1024            # kPcmPeelBlock
TILE = 256             # kPcmBlock, kPcmRows
MAX_L = 65536          # kPcmMaxL
CLUSTER_TOL = (0.05, 0.0, 0.01, 0.0)   # trans_tol, trans_drift, rot_tol, rot_drift
A_LS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3409, 4096, 4097)
A_GS = ("1", "3", "5", "L")
IDENTITY = (1.0, 0.0, 0.0, 0.0)


def _ro(a):
    a.setflags(write=False)
    return a


def words(L):
    return (L + 31) // 32


def auto_slots(L):
    """K of the pcm_peel_kernel<K> that slam_pcm_select launches for L."""
    K = 1
    while K * PEEL < L:
        K *= 4
    return K


def pack_rows(bits):
    """uint32[R][W] of bool[R][L]: bit m of a row is bit m & 31 of word m >> 5."""
    bits = np.asarray(bits, dtype=bool)
    R, L = bits.shape
    pad = np.zeros((R, words(L) * 32), dtype=np.uint8)
    pad[:, :L] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view("<u4").astype(np.uint32)


def unpack_row(row, L):
    """bool[L] of one packed row."""
    return np.unpackbits(np.ascontiguousarray(row, dtype="<u4").view(np.uint8), bitorder="little")[:L].astype(bool)


_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def popcounts(adj):
    """int32[L]: the set bits of every packed row."""
    adj = np.ascontiguousarray(adj, dtype=np.uint32)
    out = np.empty(len(adj), dtype=np.int32)
    for r0 in range(0, len(adj), 4096):
        out[r0:r0 + 4096] = _POP8[adj[r0:r0 + 4096].view(np.uint8)].sum(1)
    return out


# ------------------------------------------------------------------ the peel on packed rows

def select_packed(adj, deg, min_size=2, patch=None):
    """``(order int32[L], keep uint8[L], steps)`` of packed rows and their
    degrees: lowest degree, then highest index, until the lowest degree touches
    everyone alive.  Only the removed row is unpacked.  ``patch`` maps a row
    index to words used in place of that row."""
    L = len(deg)
    d = np.array(deg, dtype=np.int64)
    big = np.int64(1) << 40
    alive = np.ones(L, dtype=bool)
    order = np.full(L, -1, np.int32)
    n_alive, steps = L, 0
    while n_alive > 1:
        masked = np.where(alive, d, big)
        low = masked.min()
        r = int(np.flatnonzero(masked == low)[-1])
        if low == n_alive - 1:
            break
        alive[r] = False
        order[r] = steps
        row = adj[r] if patch is None or r not in patch else patch[r]
        d[unpack_row(row, L) & alive] -= 1
        n_alive -= 1
        steps += 1
    keep = alive if n_alive >= min_size else np.zeros(L, dtype=bool)
    return order, keep.astype(np.uint8), steps


# ------------------------------------------------------------------ group A: clusters

def cluster_ids(L, G):
    """int64[L]: the cluster of every closure; ``G`` is 1, 3, 5 or "L"."""
    i = np.arange(L, dtype=np.int64)
    if G == "L":
        return _ro(i)
    return _ro((i * 7 + (i >> 6)) % int(G))


def cluster_inputs(g):
    """``(X float64[1][4], a, b, Z float64[L][4])`` of cluster ids g."""
    L = len(g)
    Z = np.tile(np.array(IDENTITY), (L, 1))
    Z[:, 2] = 10.0 * np.asarray(g, dtype=np.float64)
    zero = np.zeros(L, dtype=np.int64)
    return _ro(np.array([IDENTITY])), _ro(zero), _ro(zero.copy()), _ro(Z)


def cluster_adjacency(g, rows=None):
    """``(adj uint32[R][W], deg int32[L])``: row l is the mask of l's cluster
    without l, its degree the cluster's size minus 1.  ``rows``: those rows only."""
    g = np.asarray(g)
    L = len(g)
    ids, inverse, counts = np.unique(g, return_inverse=True, return_counts=True)
    masks = pack_rows(g[None, :] == ids[:, None])
    rows = np.arange(L) if rows is None else np.asarray(rows)
    adj = masks[inverse[rows]]
    adj[np.arange(len(rows)), rows >> 5] &= ~(np.uint32(1) << (rows & 31).astype(np.uint32))
    return adj, (counts[inverse] - 1).astype(np.int32)


def cluster_peel(g, min_size=2):
    """``(order, keep, steps)``: the clusters are emptied in ascending size, each
    from its highest index down; of equal sizes the one holding the highest
    index goes first; the last one in that order stays.  steps = L - its size."""
    g = np.asarray(g)
    L = len(g)
    members = [np.flatnonzero(g == c) for c in np.unique(g)]
    members.sort(key=lambda m: (len(m), -int(m[-1])))
    order = np.full(L, -1, np.int32)
    steps = 0
    for m in members[:-1]:
        order[m[::-1]] = steps + np.arange(len(m), dtype=np.int32)
        steps += len(m)
    keep = np.zeros(L, dtype=np.uint8)
    if len(members[-1]) >= min_size:
        keep[members[-1]] = 1
    return order, keep, steps


CAP_ROWS = (0, 31, 32, 255, 256, 32767, 32768, 65280, 65535, 17 + 653 * 40, 301 + 601 * 77)


@functools.lru_cache(maxsize=None)
def capacity_clusters():
    """g at L = 65,536: cluster 1 = {17 + 653 k, k < 100}, cluster 2 = {301 + 601
    k, k < 101}, everyone else cluster 0.  Both small clusters have members in
    many peel slots (index >> 10) and waves; 201 steps."""
    g = np.zeros(MAX_L, dtype=np.int64)
    c1, c2 = 17 + 653 * np.arange(100), 301 + 601 * np.arange(101)
    assert not np.intersect1d(c1, c2).size and max(c1[-1], c2[-1]) < MAX_L
    g[c1], g[c2] = 1, 2
    return _ro(g)


# ------------------------------------------------------------------ group B: bounds on the bit

B_L = 520
B_ANCHORS = {"anchor-first": 0, "anchor-middle": 259, "anchor-last": B_L - 1}
B_CENTRE = 200         # the anchor's a and b in a chain of 401 identity poses


def _scan(f, guess, target, span=24):
    """The first double v within ``span`` doubles of ``guess`` with f(v) == target, or None."""
    v = np.float64(guess)
    for _ in range(span):
        v = np.nextafter(v, 0.0)
    for _ in range(2 * span + 1):
        if f(v) == target:
            return v
        v = np.nextafter(v, np.inf)
    return None


def _chain_offsets(n, pattern):
    """(da, db) with |da| + |db| = n: da alone, db alone, both, each with either sign."""
    j = max(1, n // 3) if n else 0
    return [(n, 0), (-n, 0), (0, n), (0, -n), (j, n - j), (-j, n - j), (j, j - n), (-j, j - n)][pattern]


@functools.lru_cache(maxsize=None)
def bound_case(name):
    """The case with the anchor where ``name`` says.  Probe i (every other index)
    is meant to sit on the translation bound (``t_on[i]``) or one ulp above it,
    and on the rotation bound (``r_on[i]``) or one ulp above it, the combination
    (i + (i >> 6)) & 3, the sign pattern (i >> 2) & 7, at chain length ``n[i]``.
    Bit (anchor, i) is t_on[i] & r_on[i].  Probes 0-15 try n = 0 first."""
    L, anchor = B_L, B_ANCHORS[name]
    tt0, ttd, tr0, trd = (np.float64(v) for v in TOL)
    X = np.tile(np.array(IDENTITY), (2 * B_CENTRE + 1, 1))
    a = np.full(L, B_CENTRE, dtype=np.int64)
    b = np.full(L, B_CENTRE, dtype=np.int64)
    Z = np.tile(np.array(IDENTITY), (L, 1))
    t_on, r_on, ns = np.zeros(L, bool), np.zeros(L, bool), np.zeros(L, np.int64)
    dt, dr = np.zeros(L), np.zeros(L)
    for i in range(L):
        if i == anchor:
            continue
        combo = (i + (i >> 6)) & 3
        want_t, want_r = bool(combo & 1), bool(combo & 2)
        start = 0 if i < 16 else (i * 3) % (B_CENTRE + 1)
        for n in [(start + k) % (B_CENTRE + 1) for k in range(B_CENTRE + 1)]:
            bt = tt0 * tt0 + (ttd * ttd) * np.float64(n)
            br = tr0 * tr0 + (trd * trd) * np.float64(n)
            d = _scan(lambda v: v * v, np.sqrt(br), br if want_r else np.nextafter(br, np.inf))
            if d is None:
                continue
            if i < anchor:   # the probe is the low index: E = (1, d, -x, 0)
                def f(v):
                    return v * v
                guess = np.sqrt(bt)
            else:            # the probe is the high index: E = (1, -d, x, -d x)
                def f(v, d=d):
                    return v * v + (d * v) * (d * v)
                guess = np.sqrt(bt / (1 + d * d))
            x = _scan(f, guess, bt if want_t else np.nextafter(bt, np.inf))
            if x is None:
                continue
            da, db = _chain_offsets(n, (i >> 2) & 7)
            a[i], b[i] = B_CENTRE + da, B_CENTRE + db
            Z[i, 1], Z[i, 2] = d, -x
            t_on[i], r_on[i], ns[i], dt[i], dr[i] = want_t, want_r, n, f(x), d * d
            break
        else:
            raise AssertionError(f"no probe found for index {i}")
    return SimpleNamespace(name=name, L=L, anchor=anchor, X=_ro(X), a=_ro(a), b=_ro(b), Z=_ro(Z), tol=TOL,
                           t_on=_ro(t_on), r_on=_ro(r_on), n=_ro(ns), dt=_ro(dt), dr=_ro(dr))


# ------------------------------------------------------------------ group C: every peel slot

# (K, L): every slot full, and an odd W whose last word is the `lo` word of wave 5 in the last slot.  K = 64 is
# the automatic choice from L = 16,385; slots 17-63 hold closures from L = 17,409 and all of them from 64,513.
SLOT_SHAPES = ((1, 1024), (1, 337), (4, 4096), (4, 3409), (16, 16384), (16, 15697), (64, 65536), (64, 64849))


def slot_name(K, L):
    return f"K{K}-L{L}"


def _straggler_neighbour(i, j):
    """Whether clique member i is a neighbour of the straggler at position j before the counts are trimmed: 3 in
    11, different from word to word and from slot to slot."""
    return (i * (2 * j + 3) + (i >> 5) * 5 + (i >> 10)) % 11 < 3


@functools.lru_cache(maxsize=None)
def slot_graph(K, L):
    """A clique of all but K + 2 stragglers.  Straggler s_k sits in slot k at 1024
    k + t_k, t_k = 64 ((5 k + 3) % 16) + (37 k + 9) % 64 (reduced into the last
    slot where that one is short): the waves and lane halves vary with k.  p =
    1024 (K / 2) + 100 goes first and q = L - 2 goes last.  All stragglers are
    neighbours of each other, and the one at position j of (p, s_0, ..., s_{K-1},
    q) has n0 + j neighbours in the clique: at its turn it has degree K + 1 + n0
    and its successor, which has the higher index, one more.  If s_k misses the
    decrement of its predecessor's removal, it ties with its successor and the
    successor goes first.  Every straggler's clique neighbours include index ^ 32
    (the same wave's other lane half), L - 1 (word W - 1) and members of every
    other slot.  steps = K + 2; the clique of L - K - 2 is kept."""
    assert auto_slots(L) == K and L - PEEL * (K - 1) >= 3
    s = [PEEL * k + (64 * ((5 * k + 3) % 16) + (37 * k + 9) % 64) % min(PEEL, L - PEEL * k - 2) for k in range(K)]
    strag = np.array([PEEL * (K // 2) + 100] + s + [L - 2], dtype=np.int64)
    S = len(strag)
    assert len(set(strag.tolist())) == S and strag.max() < L - 1 and (np.diff(strag[1:]) > 0).all()
    is_clique = np.ones(L, dtype=bool)
    is_clique[strag] = False
    idx = np.arange(L, dtype=np.int64)
    bits = np.zeros((S, L), dtype=bool)
    must = []
    for j, sj in enumerate(strag):
        bits[j] = _straggler_neighbour(idx, j) & is_clique
        m = [v for v in (int(sj) ^ 32, L - 1) if v < L and is_clique[v]]
        bits[j, m] = True
        must.append(m)
    n0 = int(bits.sum(1).min()) - S
    for j in range(S):
        cand = np.setdiff1d(np.flatnonzero(bits[j]), must[j])
        extra = int(bits[j].sum()) - (n0 + j)
        bits[j, cand[::len(cand) // extra][:extra]] = False   # taken evenly over the whole row
        assert bits[j].sum() == n0 + j
    bits[:, strag] = ~np.eye(S, dtype=bool)
    W = words(L)
    adj = np.empty((L, W), dtype=np.uint32)
    adj[:] = pack_rows(np.ones((1, L), dtype=bool))
    one = np.uint32(1)
    for j, sj in enumerate(strag):
        adj[~bits[j], sj >> 5] &= ~(one << np.uint32(sj & 31))
    adj[strag] = pack_rows(bits)
    adj[idx, idx >> 5] &= ~(one << (idx & 31).astype(np.uint32))
    C = L - S
    deg = (C - 1 + bits.sum(0)).astype(np.int32)
    deg[strag] = bits.sum(1)
    order = np.full(L, -1, np.int32)
    order[strag] = np.arange(S)
    keep = is_clique.astype(np.uint8)
    return SimpleNamespace(name=slot_name(K, L), K=K, L=L, W=W, adj=_ro(adj), deg=_ro(deg), stragglers=_ro(strag),
                           bits=_ro(bits), n0=n0, want=(_ro(order), _ro(keep), S), kept=C)


def dropped_decrement(graph, k):
    """The peel of ``graph`` when the removal of s_k's predecessor does not reach s_k: ``select_packed`` with bit
    s_k of that one row cleared."""
    pred, sk = int(graph.stragglers[k]), int(graph.stragglers[k + 1])
    row = graph.adj[pred].copy()
    assert (row[sk >> 5] >> np.uint32(sk & 31)) & 1
    row[sk >> 5] &= ~(np.uint32(1) << np.uint32(sk & 31))
    return select_packed(graph.adj, graph.deg, 2, patch={pred: row})


# ------------------------------------------------------------------ group D: ties, the stop rule, min_size

def graph_of(L, pairs):
    """``(adj, deg)`` of undirected pairs."""
    full = np.zeros((L, L), dtype=bool)
    for l, m in pairs:
        assert l != m
        full[l, m] = full[m, l] = True
    return _ro(pack_rows(full)), _ro(full.sum(1).astype(np.int32))


def _clique(members):
    members = list(members)
    return [(l, m) for i, l in enumerate(members) for m in members[:i]]


def clique_without(L, out):
    """``(adj, deg)``: a clique of all of range(L) but ``out``, which are isolated.  Packed directly."""
    out = np.asarray(out, dtype=np.int64)
    adj = np.empty((L, words(L)), dtype=np.uint32)
    adj[:] = pack_rows(np.ones((1, L), dtype=bool))
    one = np.uint32(1)
    idx = np.arange(L)
    adj[idx, idx >> 5] &= ~(one << (idx & 31).astype(np.uint32))
    for o in out:
        adj[:, o >> 5] &= ~(one << np.uint32(o & 31))
    adj[out] = 0
    deg = np.full(L, L - len(out) - 1, dtype=np.int32)
    deg[out] = 0
    return _ro(adj), _ro(deg)


def _hand(name, L, pairs, min_size, order, keep, steps, graph=None):
    adj, deg = graph if graph is not None else graph_of(L, pairs)
    return SimpleNamespace(name=name, L=L, adj=adj, deg=deg, min_size=min_size,
                           want=(_ro(np.array(order, np.int32)), _ro(np.array(keep, np.uint8)), steps))


TIE_L = 2113
# threads 5, 70, 5, 76, 2, 64; waves 0, 1, 0, 1, 0, 1; slots 0, 0, 1, 1, 2, 2
TIE_OUT = (5, 70, 1029, 1100, 2050, 2112)


@functools.lru_cache(maxsize=None)
def hand_graphs():
    """Small graphs whose peel is written out by hand: ``want`` = (order, keep, steps)."""
    out = []
    # equal degrees (0) in different threads, waves and slots of K = 4: the highest index goes first
    order = np.full(TIE_L, -1)
    order[list(TIE_OUT)] = [5, 4, 3, 2, 1, 0]
    keep = np.ones(TIE_L, int)
    keep[list(TIE_OUT)] = 0
    out.append(_hand("ties-across-slots", TIE_L, None, 2, order, keep, 6, graph=clique_without(TIE_L, TIE_OUT)))
    # equal degrees (1) in one wave, lanes 0, 31, 32, 63 and the next wave: a perfect matching on 66 closures
    # goes from the top down, and the last pair is a clique of 2
    out.append(_hand("ties-in-a-wave", 66, [(2 * i, 2 * i + 1) for i in range(33)], 2,
                     [-1, -1] + list(range(63, -1, -1)), [1, 1] + [0] * 64, 64))
    # a clique only after s removals
    out.append(_hand("clique-after-1", 6, _clique(range(5)), 2, [-1] * 5 + [0], [1] * 5 + [0], 1))
    out.append(_hand("clique-after-2", 6, _clique(range(4)), 2, [-1] * 4 + [1, 0], [1] * 4 + [0, 0], 2))
    # a path 0 - 1 - 2 - 3 - 4 - 5: the end of the path ties with closure 0 at degree 1 and goes; {0, 1} after L - 2
    out.append(_hand("clique-after-L-2", 6, [(i, i + 1) for i in range(5)], 2, [-1, -1, 3, 2, 1, 0],
                     [1, 1, 0, 0, 0, 0], 4))
    # two disjoint cliques of equal size: the one holding the highest index is emptied
    out.append(_hand("equal-cliques-blocks", 8, _clique(range(4)) + _clique(range(4, 8)), 2,
                     [-1] * 4 + [3, 2, 1, 0], [1] * 4 + [0] * 4, 4))
    out.append(_hand("equal-cliques-interleaved", 8, _clique(range(0, 8, 2)) + _clique(range(1, 8, 2)), 2,
                     [-1, 3, -1, 2, -1, 1, -1, 0], [1, 0] * 4, 4))
    # the end of the loop: one alive; the break at two alive; a clique from the start
    out.append(_hand("ends-with-1-alive", 3, [], 1, [-1, 1, 0], [1, 0, 0], 2))
    out.append(_hand("ends-with-1-alive-min2", 3, [], 2, [-1, 1, 0], [0, 0, 0], 2))
    out.append(_hand("break-at-2-alive", 3, [(0, 1)], 2, [-1, -1, 0], [1, 1, 0], 1))
    out.append(_hand("clique-from-the-start", 4, _clique(range(4)), 2, [-1] * 4, [1] * 4, 0))
    # min_size around the kept size of 4
    for ms, kept in ((0, 1), (1, 1), (4, 1), (5, 0), (2 ** 31 - 1, 0)):
        out.append(_hand(f"min-size-{ms}", 6, _clique(range(4)), ms, [-1] * 4 + [1, 0], [kept] * 4 + [0, 0], 2))
    # min_size = 0 keeps the last one alive of an empty graph
    out.append(_hand("min-size-0-one-left", 3, [], 0, [-1, 1, 0], [1, 0, 0], 2))
    # L = 1 and L = 2
    out.append(_hand("L1", 1, [], 1, [-1], [1], 0))
    out.append(_hand("L1-min2", 1, [], 2, [-1], [0], 0))
    out.append(_hand("L2-connected", 2, [(0, 1)], 2, [-1, -1], [1, 1], 0))
    out.append(_hand("L2-apart", 2, [], 1, [-1, 0], [1, 0], 1))
    out.append(_hand("L2-apart-min2", 2, [], 2, [-1, 0], [0, 0], 1))
    return tuple(out)


# ------------------------------------------------------------------ group G: non-finite input

def _from_groups(L, groups):
    """bool[L][L]: consistent exactly within each group."""
    full = np.zeros((L, L), dtype=bool)
    for grp in groups:
        for l in grp:
            for m in grp:
                full[l, m] = l != m
    return full


@functools.lru_cache(maxsize=None)
def nonfinite_cases():
    """Seven closures each; 0-3 are the identity over identity poses and
    consistent with each other.  ``full`` is the expected bit matrix by hand:
    a comparison with NaN is false, inf <= finite is false, inf <= inf is true."""
    inf, nan = np.inf, np.nan
    out = []

    def case(name, X, a, b, Z, tol, groups):
        L = len(a)
        out.append(SimpleNamespace(name=name, L=L, X=_ro(np.array(X, dtype=np.float64)), a=_ro(np.array(a)),
                                   b=_ro(np.array(b)), Z=_ro(np.array(Z, dtype=np.float64)), tol=tol,
                                   full=_ro(_from_groups(L, groups))))
    I = list(IDENTITY)
    # pose 1 has a NaN cosine, pose 2 a NaN y: closures 4 (a), 5 (b) and 6 (both) go through them: V, U, Di are NaN
    case("nan-in-a-pose", [I, [nan, 0, 0, 0], [1, 0, 0, nan]], [0, 0, 0, 0, 1, 0, 2], [0, 0, 0, 0, 0, 1, 2],
         [I] * 7, CLUSTER_TOL, [[0, 1, 2, 3]])
    # pose 1 is at x = +inf.  Closure 4 starts there: V.x = inf, and inv(V) has 0 * inf = NaN in it.  Closure 5 ends
    # there: inv(X_b) has the NaN.  Closure 6 starts and ends there: inf - inf.
    case("inf-in-a-pose", [I, [1, 0, inf, 0]], [0, 0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 1, 1], [I] * 7, CLUSTER_TOL,
         [[0, 1, 2, 3]])
    # Z_4 = Z_5 = (1, 0, 1e200, 0): against 0-3 and 6, E.x = -+1e200 and dt = inf, not <= 0.0025; against each
    # other E.x = 0.  Z_6 = (1, 0, 3, 0): dt = 9 against 0-3.
    over = [I] * 4 + [[1, 0, 1e200, 0], [1, 0, 1e200, 0], [1, 0, 3, 0]]
    case("overflowing-translation", [I], [0] * 7, [0] * 7, over, CLUSTER_TOL, [[0, 1, 2, 3], [4, 5]])
    # trans_tol = inf: the bound is inf * inf + 0 = inf.  dt finite (6 against 0-3: 9), dt = inf (4 against the
    # others): both pass.  Z_5 has a NaN x: dt = NaN against everyone, and NaN <= inf is false.
    mixed = [I] * 4 + [[1, 0, 1e200, 0], [1, 0, nan, 0], [1, 0, 3, 0]]
    case("infinite-tolerance", [I], [0] * 7, [0] * 7, mixed, (inf, 0.0, 0.01, 0.0), [[0, 1, 2, 3, 4, 6]])
    # the same closures under the finite tolerance: 4 and 6 are alone too
    case("finite-tolerance", [I], [0] * 7, [0] * 7, mixed, CLUSTER_TOL, [[0, 1, 2, 3]])
    # an infinite rotation tolerance and an infinite drift with n = 0 (0 * inf = NaN in the bound: nothing passes)
    case("infinite-rot-tolerance", [I], [0] * 7, [0] * 7, [I] * 4 + [[1, 7.0, 0, 0], [1, nan, 0, 0], [1, 1e200, 0, 0]],
         (0.05, 0.0, inf, 0.0), [[0, 1, 2, 3, 4, 6]])
    case("infinite-drift-at-n-0", [I], [0] * 7, [0] * 7, [I] * 7, (0.05, inf, 0.01, 0.0), [])
    return tuple(out)
