"""GPU parity of the pairwise-consistency check (csrc/pcm_kernels.hip) on every
``pcm_peel_kernel<K>`` slot, every tile edge of the pair kernel and the capacity
L = 65,536, on the hand-placed inputs of tests/pcm_cases.py.

tests/test_pcm_gpu.py runs seeded random closures; its peel reaches slot k <= 4
with bits that matter and never launches the capacity.  Here: clusters of exact
translations at the word, wave, tile and peel-workgroup edges (group A); pairs
whose dt and dr equal their bound to the last bit or exceed it by one ulp, in
the four combinations, seen from the lower and from the higher index (B); a
clique with a straggler in every peel slot, automatic and forced, at L = 1024 K
and at an odd W whose last word has no `hi` word behind it, K = 64 at L = 64,849
and 65,536 (C); ties, the stop rule, min_size and L = 1, 2 with the order
written out (D); the capacity: nothing consistent, everything consistent (the
key of closure 0 equals the dead-slot sentinel 0xFFFFFFFF), and clusters end to
end (E); every output byte written over a 0xA5 fill and 64 guard bytes behind
each output untouched (F); NaN and infinities in poses, overflow and an infinite
tolerance (G); and a case of A, B and C again behind another L, on a side stream
and after a launch that raised the bad-index flag (H).
tests/test_pcm_cases.py shows on the CPU that the inputs are what they claim and
pins ``select_packed`` and the closed forms to tests/pcm_ref.py.

Bounds: none.  Adjacency words (padding bits included), degrees, order, keep and
steps are compared with ``np.array_equal``: only integers and individually
rounded fp64 operations decide an outcome.  ``_select`` fills order, keep and
steps with 0xA5 before every launch, so a word left unwritten fails.

L = 65,537 is refused with SLAM_ETOOBIG by both entry points before any launch:
tests/test_pcm.py::test_host_only_argument_checks has both.

Measured on an MI355X: the 131 tests of this file take 4.3 s together; the slowest are
test_capacity_nothing_consistent (65,535 peel steps) 0.44 s, test_bounds_on_the_bit[anchor-first] 0.20 s
(the restatement's 520 x 520 terms), test_every_peel_slot[K64-L65536] 0.20 s and [K64-L64849] 0.16 s,
test_capacity_everything_consistent 0.12 s and test_capacity_clusters 0.11 s; every other test is under
0.1 s.  No case failed on the kernels as they were.  On the CPU, tests/test_pcm_cases.py takes 15 s, of
which the two K = 64 slot graphs (a 512 MiB matrix each, its popcounts and 9 peels of 66 steps) take 4.6 s
and 4.2 s.

Mutation check (scratch builds, never committed; each edit of csrc/pcm_kernels.hip built and run once
against this file and tests/test_pcm_gpu.py; only values were edited, no address, guard or barrier; the
32-bit shifts were written `1u << (k & 31)`, as the hardware would take them; the tests that fail):
  `1ull << k`, `live >> k` in 32 bits   test_every_peel_slot[K64-L65536, K64-L64849],
                                        test_capacity_nothing_consistent, test_capacity_clusters;
                                        test_pcm_gpu.py: none
  `16 * lane` in `wi`                   test_every_peel_slot[all six of K = 4, 16, 64], test_clusters[1025-5,
                                        3409-3, 3409-5, 4096-3, 4096-5, 4097-3, 4097-5], test_capacity_clusters,
                                        test_every_output_byte...[3409], the five group H tests;
                                        test_pcm_gpu.py: random_closures[1025, 2049], select_alone_4097
  `lane & 32 ? wl : wh`                 59 tests: test_every_peel_slot[all eight], test_clusters[G = 3 and 5 from
                                        L = 31], test_bounds_on_the_bit[all], test_hand_graphs[ties-in-a-wave,
                                        clique-after-L-2, equal-cliques-interleaved], test_capacity_clusters,
                                        group F, group H; test_pcm_gpu.py: 17
  key index field `m` (and its decode)  91 tests: every tie (test_hand_graphs[ties-across-slots, ...],
                                        test_clusters[G = 3, 5, L], test_capacity_nothing_consistent, ...);
                                        test_pcm_gpu.py: 15
  `d >= alive - 2`                      37 tests: test_clusters[G = L], test_hand_graphs[clique-after-L-2,
                                        ends-with-1-alive, ends-with-1-alive-min2, min-size-0-one-left, L2-apart,
                                        L2-apart-min2], test_capacity_nothing_consistent, ...; test_pcm_gpu.py: 9
  `dr <`                                test_bounds_on_the_bit[all], test_nonfinite_input[infinite-rot-tolerance],
                                        the five group H tests; test_pcm_gpu.py: none
  `btd` for `brd`                       test_bounds_on_the_bit[all], the five group H tests; test_pcm_gpu.py:
                                        random_closures[1025], lap_graphs[0, 2]
  `|da + db|`                           test_bounds_on_the_bit[all], the five group H tests; test_pcm_gpu.py: 16
  `lo = l <= m`                         nothing, here or there: the pair l == m is masked by `m != l`, so the
                                        edit changes no output
  `kept = alive > min_size`             test_hand_graphs[ties-in-a-wave, clique-after-L-2, ends-with-1-alive,
                                        break-at-2-alive, min-size-4, L1, L2-connected, L2-apart],
                                        test_clusters[2-1], test_capacity_nothing_consistent,
                                        test_capacity_everything_consistent; test_pcm_gpu.py: 3
Every edit that changes an output fails a test of this file; the first and `dr <` fail none of
tests/test_pcm_gpu.py.
"""
import numpy as np
import pytest

import pcm_cases as pc
import pcm_ref
from test_pcm_gpu import _mats, _params

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _device(X, a, b, Z, tol, min_size=2, **kw):
    from slamhip import pcm
    got = pcm.consistency(X, a, b, _mats(Z), _params(tol, min_size), return_adjacency=True, **kw)
    assert got.adjacency.dtype == np.uint32 and got.keep.dtype == bool
    return got


def _upload(adj, deg):
    import torch
    return (torch.from_numpy(np.array(adj, dtype=np.uint32).view(np.int32)).cuda(),   # copies: the cases are read-only
            torch.from_numpy(np.array(deg, dtype=np.int32)).cuda())


def _select(d_adj, d_deg, min_size=2, slots=0, stream=None):
    """slam_pcm_select on a resident packed matrix, forced to ``slots`` closures a thread (0: automatic), the
    outputs filled with 0xA5 first: ``(order, keep, steps)``."""
    import torch
    from slamhip import _abi
    lib = _abi.lib()
    L = len(d_deg)
    d_order = torch.full((L,), FILL, dtype=torch.uint8, device="cuda").repeat_interleave(4).view(torch.int32)
    d_keep = torch.full((L,), FILL, dtype=torch.uint8, device="cuda")
    d_steps = torch.full((4,), FILL, dtype=torch.uint8, device="cuda").view(torch.int32)
    h = None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        h = stream.cuda_stream
    try:
        assert lib.slam_pcm_set_peel_slots(slots) == 0
        _abi.check(lib.slam_pcm_select(d_adj.data_ptr(), d_deg.data_ptr(), L, min_size, d_order.data_ptr(),
                                       d_keep.data_ptr(), d_steps.data_ptr(), h), "slam_pcm_select")
    finally:
        assert lib.slam_pcm_set_peel_slots(0) == 0
    assert lib.slam_pcm_status(h) == 0   # waits for the stream
    return d_order.cpu().numpy(), d_keep.cpu().numpy(), int(d_steps.cpu().numpy()[0])


def _forced(L):
    """Automatic, then every instance that can be forced at L (a smaller one than the automatic is not taken)."""
    return (0,) + tuple(K for K in (1, 4, 16, 64) if K >= pc.auto_slots(L))


# ---------------------------------------------------------------------------------- A

def _clusters(g, min_size=2, **kw):
    X, a, b, Z = pc.cluster_inputs(g)
    return _device(X, a, b, Z, pc.CLUSTER_TOL, min_size, **kw)


def _clusters_equal(got, g, min_size=2):
    adj, deg = pc.cluster_adjacency(g)
    order, keep, steps = pc.cluster_peel(g, min_size)
    assert np.array_equal(got.adjacency, adj), np.argwhere(got.adjacency != adj)[:4]
    assert np.array_equal(got.degree, deg)
    assert np.array_equal(got.order, order), np.flatnonzero(got.order != order)[:8]
    assert np.array_equal(got.keep, keep.astype(bool)) and got.steps == steps


@pytest.mark.parametrize("G", pc.A_GS)
@pytest.mark.parametrize("L", pc.A_LS)
def test_clusters(L, G):
    """Group A: adjacency with its padding bits, degrees, order, keep, steps against the closed forms."""
    g = pc.cluster_ids(L, G)
    _clusters_equal(_clusters(g), g)


# ---------------------------------------------------------------------------------- B

def _bounds_equal(got, c):
    """The device result of a bound case against the restatement and the bits stated by hand, both triangles."""
    adj, deg = pcm_ref.adjacency(c.X, c.a, c.b, c.Z, c.tol)
    assert np.array_equal(got.adjacency, adj), np.argwhere(got.adjacency != adj)[:4]
    assert np.array_equal(got.degree, deg)
    assert _same((got.order, got.keep, got.steps), _ref_select(c.name, adj, deg))
    full = pcm_ref.unpack(got.adjacency, c.L)
    probes = np.delete(np.arange(c.L), c.anchor)
    want = c.t_on[probes] & c.r_on[probes]
    assert np.array_equal(full[c.anchor, probes], want) and np.array_equal(full[probes, c.anchor], want)


_REF = {}


def _ref_select(name, adj, deg):
    """The restatement's peel of a bound case, computed once."""
    if name not in _REF:
        order, keep, steps = pcm_ref.select(adj, deg, 2)
        _REF[name] = (order, keep.astype(bool), steps)
    return _REF[name]


@pytest.mark.parametrize("name", list(pc.B_ANCHORS))
def test_bounds_on_the_bit(name):
    """Group B: dt and dr on their bound and one ulp above, the anchor as the low and as the high index."""
    c = pc.bound_case(name)
    _bounds_equal(_device(c.X, c.a, c.b, c.Z, c.tol), c)


# ---------------------------------------------------------------------------------- C

def _slots_equal(gr, d_adj, d_deg, **kw):
    got = _select(d_adj, d_deg, **kw)
    assert np.array_equal(got[0], gr.want[0]), (gr.name, kw, got[0][gr.stragglers])
    assert np.array_equal(got[1], gr.want[1]) and got[2] == gr.want[2]
    assert got[2] == gr.K + 2 and got[1].sum() == gr.L - gr.K - 2       # by hand
    assert np.array_equal(got[0][gr.stragglers], np.arange(gr.K + 2))


@pytest.mark.parametrize("K,L", pc.SLOT_SHAPES, ids=[pc.slot_name(*s) for s in pc.SLOT_SHAPES])
def test_every_peel_slot(K, L):
    """Group C: a straggler in every slot; a decrement lost or misplaced in any of them changes the order."""
    gr = pc.slot_graph(K, L)
    d_adj, d_deg = _upload(gr.adj, gr.deg)
    for slots in _forced(L):
        _slots_equal(gr, d_adj, d_deg, slots=slots)
    assert np.array_equal(d_deg.cpu().numpy(), gr.deg)                  # only read
    if L <= 16384:
        assert np.array_equal(d_adj.cpu().numpy().view(np.uint32), gr.adj)


# ---------------------------------------------------------------------------------- D

@pytest.mark.parametrize("case", pc.hand_graphs(), ids=[c.name for c in pc.hand_graphs()])
def test_hand_graphs(case):
    """Group D: ties, the stop rule, min_size, L = 1 and 2: the order written out by hand, on every instance."""
    d_adj, d_deg = _upload(case.adj, case.deg)
    for slots in _forced(case.L):
        got = _select(d_adj, d_deg, case.min_size, slots=slots)
        assert _same(got, case.want), (case.name, slots, got)


# ---------------------------------------------------------------------------------- E

def test_capacity_nothing_consistent():
    """65,535 steps from the highest index down, closure 0 left."""
    import torch
    L = pc.MAX_L
    d_adj = torch.zeros((L, pc.words(L)), dtype=torch.int32, device="cuda")
    d_deg = torch.zeros(L, dtype=torch.int32, device="cuda")
    order, keep, steps = _select(d_adj, d_deg, min_size=1)
    assert steps == L - 1 and keep[0] == 1 and not keep[1:].any()
    assert np.array_equal(order, np.r_[-1, np.arange(L - 2, -1, -1)])


def test_capacity_everything_consistent():
    """Degree 65,535 everywhere: the key of closure 0 is 0xFFFFFFFF, the dead-slot sentinel; no step, all kept."""
    L = pc.MAX_L
    adj, deg = pc.clique_without(L, [])
    assert deg[0] == 65535 and (int(deg[0]) << 16 | (65535 - 0)) == 0xFFFFFFFF
    d_adj, d_deg = _upload(adj, deg)
    for min_size in (2, L, L + 1):
        order, keep, steps = _select(d_adj, d_deg, min_size=min_size)
        assert steps == 0 and (order == -1).all() and keep.all() == (min_size <= L) and keep.any() == (min_size <= L)


def test_capacity_clusters():
    """Group A at L = 65,536 (W = 2,048, a pair grid of 256 x 256): two clusters of 100 and 101 go in 201 steps."""
    g = pc.capacity_clusters()
    got = _clusters(g)
    order, keep, steps = pc.cluster_peel(g)
    rows = list(pc.CAP_ROWS)
    adj, deg = pc.cluster_adjacency(g, rows=rows)
    assert got.adjacency.shape == (pc.MAX_L, 2048) and np.array_equal(got.adjacency[rows], adj)
    assert np.array_equal(got.degree, deg) and np.array_equal(got.order, order)
    assert np.array_equal(got.keep, keep.astype(bool)) and got.steps == steps == 201


# ---------------------------------------------------------------------------------- F

@pytest.mark.parametrize("L", [65, 257, 3409])
def test_every_output_byte_is_written_and_no_other(L):
    """Group F through the raw entry points: outputs filled with 0xA5, 64 guard bytes behind each."""
    import torch
    from slamhip import _abi
    lib = _abi.lib()
    g = pc.cluster_ids(L, "3")
    X, a, b, Z = pc.cluster_inputs(g)
    W = pc.words(L)
    d_X = torch.from_numpy(np.array(X, dtype=np.float64)).cuda()
    d_a = torch.from_numpy(np.array(a, dtype=np.int32)).cuda()
    d_b = torch.from_numpy(np.array(b, dtype=np.int32)).cuda()
    d_Z = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    n_work = int(lib.slam_pcm_work_size(L))
    assert n_work >= 96 * L
    size = dict(adj=4 * L * W, deg=4 * L, order=4 * L, keep=L, steps=4, work=n_work)
    buf = {k: torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, n in size.items()}
    p = {k: v.data_ptr() for k, v in buf.items()}
    tol = pc.CLUSTER_TOL
    _abi.check(lib.slam_pcm_adjacency_f64(d_X.data_ptr(), 1, d_a.data_ptr(), d_b.data_ptr(), d_Z.data_ptr(), L,
                                          tol[0], tol[1], tol[2], tol[3], p["adj"], p["deg"], p["work"], None),
               "slam_pcm_adjacency_f64")
    assert lib.slam_pcm_status(None) == 0
    after_adjacency = {k: buf[k].cpu().numpy().copy() for k in ("adj", "deg")}
    _abi.check(lib.slam_pcm_select(p["adj"], p["deg"], L, 2, p["order"], p["keep"], p["steps"], None),
               "slam_pcm_select")
    assert lib.slam_pcm_status(None) == 0
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    for k, n in size.items():
        assert (host[k][n:] == FILL).all(), k                       # the guard
    adj, deg = pc.cluster_adjacency(g)
    order, keep, steps = pc.cluster_peel(g)
    assert np.array_equal(host["adj"][:size["adj"]].view(np.uint32).reshape(L, W), adj)
    assert np.array_equal(host["deg"][:size["deg"]].view(np.int32), deg)
    assert np.array_equal(host["order"][:size["order"]].view(np.int32), order)
    assert np.array_equal(host["keep"][:L], keep)
    assert host["steps"][:4].view(np.int32)[0] == steps
    for k in ("adj", "deg"):                                        # slam_pcm_select only reads them
        assert np.array_equal(host[k], after_adjacency[k]), k


# ---------------------------------------------------------------------------------- G

@pytest.mark.parametrize("case", pc.nonfinite_cases(), ids=[c.name for c in pc.nonfinite_cases()])
def test_nonfinite_input(case):
    """Group G: the bits stated by hand; degree and place in the order follow from them."""
    got = _device(case.X, case.a, case.b, case.Z, case.tol)
    adj, deg = pc.pack_rows(case.full), case.full.sum(1)
    assert np.array_equal(got.adjacency, adj) and np.array_equal(got.degree, deg)
    assert _same((got.order, got.keep.astype(np.uint8), got.steps), pc.select_packed(adj, deg, 2))
    alone = np.flatnonzero(deg == 0)
    if len(alone) < case.L:
        assert np.array_equal(got.order[alone[::-1]], np.arange(len(alone))) and not got.keep[alone].any()


# ---------------------------------------------------------------------------------- H

H_G = ("513", "3")
H_BOUND = "anchor-middle"
H_SLOTS = (4, 3409)


def _behind(before, **kw):
    """One case each of A, B and C, each after ``before()``."""
    g = pc.cluster_ids(int(H_G[0]), H_G[1])
    before()
    _clusters_equal(_clusters(g, **kw), g)
    c = pc.bound_case(H_BOUND)
    before()
    _bounds_equal(_device(c.X, c.a, c.b, c.Z, c.tol, **kw), c)
    gr = pc.slot_graph(*H_SLOTS)
    d_adj, d_deg = _upload(gr.adj, gr.deg)
    before()
    _slots_equal(gr, d_adj, d_deg, **kw)


def test_behind_another_length():
    """Group H: after a launch of a different L on the same stream."""
    other = pc.cluster_ids(1025, "5")
    _behind(lambda: _clusters(other))


def test_on_a_side_stream():
    import torch
    other = pc.cluster_ids(257, "5")
    _behind(lambda: _clusters(other), stream=torch.cuda.Stream())


@pytest.mark.parametrize("bad", [0, 255, 512], ids=["first", "tile-end", "last"])
def test_behind_a_flagged_launch(bad):
    """A closure index outside [0, N) at closure 0, at the last closure of a 256-tile and at L - 1: reported once,
    and the next result is unaffected."""
    from slamhip import _abi, pcm
    lib = _abi.lib()
    g = pc.cluster_ids(513, "3")
    X, a, b, Z = pc.cluster_inputs(g)
    a = a.copy()
    a[bad] = 1   # N = 1

    def flagged():
        with pytest.raises(_abi.SlamHipError, match="status -1.*index"):
            pcm.consistency(X, a, b, _mats(Z), _params(pc.CLUSTER_TOL))
        assert lib.slam_pcm_status(None) == 0   # once
    _behind(flagged)
