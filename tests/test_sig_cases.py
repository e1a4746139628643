"""CPU checks of the inputs of tests/test_sig_paths_gpu.py (tests/sig_cases.py).

The GPU tests compare the signature kernels with the NumPy restatement
(tests/sig_ref.py) on hand-placed cases; here (1) the restatement itself is
pinned on every case to plain loops (``plain_signature`` and ``plain_distance``
of tests/test_sig.py, ``plain_match`` below: Python ints, a sort on (d, j), a
count by explicit comparison) and to every hand-written literal; (2) every case
is shown to be what it claims: the boundary pairs satisfy their equalities in
Python ints with the ring-count bound taken by plain loops, the far columns of
the placed lists fail the gate, every tie case ties at exactly the shifts named,
the big denominators' products exceed 2^32 and a 32-bit multiply decides the
wrap pairs the other way, the shapes give the chunk counts they claim under the
``sig_shape`` rule and the forced starts land on the edges named; (3) the number
of cases per group is asserted.

One finding about the cases themselves: for full against empty at the
denominators 2^31 - 1 and numerators 2^31 - 1 and 2^31 - 2 both products
exceed 2^43, but their low 32 bits compare like the full products (the two
sides differ by 4,096 and wrap together), so a 32-bit multiply would pass them.
``test_big_denominators`` asserts exactly that, and the ``wrap-*`` pairs are
there because of it.

No device, no mutation: every case's arrays are read-only.
"""
import math

import numpy as np
import pytest

import sig_cases as sc
import sig_ref
from test_sig import plain_distance, plain_signature

# ------------------------------------------------------------ the rule, in plain loops


def plain_rings(masks):
    return [sum((int(m) >> r) & 1 for m in masks) for r in range(32)]


def plain_lb(a, b):
    return sum(abs(x - y) for x, y in zip(plain_rings(a), plain_rings(b)))


def plain_match(sig, start, num, den, K, rows):
    """{row: (j list, d list, k list, count)} of slam_sig_match, lists of K entries padded with -1."""
    N = len(sig)
    n = [sc.popcount(s) for s in sig]
    out = {}
    for i in rows:
        found, count = [], 0
        for j in range(max(int(start[i]), 0), N):
            d, k = plain_distance(sig[i], sig[j])
            if d * den <= num * (n[i] + n[j]):
                count += 1
                found.append((d, j, k))
        found.sort()
        found = found[:K] + [(-1, -1, -1)] * (K - len(found[:K]))
        out[i] = ([f[1] for f in found], [f[0] for f in found], [f[2] for f in found], count)
    return out


def check_match(case, K, rows):
    """sig_ref.match of the case at K against plain_match on ``rows`` and against the literals."""
    j, d, k, count = case.ref(K)
    at = {int(r): a for a, r in enumerate(range(case.n_rows) if case.rows is None else case.rows)}
    want = plain_match(case.sig, case.start, case.frac[0], case.frac[1], K, rows)
    for r in rows:
        a = at[r]
        assert (j[a].tolist(), d[a].tolist(), k[a].tolist(), int(count[a])) == want[r], (case.name, K, r)
    for r in case.expect:
        ej, ed, ek, ec = case.expected(r, K)
        a = at[r]
        assert np.array_equal(j[a], ej) and np.array_equal(d[a], ed) and np.array_equal(k[a], ek), (case.name, K, r)
        assert count[a] == ec, (case.name, K, r)


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def u32(v):
    return v & 0xFFFFFFFF


# ------------------------------------------------------------------------------ group A

@pytest.mark.parametrize("S", sc.ALL_S)
def test_build_cases(S):
    dirs, edges2 = sig_ref.tables(S)
    cases = sc.build_cases(S)
    assert [c.name.rsplit("-", 1)[0] for c in cases] == ["diagonal", "one-ring", "boundary", "nonfinite"]
    for c in cases:
        with np.errstate(over="ignore", invalid="ignore"):
            got = sig_ref.signature(c.points, dirs, edges2)
        want = plain_signature(c.points, dirs, edges2)
        for a in (got, want):
            assert a[0].dtype == np.uint32 and a[1].dtype == np.uint8
            assert np.array_equal(a[0], c.sig) and np.array_equal(a[1], c.ring) and a[2] == c.n, c.name
    diag, ring1, edge, odd = cases
    assert [int(m) for m in diag.sig] == [1 << (s % 32) for s in range(S)] and len(diag.points) == S
    r0 = sc.one_ring(S)
    assert int(ring1.ring[r0]) == S == ring1.n and 0 <= r0 < 32 and (r0 == 31) == (S == 128)
    # the boundary points lie where they claim: 1e-9 rad from the boundary, on the side named
    for m, b in enumerate(sc.boundaries(S)):
        for side in (0, 1):
            x, y = edge.points[2 * m + side]
            off = math.remainder(math.atan2(y, x) - b * 2 * math.pi / S, 2 * math.pi)
            assert abs(abs(off) - 1e-9) < 1e-12 and (off > 0) == bool(side)
            assert 2 * m + side == math.floor(math.hypot(x, y) / 0.4)
    if S == 8:
        assert tuple(int(m) for m in edge.sig) == sc.BOUNDARY_SIG_8
    if S == 128:
        assert {s: int(m) for s, m in enumerate(edge.sig) if m} == sc.BOUNDARY_SIG_128
    # the odd values: r2 of each is inf, NaN or 0
    r2 = [float(x) * float(x) + float(y) * float(y) for x, y in odd.points]
    assert sum(math.isinf(v) for v in r2) == 7 and sum(math.isnan(v) for v in r2) == 4 and r2[-2:] == [0.0, 0.0]
    assert float(dirs[0][0]) * 5e-324 == 5e-324 and float(dirs[0][0]) > 0.5


# ------------------------------------------------------------------------------ group B

@pytest.mark.parametrize("S", sc.ALL_S)
def test_rolls(S):
    c = sc.roll_case(S)
    ks = sc.roll_shifts(S)
    m = len(ks)
    assert m == sc.N_SHIFTS[S] and c.N == 2 * m + 1 and set(ks) >= {0, 1, S // 2, S - 1, min(63, S - 1)}
    a = c.sig[0]
    # aperiodic: no shift but 0 maps the signature onto itself, or within 3 bits of itself
    own = [sum(bin(int(a[s]) ^ int(a[(s + k) % S])).count("1") for s in range(S)) for k in range(S)]
    assert own[0] == 0 and min(own[1:]) > 2 * sc.FLIPS_B
    D, Kk = sig_ref.distances(c.sig, [0])
    for n, k in enumerate(ks):
        assert np.array_equal(c.sig[1 + n], np.roll(a, k))
        assert plain_distance(a, c.sig[1 + n]) == (0, k) == (D[0, 1 + n], Kk[0, 1 + n])
        assert plain_distance(a, c.sig[1 + m + n]) == (sc.FLIPS_B, k) == (D[0, 1 + m + n], Kk[0, 1 + m + n])
    for K in c.Ks:
        check_match(c, K, range(c.N) if S <= 64 else (0, 1, c.N - 2))
    assert c.ref(16)[3][0] == 2 * m <= 16


@pytest.mark.parametrize("S", sc.ALL_S)
def test_realised_clouds(S):
    """The cloud of every signature of the roll case gives back its masks."""
    c = sc.roll_case(S)
    tab = sig_ref.tables(S)
    clouds = [sc.realise(s) for s in c.sig]
    got = sig_ref.signatures(clouds, *tab)
    ring, n = sig_ref.ring_counts(c.sig)
    assert np.array_equal(got[0], c.sig) and np.array_equal(got[1], ring) and np.array_equal(got[2], n)
    assert all(len(p) == k for p, k in zip(clouds, n))
    if S in (24, 120):
        assert np.array_equal(plain_signature(clouds[0], *tab)[0], c.sig[0])
    assert np.array_equal(sig_ref.signature(sc.realise(np.zeros(S, np.uint32)), *tab)[0], np.zeros(S, np.uint32))


# ------------------------------------------------------------------------------ group C

@pytest.mark.parametrize("S,period,roll", sc.TIES)
def test_ties(S, period, roll):
    c = sc.tie_case(S, period, roll)
    a = c.sig[0]
    assert all(np.array_equal(a, np.roll(a, period * m)) for m in range(S // period))
    for col, d in ((1, 0), (2, 3)):
        ds = [sum(bin(int(a[s]) ^ int(c.sig[col][(s + k) % S])).count("1") for s in range(S)) for k in range(S)]
        assert min(ds) == d and [k for k in range(S) if ds[k] == d] == sc.TIE_SHIFTS[S]
        assert plain_distance(a, c.sig[col]) == (d, 6)
    assert sc.TIE_SHIFTS[S][0] == 6 and (S <= 64 or sc.TIE_SHIFTS[S][-1] >= 64)
    for K in c.Ks:
        check_match(c, K, range(3))


# ------------------------------------------------------------------------------ group D

def test_pairs_on_the_bounds():
    c = sc.boundary_pairs_case()
    base, n_i = c.sig[0], 3
    assert sc.popcount(base) == n_i and c.frac == (1, 4)
    facts = {}
    for col, name in enumerate(sc.BASE_PAIRS, start=1):
        d, lb, n_j = plain_distance(base, c.sig[col])[0], plain_lb(base, c.sig[col]), sc.popcount(c.sig[col])
        assert (d, lb, n_j) == sc.BASE_PAIRS[name], name
        facts[name] = (4 * lb <= n_i + n_j, 4 * d <= n_i + n_j)
    assert 4 * 2 == 3 + 5                                           # inside: on both bounds
    assert facts == {"inside": (True, True), "outside": (False, False), "screen passes": (True, False),
                     "gate outside": (True, False)}
    g = sc.gate_only_case()
    assert plain_distance(g.sig[0], g.sig[1]) == (2, 0) and plain_lb(g.sig[0], g.sig[1]) == 0
    assert 4 * 2 == sc.popcount(g.sig[0]) + sc.popcount(g.sig[1])   # the gate's bound, the screen far inside
    p = sc.plus_one_case()
    lb, nij = plain_lb(p.sig[0], p.sig[1]), sc.popcount(p.sig[0]) + sc.popcount(p.sig[1])
    assert p.frac == (1, 2) and lb * 2 == 1 * nij + 1 and plain_distance(p.sig[0], p.sig[1])[0] == lb == 3
    for case in (c, g, p):
        for K in case.Ks:
            check_match(case, K, range(case.n_rows))


def test_big_denominators():
    big = sc.BIG
    assert big == 2 ** 31 - 1 and sc.FULL_EMPTY_FRACS == ((1, 1), (big, big), (big - 1, big))
    for frac in sc.FULL_EMPTY_FRACS:
        c = sc.full_empty_case(frac)
        d, lb = plain_distance(c.sig[0], c.sig[1])[0], plain_lb(c.sig[0], c.sig[1])
        nij = sc.popcount(c.sig[0]) + sc.popcount(c.sig[1])
        assert d == lb == nij == 4096 and max(plain_rings(c.sig[0])) == 128
        num, den = frac
        assert (d * den <= num * nij) == (num == den)
        if den == big:
            assert d * den > 2 ** 32 and num * nij > 2 ** 32
            # the two sides differ by 0 or 4,096 and wrap together: the low words compare like the products
            assert (s32(d * den) <= s32(num * nij)) == (u32(d * den) <= u32(num * nij)) == (num == den)
        for K in c.Ks:
            check_match(c, K, range(3))
    for name, (frac, row, col, d, lb, cand) in sc.WRAP_PAIRS.items():
        c = sc.wrap_case(name)
        num, den = frac
        nij = sc.popcount(row) + sc.popcount(col)
        assert plain_distance(row, col) == (d, 0) and plain_lb(row, col) == lb and den == big
        assert (lb == d) == name.endswith("screen") and (lb == 0) == name.endswith("gate")
        assert (d * den <= num * nij) == cand == name.startswith("in")
        assert max(d * den, num * nij) >= 2 ** 32
        assert (s32(d * den) <= s32(num * nij)) == (u32(d * den) <= u32(num * nij)) == (not cand), name
        for K in c.Ks:
            check_match(c, K, range(2))


# ------------------------------------------------------------------------------ group E

def test_far_columns_fail_the_gate():
    base = sc.base_e()
    n_i = sc.popcount(base)
    passes_screen = 0
    for j in range(1, sc.N_E):
        col = sc.far(j)
        d, n_j = plain_distance(base, col)[0], sc.popcount(col)
        assert 4 * d > n_i + n_j, j
        passes_screen += 4 * plain_lb(base, col) <= n_i + n_j
    assert passes_screen >= sc.N_E // 2 - 1                         # the odd columns: equal ring counts
    assert sc.chunk_shape(sc.N_E) == (256, 3) and sc.N_E - 2 * 256 == 8


@pytest.mark.parametrize("name", list(sc.PLACED))
def test_placed_lists(name):
    c = sc.placed_case(name)
    named, js = sc.PLACED[name]
    base, n_i = sc.base_e(), sc.popcount(sc.base_e())
    for j, f in named.items():
        assert plain_distance(base, c.sig[j]) == (f, 0) and 4 * f <= n_i + sc.popcount(c.sig[j]), j
    for j in range(1, sc.N_E):
        if j not in named:
            assert np.array_equal(c.sig[j], sc.far(j))
    order = sorted(named, key=lambda j: (named[j], j))
    assert js == order[:16] and len(set(js)) == len(js)
    for K in c.Ks:
        check_match(c, K, (0, min(named), sc.N_E - 1))


def test_placements_are_what_they_claim():
    asc, desc = sc.PLACED["ascending"][0], sc.PLACED["descending"][0]
    assert len(asc) == 20 and max(asc) < 256 and [asc[j] for j in sorted(asc)] == list(range(1, 21))
    assert [desc[j] for j in sorted(desc)] == list(range(20, 0, -1))
    for name in ("edge-pairs", "edge-all-equal"):
        p = sc.PLACED[name][0]
        assert sorted(p) == [63, 64, 255, 256, 511, 512] and p[63] == p[64] and p[255] == p[256] and p[511] == p[512]
    last, js = sc.PLACED["last-chunk"]
    assert set(range(512, 520)) <= set(js) and len(last) == 21 and len(js) == 16
    assert {j // 256 for j in js} == {0, 1, 2} and max(last[j] for j in js) < min(last[j] for j in last if j not in js)
    for n in sc.COUNTS:
        p = sc.PLACED["count-%d" % n][0]
        assert len(p) == n and (n < 10 or {j // 256 for j in p} == {0, 1, 2})
    assert {n for n in sc.COUNTS} >= {K for K in sc.KS} | {K + 1 for K in sc.KS}   # exactly K and K + 1 for every K


# ------------------------------------------------------------------------------ group F

def restated_shape(N):
    w = max(256, (((N + 15) // 16) + 63) // 64 * 64)
    return w, (N + w - 1) // w


@pytest.mark.parametrize("N", sc.SHAPE_N)
def test_shapes(N):
    assert sc.chunk_shape(N) == restated_shape(N) == sc.SHAPE_CHUNKS[N]
    chunk = restated_shape(N)[0]
    c1 = min(chunk, N)
    start = sc.shape_start(N)
    f = sc.forced_starts(N)
    assert start[:len(f)].tolist() == f[:N] and 0 <= start.min() and start.max() <= N and len(start) == N
    want = {v for v in (0, 63, 64, 65, c1 - 1, c1, c1 + 1, N - 1, N) if 0 <= v <= N}
    assert set(f) == want
    if N > 65:
        assert {0, N} <= set(start.tolist())
        assert any(s % 64 == 0 and s > 0 for s in f) and any(s % 64 not in (0, 63) for s in f)   # on and inside a tile
        assert (c1 in f) and (N <= chunk or chunk in f)                                          # on c1 = the next c0
    cases = [c for c in sc.shape_cases() if c.N == N]
    assert [c.n_rows for c in cases] == sorted({r for r in sc.SHAPE_ROWS if r <= N} | {N})
    for c in cases:
        (K,) = c.Ks
        if c.rows is not None:
            assert len(c.rows) >= sc.N_SAMPLE and set(range(min(len(f), c.n_rows))) <= set(c.rows.tolist())
        if N <= 65:
            rows = range(c.n_rows)
        elif c.n_rows == N:
            rows = (0, 4, len(f) - 1, N - 1)
        else:
            rows = (c.n_rows - 1,)
        check_match(c, K, rows)
    full = cases[-1].ref(16)
    if N >= 255:
        assert (full[3] > 16).any() and (full[3] == 0).any()


def test_single_starts():
    for start in (0, 1):
        c = sc.single_start_case(start)
        for K in c.Ks:
            check_match(c, K, (0,))


def test_shifted_cases_keep_their_answers():
    """``shifted`` moves a case up p rows: the restatement's answers move with it."""
    for c in (sc.roll_case(72), sc.tie_case(*sc.TIES[0]), sc.boundary_pairs_case(), sc.placed_case("last-chunk"),
              sc.shape_case(257, 17)):
        s = sc.shifted(c, 5)
        K = c.Ks[-1]
        a, b = c.ref(K), s.ref(K)
        assert s.N == c.N + 5 and (b[3][:5] == 0).all()
        assert np.array_equal(np.where(b[0][5:] >= 0, b[0][5:] - 5, -1), a[0])
        assert all(np.array_equal(x[5:], y) for x, y in zip(b[1:], a[1:]))


# ------------------------------------------------------------------------------- counts

def test_case_counts():
    groups = sc.match_cases()
    assert {g: len(v) for g, v in groups.items()} == {"B": 16, "C": 3, "D": 10, "E": 11, "F": 83}
    assert sum(len(sc.build_cases(S)) for S in sc.ALL_S) == 64 and len(sc.ALL_S) == 16
    names = [c.name for v in groups.values() for c in v]
    assert len(set(names)) == len(names)
    assert [c.S for c in groups["B"]] == list(range(8, 129, 8))
    for v in groups.values():
        for c in v:
            assert not c.sig.flags.writeable and not c.start.flags.writeable
    for S in sc.ALL_S:
        assert all(not b.points.flags.writeable and not b.sig.flags.writeable for b in sc.build_cases(S))
