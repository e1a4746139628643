"""Hand-placed inputs for the scan signatures (no GPU; no randomness but the
seeded fills named below).

csrc/sig_kernels.hip compiles one ``sig_scan_kernel<S>`` for each of the sixteen
sector counts S = 8, 16, ..., 128, each with its own register-resident rotation
table: for S < 64 the 64 lanes wrap through ``(S - lane % S) % S``, for S > 64
the shifts 64 and up are a second pass ``rot[(t + S - 64) % S]``.  A pair is
decided by two integer comparisons (the ring-count screen ``lb den <= num (n_i
+ n_j)`` and the gate ``d den <= num (n_i + n_j)``) in 64-bit products, a
candidate goes into a sorted list of K slots per (row, column chunk), and the
chunks' lists are merged.  The cases here put inputs on those positions by hand:

* group A (build, every S): one point per sector on the sector's centre angle
  in ring ``s % 32`` (``sig[s] == 1 << (s % 32)``); every sector's point in one
  ring (``ring[r0] == S``: 128 in the uint8 at S = 128); points 1e-9 rad on
  either side of four sector boundaries; infinities, 1e200, NaN, a denormal
  and -0.0;
* group B (match, every S): an aperiodic signature against its rolls by 0, 1,
  S / 2, S - 1, min(63, S - 1) and min(64, S - 1), exact (d = 0, k the roll)
  and with three bits flipped (d = 3); a cloud that realises the same masks;
* group C: periodic signatures for which a shift below 64 ties with one found
  by the second pass (or by a wrapped lane): the first shift wins;
* group D: pairs exactly on the gate and on the screen, one step outside, and
  denominators near 2^31 whose products a 32-bit multiply would wrap;
* group E: 520 signatures of 8 masks (chunks of 256, 256 and 8 columns) in
  which only named columns are candidates of row 0, at distances that arrive
  ascending, descending, equal across tile and chunk edges, with the best all
  in the short last chunk, and 1, 2, 3, 15, 16 and 17 candidates in all;
* group F: N on either side of the tile, the minimum chunk and the step at
  which the chunk grows, starts on every edge, n_rows around the 4 rows of a
  scan workgroup and the 16 rows of a merge workgroup.

Every array is read-only; every case is built once per process and its
restatement result is computed once (``MatchCase.ref``) and shared.

tests/test_sig_cases.py checks these inputs on the CPU;
tests/test_sig_paths_gpu.py runs them on the GPU.
"""
import functools

import numpy as np

import sig_ref
from test_sig_gpu import _random_signatures

RINGS = 32
ALL_S = tuple(range(8, 129, 8))       # the sixteen sig_scan_kernel<S>
TILE = 64                             # kSigTile
MIN_CHUNK = 256                       # kSigMinChunk
MAX_CHUNKS = 16                       # kSigMaxChunks
SCAN_ROWS = 4                         # rows per sig_scan_kernel workgroup (one wave each)
MERGE_ROWS = 16                       # rows per sig_merge_kernel workgroup (16 lanes each)
KS = (1, 2, 15, 16)
DR = 0.4                              # SigParams' default ring width, r_min = 0


def _ro(a):
    a.setflags(write=False)
    return a


def _u32(a):
    return _ro(np.array(a, dtype=np.uint64).astype(np.uint32))


def chunk_shape(N):
    """(chunk, n_chunks) of sig_shape: at most 16 chunks of whole tiles, 256 columns at least."""
    per = -(-N // MAX_CHUNKS)
    w = max(-(-per // TILE) * TILE, MIN_CHUNK)
    return w, -(-N // w)


def popcount(masks):
    return sum(bin(int(m)).count("1") for m in masks)


def flip(sig, positions):
    """``sig`` (S masks) with the bits at flat positions q (sector q % S, ring q // S) flipped."""
    out = np.array(sig, dtype=np.uint32)
    S = len(out)
    for q in positions:
        out[q % S] ^= np.uint32(1 << (q // S))
    return out


# ----------------------------------------------------------------------- group A: build

class BuildCase:
    """One scan for ``SigParams(sectors=S)`` (r_min = 0, dr = 0.4); ``sig`` (S,), ``ring`` (32,)
    and ``n`` are written by rule, not computed from the points."""

    def __init__(self, name, S, points, sig, ring=None, n=None):
        self.name, self.S = name, S
        self.points = _ro(np.array(points, np.float64).reshape(-1, 2))
        self.sig = _u32(sig)
        assert self.sig.shape == (S,)
        self.ring = None if ring is None else _ro(np.array(ring, np.uint8))
        self.n = n


def polar(S, sector_pos, ring_pos):
    """The point at angle ``sector_pos`` sectors and radius ``ring_pos`` rings."""
    a, r = sector_pos * 2 * np.pi / S, ring_pos * DR
    return (r * np.cos(a), r * np.sin(a))


def one_ring(S):
    """The ring of the one-ring cloud: 1, 3, ..., 31 (bit 31 at S = 128)."""
    return S // 4 - 1


@functools.lru_cache(maxsize=None)
def diagonal_case(S):
    """Point s on the centre angle of sector s in the middle of ring s % 32."""
    pts = [polar(S, s + 0.5, s % RINGS + 0.5) for s in range(S)]
    ring = [len(range(r, S, RINGS)) for r in range(RINGS)]
    return BuildCase("diagonal-%d" % S, S, pts, [1 << (s % RINGS) for s in range(S)], ring, S)


@functools.lru_cache(maxsize=None)
def one_ring_case(S):
    """Every sector's point in ring r0: ring[r0] == S == n."""
    r0 = one_ring(S)
    pts = [polar(S, s + 0.5, r0 + 0.5) for s in range(S)]
    return BuildCase("one-ring-%d" % S, S, pts, [1 << r0] * S, [S if r == r0 else 0 for r in range(RINGS)], S)


EPS_ANGLE = 1e-9                      # rad


def boundaries(S):
    """The four sector boundaries b (the angle b 2 pi / S between sectors b - 1 and b)."""
    return (0, 1, S // 2, S - 1)


@functools.lru_cache(maxsize=None)
def boundary_case(S):
    """Boundary number m of ``boundaries(S)``: a point 1e-9 rad below it in ring 2 m, which falls
    in sector b - 1 (S - 1 for b = 0), and one 1e-9 rad above it in ring 2 m + 1, in sector b."""
    pts, sig = [], [0] * S
    for m, b in enumerate(boundaries(S)):
        for side, sector in ((-1, (b - 1) % S), (1, b)):
            r = 2 * m + (side > 0)
            a = b * 2 * np.pi / S + side * EPS_ANGLE
            pts.append(((r + 0.5) * DR * np.cos(a), (r + 0.5) * DR * np.sin(a)))
            sig[sector] |= 1 << r
    return BuildCase("boundary-%d" % S, S, pts, sig, [1] * 8 + [0] * 24, 8)


# at S = 8 the rule gives: below 0 -> sector 7 ring 0, above 0 -> sector 0 ring 1, below 1 -> sector 0 ring 2,
# above 1 -> sector 1 ring 3, below 4 -> sector 3 ring 4, above 4 -> sector 4 ring 5, below 7 -> sector 6
# ring 6, above 7 -> sector 7 ring 7
BOUNDARY_SIG_8 = (0b110, 0b1000, 0, 0b10000, 0b100000, 0, 0b1000000, 0b10000001)
BOUNDARY_SIG_128 = {127: 0b10000001, 0: 0b110, 1: 0b1000, 63: 0b10000, 64: 0b100000, 126: 0b1000000}

NONFINITE = ((np.inf, 0.0), (-np.inf, 1.0), (0.0, np.inf), (np.inf, -np.inf), (1e200, 0.0), (0.0, -1e200),
             (1e200, 1e200), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.nan),
             (-0.0, -0.0), (5e-324, 0.0))


@functools.lru_cache(maxsize=None)
def nonfinite_case(S):
    """r2 is inf for the infinities and for 1e200 (past every ring), NaN for the NaNs (in no
    ring); -0.0 has r2 = 0 and every projection +-0: ring 0, sector 0 of an all-way tie; the
    denormal has r2 = 0 and the projection 5e-324 in every sector whose cosine exceeds 1/2: ring
    0, sector 0 again.  One bit in all."""
    return BuildCase("nonfinite-%d" % S, S, NONFINITE, [1] + [0] * (S - 1), [1] + [0] * 31, 1)


def build_cases(S):
    return [diagonal_case(S), one_ring_case(S), boundary_case(S), nonfinite_case(S)]


def realise(sig):
    """A cloud with one point for every set bit (sector s, ring r) of ``sig`` (S masks): on the
    sector's centre angle in the middle of the ring; a point outside every ring if none is set."""
    S = len(sig)
    pts = [polar(S, s + 0.5, r + 0.5) for s in range(S) for r in range(RINGS) if (int(sig[s]) >> r) & 1]
    return _ro(np.array(pts if pts else [(100.0, 0.0)], np.float64))


# ----------------------------------------------------------------------- match cases

class MatchCase:
    """``sig`` (N, S) against itself: rows ``0..n_rows-1`` from ``start`` at ``frac = (num,
    den)``.  ``expect``: {row: (j list, d list, k list, count)}, the row's whole sorted list (its
    first 16 entries) written by hand; ``rows``: the rows compared (all when None)."""

    def __init__(self, name, sig, start, n_rows, frac, expect=None, rows=None, Ks=KS):
        self.name = name
        self.sig = _ro(np.array(sig, dtype=np.uint32))
        self.N, self.S = self.sig.shape
        self.start = _ro(np.array(start, np.int64))
        self.n_rows, self.frac, self.Ks = int(n_rows), tuple(frac), tuple(Ks)
        self.expect = dict(expect or {})
        self.rows = None if rows is None else _ro(np.array(rows, np.int64))
        self._ref = {}
        assert len(self.start) >= self.n_rows and 0 <= self.n_rows <= self.N

    def ref(self, K):
        """sig_ref.match on the compared rows: (j, d, k (len(rows), K), count)."""
        if K not in self._ref:
            out = sig_ref.match(self.sig, self.start, self.n_rows, self.frac[0], self.frac[1], K, self.rows)
            self._ref[K] = tuple(_ro(o) for o in out)
        return self._ref[K]

    def expected(self, row, K):
        """The hand-written (j, d, k (K,), count) of ``row``, cut or padded with -1 to K slots."""
        j, d, k, count = self.expect[row]
        assert len(j) == len(d) == len(k) == min(count, 16)
        pad = [-1] * K
        return tuple(np.array((list(v) + pad)[:K], np.int64) for v in (j, d, k)) + (count,)


def shifted(case, p, seed=77):
    """The case behind ``p`` seeded rows that look at nothing (start == N): every row and column
    index moves up by p, to other waves, tiles and chunk offsets."""
    fill = _random_signatures(p, case.S, seed)
    start = np.r_[np.full(p, case.N + p), case.start[:case.n_rows] + p]
    rows = None if case.rows is None else np.r_[np.arange(p), case.rows + p]
    return MatchCase(case.name + "+%d" % p, np.concatenate([fill, case.sig]), start, case.n_rows + p, case.frac,
                     rows=rows, Ks=case.Ks)


# ------------------------------------------------------------ group B: rolls at every S

FLIPS_B = 3


def roll_shifts(S):
    """0, 1, S / 2, S - 1, min(63, S - 1), min(64, S - 1), each once, ascending."""
    return tuple(sorted({0, 1, S // 2, S - 1, min(63, S - 1), min(64, S - 1)}))


N_SHIFTS = {8: 4, 16: 4, 24: 4, 32: 4, 40: 4, 48: 4, 56: 4, 64: 4, 72: 6, 80: 6, 88: 6, 96: 6, 104: 6, 112: 6,
            120: 6, 128: 5}


@functools.lru_cache(maxsize=None)
def aperiodic(S):
    """The fixed-seed signature of group B: S masks of uniform random bits."""
    return _ro(np.random.default_rng(4000 + S).integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def roll_case(S):
    """Row 0 is a; columns 1..m are np.roll(a, k) for the m shifts k of ``roll_shifts``; columns
    m + 1..2 m the same with three bits flipped (in sectors 0, 1 and 2 of the column, rings 5, 6,
    7).  Row 0's list at 1/4: the exact rolls with d = 0, then the flipped ones with d = 3, each
    at its k.  Every row runs from i + 1."""
    a = aperiodic(S)
    ks = roll_shifts(S)
    m = len(ks)
    exact = [np.roll(a, k) for k in ks]
    flipped = [flip(c, [5 * S, 6 * S + 1, 7 * S + 2]) for c in exact]
    sig = np.stack([a] + exact + flipped)
    expect = {0: (list(range(1, 2 * m + 1)), [0] * m + [FLIPS_B] * m, list(ks) * 2, 2 * m)}
    return MatchCase("rolls-%d" % S, sig, np.arange(len(sig)) + 1, len(sig), (1, 4), expect)


# ------------------------------------------------- group C: ties across the two passes

# (S, period, roll): the shifts that tie are roll % period + m period; the first is 6 everywhere
TIES = ((128, 64, 70), (72, 8, 70), (16, 8, 14))
TIE_SHIFTS = {128: [6, 70], 72: [6, 14, 22, 30, 38, 46, 54, 62, 70], 16: [6, 14]}


@functools.lru_cache(maxsize=None)
def tie_case(S, period, roll):
    """Row 0 has the given period; column 1 is its roll, column 2 the roll with three bits
    flipped in sector 3.  (d, k) = (0, 6) and (3, 6)."""
    unit = np.random.default_rng(5000 + S).integers(0, 1 << 32, size=period, dtype=np.uint64).astype(np.uint32)
    a = np.tile(unit, S // period)
    b = np.roll(a, roll)
    c = flip(b, [4 * S + 3, 9 * S + 3, 30 * S + 3])
    expect = {0: ([1, 2], [0, 3], [6, 6], 2)}
    return MatchCase("tie-%d" % S, np.stack([a, b, c]), [1, 2, 3], 3, (1, 4), expect)


# ------------------------------------------------------ group D: the gate and the screen

BASE_D = (1, 2, 0, 4, 0, 0, 0, 0)                   # n = 3, one bit in each of the rings 0, 1, 2
INSIDE = (1, 2, 0, 4, 0, 8, 16, 0)                  # n = 5: d = lb = 2 and 4 * 2 == 3 + 5
OUTSIDE = (0, 2, 0, 4, 0, 8, 0, 0)                  # n = 3: d = lb = 2 and 4 * 2 > 3 + 3
SCREEN_PASSES = (1, 0, 2, 0, 0, 4, 0, 0)            # n = 3, the rings of the base (lb = 0), d = 4: 16 > 6
GATE_OUTSIDE = (1, 2, 0, 0, 4, 0, 0, 0)             # n = 3, the rings of the base (lb = 0), d = 2: 8 > 6
# the gate alone on its bound: equal ring counts (lb = 0), one bit in another sector (d = 2), n = 4 + 4
GATE_ROW = (1, 2, 0, 4, 0, 0, 8, 0)
GATE_ON = (1, 2, 0, 4, 0, 8, 0, 0)                  # 4 * 2 == 4 + 4
# the screen one step outside: rings {0, 1, 2, 3} against ring {0}: lb = 3, and at 1/2: 2 * 3 == (4 + 1) + 1
PLUS_ONE_ROW = (1, 2, 4, 8, 0, 0, 0, 0)
PLUS_ONE_COL = (1, 0, 0, 0, 0, 0, 0, 0)
# name -> (d, lb, n_j) of the base's columns 1..4
BASE_PAIRS = {"inside": (2, 2, 5), "outside": (2, 2, 3), "screen passes": (4, 0, 3), "gate outside": (2, 0, 3)}


@functools.lru_cache(maxsize=None)
def boundary_pairs_case():
    """Row 0 (the base) against the inside, outside, screen-passes and gate-outside columns:
    at 1/4 its one candidate is column 1."""
    sig = [BASE_D, INSIDE, OUTSIDE, SCREEN_PASSES, GATE_OUTSIDE]
    return MatchCase("on-the-bounds", sig, [1, 5, 5, 5, 5], 5, (1, 4), {0: ([1], [2], [0], 1)})


@functools.lru_cache(maxsize=None)
def gate_only_case():
    return MatchCase("gate-on-its-bound", [GATE_ROW, GATE_ON], [1, 2], 2, (1, 4), {0: ([1], [2], [0], 1)})


@functools.lru_cache(maxsize=None)
def plus_one_case():
    return MatchCase("screen-plus-one", [PLUS_ONE_ROW, PLUS_ONE_COL], [1, 2], 2, (1, 2), {0: ([], [], [], 0)})


BIG = 2 ** 31 - 1
FULL_EMPTY_FRACS = ((1, 1), (BIG, BIG), (BIG - 1, BIG))


@functools.lru_cache(maxsize=None)
def full_empty_case(frac):
    """S = 128: all masks 0xFFFFFFFF (every ring count 128), all zero, all set again, rows from
    0.  d(0, 1) = lb = n_0 + n_1 = 4,096, the largest there is: a candidate at 1/1 and at
    (2^31 - 1) / (2^31 - 1), none one step below."""
    full, zero = [0xFFFFFFFF] * 128, [0] * 128
    if frac[0] == frac[1]:
        expect = {0: ([0, 2, 1], [0, 0, 4096], [0, 0, 0], 3), 1: ([1, 0, 2], [0, 4096, 4096], [0, 0, 0], 3)}
    else:
        expect = {0: ([0, 2], [0, 0], [0, 0], 2), 1: ([1], [0], [0], 1)}
    return MatchCase("full-empty-%d/%d" % frac, [full, zero, full], [0, 0, 0], 3, frac, expect)


# Products that a 32-bit multiply decides the other way, under the signed and under the unsigned
# reading of the low 32 bits (tests/test_sig_cases.py shows it).  name -> (frac, row, column, d, lb,
# candidate?).  With den = 2^31 - 1 the low word of d den is 2^31 - d for odd d and -d for even d.
#   in, 1/2 = 2^30 / den:     1 den = 2,147,483,647 <= 5 * 2^30 = 5,368,709,120, low word 2^30
#                             2 den = 4,294,967,294 <= 6 * 2^30 = 6,442,450,944, low word 2^31
#   out, 715,827,882 / den:   3 den = 6,442,450,941 >  3 num = 2,147,483,646 = 2^31 - 2, unwrapped
#                             4 den = 8,589,934,588 >  6 num = 4,294,967,292 = 2^32 - 4, unwrapped
THIRD = 715827882                     # (2^31 - 2) / 3
WRAP_PAIRS = {
    "in-screen": ((2 ** 30, BIG), (1, 2, 0, 4, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0, 0, 0), 1, 1, True),
    "in-gate": ((2 ** 30, BIG), (1, 2, 0, 4, 0, 0, 0, 0), (1, 2, 0, 0, 4, 0, 0, 0), 2, 0, True),
    "out-screen": ((THIRD, BIG), (1, 2, 0, 4, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0), 3, 3, False),
    "out-gate": ((THIRD, BIG), (1, 2, 0, 4, 0, 0, 0, 0), (1, 0, 2, 0, 0, 4, 0, 0), 4, 0, False),
}


@functools.lru_cache(maxsize=None)
def wrap_case(name):
    """One row against one column; "screen": lb = d, the screen meets the product first; "gate":
    equal ring counts, only the gate does."""
    frac, row, col, d, _, cand = WRAP_PAIRS[name]
    expect = {0: ([1], [d], [0], 1) if cand else ([], [], [], 0)}
    return MatchCase("wrap-" + name, [row, col], [1, 2], 2, frac, expect)


# --------------------------------------------------------------- group E: the sorted list

N_E = 520                             # chunks of 256, 256 and 8 columns


@functools.lru_cache(maxsize=None)
def base_e():
    """Row 0 of group E: 8 masks of uniform random bits (seed 6000)."""
    return _ro(np.random.default_rng(6000).integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32))


def near(j, f):
    """The base with f bits flipped, at positions that depend on j: d = f at shift 0."""
    return flip(base_e(), [(7 * j + 37 * t) % 256 for t in range(f)])


def far(j):
    """Not a candidate of the base at 1/4: the complement for even j; for odd j the base's ring
    bits dealt to other sectors (equal ring counts: the screen passes it, the gate does not)."""
    b = base_e()
    if j % 2 == 0:
        return ~b
    out = np.zeros(8, np.uint32)
    for r in range(RINGS):
        bits = [(int(b[s]) >> r) & 1 for s in range(8)]
        for s in range(8):
            out[(3 * s + r + j) % 8] |= np.uint32(bits[s] << r)
    return out


# name -> ({j: f}, the j of row 0's list at K = 16)
PLACED = {
    "ascending": ({3 * m + 1: m + 1 for m in range(20)},
                  [1, 4, 7, 10, 13, 16, 19, 22, 25, 28, 31, 34, 37, 40, 43, 46]),
    "descending": ({3 * m + 1: 20 - m for m in range(20)},
                   [58, 55, 52, 49, 46, 43, 40, 37, 34, 31, 28, 25, 22, 19, 16, 13]),
    "edge-pairs": ({63: 3, 64: 3, 255: 2, 256: 2, 511: 1, 512: 1}, [511, 512, 255, 256, 63, 64]),
    "edge-all-equal": ({63: 2, 64: 2, 255: 2, 256: 2, 511: 2, 512: 2}, [63, 64, 255, 256, 511, 512]),
    "last-chunk": ({**{512 + t: t + 1 for t in range(8)}, 300: 9, 301: 10, 302: 11, 303: 12, 10: 13, 11: 14,
                    12: 15, 13: 16, 20: 17, 21: 18, 22: 19, 23: 20, 400: 18},
                   [512, 513, 514, 515, 516, 517, 518, 519, 300, 301, 302, 303, 10, 11, 12, 13]),
}
COUNTS = (1, 2, 3, 15, 16, 17)


def count_placement(n):
    """n candidates, one every 30 columns down from 519 (all three chunks from n = 10 on), with
    f = 1 + 5 t mod 7: ties and both orders."""
    return {519 - 30 * t: 1 + (5 * t) % 7 for t in range(n)}


# the j of row 0's list at K = 16, by (f, j): f of 519, 489, ... is 1, 6, 4, 2, 7, 5, 3, 1, 6, 4, 2, 7, 5, 3, 1, 6, 4
COUNT_LISTS = {
    1: [519],
    2: [519, 489],
    3: [519, 459, 489],
    15: [99, 309, 519, 219, 429, 129, 339, 249, 459, 159, 369, 279, 489, 189, 399],
    16: [99, 309, 519, 219, 429, 129, 339, 249, 459, 159, 369, 69, 279, 489, 189, 399],
    17: [99, 309, 519, 219, 429, 129, 339, 39, 249, 459, 159, 369, 69, 279, 489, 189],
}
for _n in COUNTS:
    PLACED["count-%d" % _n] = (count_placement(_n), COUNT_LISTS[_n])


@functools.lru_cache(maxsize=None)
def placed_case(name):
    """Row 0 from column 1; every other row from its own next column."""
    named, js = PLACED[name]
    sig = np.stack([base_e()] + [near(j, named[j]) if j in named else far(j) for j in range(1, N_E)])
    expect = {0: (js, [named[j] for j in js], [0] * len(js), len(named))}
    return MatchCase("placed-" + name, sig, np.arange(N_E) + 1, N_E, (1, 4), expect)


# ---------------------------------------------------------------------- group F: shapes

SHAPE_N = (1, 63, 64, 65, 255, 256, 257, 512, 513, 4096, 4097)
SHAPE_ROWS = (1, SCAN_ROWS - 1, SCAN_ROWS, SCAN_ROWS + 1, MERGE_ROWS - 1, MERGE_ROWS, MERGE_ROWS + 1)   # and N
assert SHAPE_ROWS == (1, 3, 4, 5, 15, 16, 17)
SHAPE_CHUNKS = {1: (256, 1), 63: (256, 1), 64: (256, 1), 65: (256, 1), 255: (256, 1), 256: (256, 1), 257: (256, 2),
                512: (256, 2), 513: (256, 3), 4096: (256, 16), 4097: (320, 13)}
SHAPE_FRAC = (2, 5)
N_SAMPLE = 200


def forced_starts(N):
    """0, 63, 64, 65, c1 - 1, c1, c1 + 1, N - 1, N where they lie in [0, N], each once, in this
    order; c1 = min(chunk, N) is the end of the first column chunk."""
    c1 = min(chunk_shape(N)[0], N)
    out = []
    for v in (0, 63, 64, 65, c1 - 1, c1, c1 + 1, N - 1, N):
        if 0 <= v <= N and v not in out:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def shape_sig(N):
    return _ro(_random_signatures(N, 8, 7000 + N))


@functools.lru_cache(maxsize=None)
def shape_start(N):
    """Random starts in [0, N], the first rows forced (at N = 1 the one row starts at 0;
    ``single_start_case`` adds the start 1)."""
    start = np.random.default_rng(7100 + N).integers(0, N + 1, size=N)
    f = forced_starts(N)
    start[:len(f)] = f[:N]
    return _ro(start)


@functools.lru_cache(maxsize=None)
def shape_case(N, n_rows):
    """Up to 513 every row is compared; above, the forced rows, the rows around the workgroup
    edges and a seeded sample: at least 200 rows."""
    rows = None
    if N > 513 and n_rows > N_SAMPLE:
        rows = np.unique(np.r_[np.arange(17), 255, 256, 257, 319, 320, 321, n_rows - 2, n_rows - 1,
                               np.random.default_rng(7200 + N).integers(0, n_rows, N_SAMPLE)])
    return MatchCase("shape-%d-rows-%d" % (N, n_rows), shape_sig(N), shape_start(N), n_rows, SHAPE_FRAC, rows=rows,
                     Ks=(4,) if n_rows != N else (16,))


def shape_cases():
    """Every N at n_rows = 1, 3, 4, 5, 15, 16, 17 (where N has that many) and N."""
    return [shape_case(N, r) for N in SHAPE_N for r in sorted({r for r in SHAPE_ROWS if r <= N} | {N})]


@functools.lru_cache(maxsize=None)
def single_start_case(start):
    """N = 1: the row looks at itself (start 0) or at nothing (start 1)."""
    return MatchCase("shape-1-start-%d" % start, shape_sig(1), [start], 1, SHAPE_FRAC,
                     {0: ([0], [0], [0], 1) if start == 0 else ([], [], [], 0)}, Ks=(1, 16))


# ------------------------------------------------------------------------------- counts

def match_cases():
    """{group: [MatchCase]} of the groups B to F."""
    return {
        "B": [roll_case(S) for S in ALL_S],
        "C": [tie_case(*t) for t in TIES],
        "D": [boundary_pairs_case(), gate_only_case(), plus_one_case()] + [full_empty_case(f) for f in FULL_EMPTY_FRACS]
             + [wrap_case(name) for name in WRAP_PAIRS],
        "E": [placed_case(name) for name in PLACED],
        "F": shape_cases() + [single_start_case(0), single_start_case(1)],
    }
