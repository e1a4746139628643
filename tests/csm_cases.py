"""Hand-placed inputs for the correlative scan matcher (no GPU; no randomness
but the seeded fills named below).

csrc/csm_kernels.hip treats a query cell differently by where it lies against
the clamp ``[hx - nx, G + hx]`` and the zero border, a shift by the slot, pass
and wave that own it (which of the 8 + 16 ``csm_score_kernel<R, W>`` the window
selects), a dword gather by the columns it reads past the window, a score by
whether it fits the packed 16-bit accumulators, and a point by the cell its
three-rounding ``(c x - s y) + tx0`` falls in.  The cases here put inputs on
those positions by hand:

* the reach, overhang, raster, boundary, saturation and tie cases use one or a
  few points on cell centres of a 16-cell grid of width 1 (every product and
  sum exact) and carry their expected volumes or best bins as literals;
* the boundary cases put a coordinate on a cell edge, one ulp to either side
  and on ``-0.0``; the cell each value falls in is a literal;
* the contraction cases come from a seeded search (``contraction_points``) for
  points whose cell differs between the three-rounding evaluation and one with
  either product kept exact; tests/test_csm_cases.py proves each with
  ``fractions.Fraction``;
* ``sweep_windows`` lists windows for which ``host_shape`` (the dispatch rule
  of ``slam_csm_batch``, restated) selects every R of both gather widths with
  no idle slot and with all but one slot of the last group idle, windows of two
  and three passes, and the default 61 x 61 window;
* every case is built once per process; its restatement result (``Case.ref``)
  is computed once and shared read-only.

tests/test_csm_cases.py checks these inputs on the CPU;
tests/test_csm_paths_gpu.py runs them on the GPU.
"""
import functools
from fractions import Fraction

import numpy as np

import csm_ref

BLOCK = 256                 # kCsmBlock: threads per workgroup, slots per register group
MAX_R = {1: 16, 4: 8}       # kCsmMaxR, kCsmMaxR4: slots per thread and pass by gather width
TILE = 4096                 # kCsmTile: query cells per LDS tile
WIDTHS = (4, 1)


def _ro(a):
    a.setflags(write=False)
    return a


class Case:
    """B pairs (query ``src[b]`` against reference ``dst[b]``, centre
    ``centre[b]``) over shared scans with one set of parameters: one launch.
    ``expect`` (B, n_theta, ny, nx), ``expect_index`` (B, 3) and
    ``expect_score`` (B,) are hand-written where given."""

    def __init__(self, name, scans, src, dst, params, centre=None, expect=None, expect_index=None, expect_score=None,
                 labels=None):
        self.name = name
        self.scans = [_ro(np.array(s, np.float64).reshape(-1, 2)) for s in scans]
        self.src, self.dst = _ro(np.array(src, np.int32)), _ro(np.array(dst, np.int32))
        B = len(self.src)
        self.centre = _ro(np.zeros((B, 3)) if centre is None else np.array(centre, np.float64).reshape(B, 3))
        self.params = dict(params)
        p = self.params
        self.shape = (B, p["n_theta"], p["ny"], p["nx"])
        self.expect = None if expect is None else _ro(np.array(expect, np.int32).reshape(self.shape))
        self.expect_index = None if expect_index is None else _ro(np.array(expect_index, np.int32).reshape(B, 3))
        self.expect_score = None if expect_score is None else _ro(np.array(expect_score, np.int32).reshape(B))
        self.labels = list(labels) if labels is not None else ["pair%d" % b for b in range(B)]
        assert len(self.labels) == B and len(self.dst) == B

    def pair(self, b):
        """(query, reference, centre) of pair b."""
        return self.scans[self.src[b]], self.scans[self.dst[b]], self.centre[b]

    @functools.cached_property
    def ref(self):
        """(volumes (B, n_theta, ny, nx) int32, index (B, 3), score (B,), tf (B, 3, 3)) of the restatement."""
        p = self.params
        vols, index, score, tf = [], [], [], []
        for b in range(len(self.src)):
            q, r, c = self.pair(b)
            S, cs = csm_ref.score_volume(q, r, c, **p)
            s, idx = csm_ref.best(S)
            vols.append(S)
            index.append(idx)
            score.append(s)
            tf.append(csm_ref.transform(cs, idx, c, p["res"], p["nx"], p["ny"]))
        return (_ro(np.stack(vols)), _ro(np.array(index, np.int32)), _ro(np.array(score, np.int32)),
                _ro(np.stack(tf)))

    def packed(self):
        """(pts (P, 2), off (S + 1,)) as ``slamhip.plicp.packed_scans`` takes them."""
        off = np.concatenate([[0], np.cumsum([len(s) for s in self.scans])]).astype(np.int64)
        return np.concatenate(self.scans + [np.zeros((0, 2))]), off


# -------------------------------------------------- the 16-cell grid of width 1

G16 = 16
UNIT = dict(res=1.0, G=G16, n_theta=1, d_theta=0.0)


def at(cx, cy, G=G16, res=1.0):
    """The centre of cell (cx, cy): exact for res = 1 and the dyadic widths."""
    o = csm_ref.origin(G, res)
    return (o + (cx + 0.5) * res, o + (cy + 0.5) * res)


def _swap(scans):
    return [[(y, x) for x, y in s] for s in scans]


# ------------------------------------------------------- window reach at the grid's edge

# one reference point in cell 0 (low) or G - 1 (high), one query point in the last cell from
# which a shift still reaches it; the row over the window's shifts
REACH_ROWS = {7: {"low": [0, 0, 0, 0, 0, 0, 2], "high": [2, 0, 0, 0, 0, 0, 0]},
              8: {"low": [0, 0, 0, 0, 0, 0, 0, 2], "high": [2, 0, 0, 0, 0, 0, 0, 0]},
              5: {"low": [0, 0, 0, 0, 2], "high": [2, 0, 0, 0, 0]},
              6: {"low": [0, 0, 0, 0, 0, 2], "high": [2, 0, 0, 0, 0, 0]}}
# the query cells: (low reach, low miss, high reach, high miss) = (-(n - 1 - h), that - 1, G - 1 + h, that + 1)
REACH_CELLS = {7: (-3, -4, 18, 19), 8: (-3, -4, 19, 20), 5: (-2, -3, 17, 18), 6: (-2, -3, 18, 19)}
FAR = 10 ** 6               # cells: the clamp proper
REACH_1D = ((7, "x"), (8, "x"), (5, "y"), (6, "y"))


@functools.lru_cache(maxsize=None)
def reach_case(n, axis):
    """Window of n shifts along ``axis`` and 1 along the other; the other coordinate in cell 5."""
    lo_hit, lo_miss, hi_hit, hi_miss = REACH_CELLS[n]
    scans = [[at(0, 5)], [at(G16 - 1, 5)], [at(lo_hit, 5)], [at(lo_miss, 5)], [at(hi_hit, 5)], [at(hi_miss, 5)],
             [at(FAR, 5)], [at(-FAR, 5)]]
    zero = [0] * n
    rows = REACH_ROWS[n]
    pairs = [("low reach", 2, 0, rows["low"]), ("low miss", 3, 0, zero), ("high reach", 4, 1, rows["high"]),
             ("high miss", 5, 1, zero), ("low reach again", 2, 0, rows["low"]), ("far high", 6, 1, zero),
             ("far low", 7, 0, zero), ("high reach again", 4, 1, rows["high"])]
    nx, ny = (n, 1) if axis == "x" else (1, n)
    return Case("reach-%s%d" % (axis, n), scans if axis == "x" else _swap(scans), [p[1] for p in pairs],
                [p[2] for p in pairs], dict(UNIT, nx=nx, ny=ny), expect=[p[3] for p in pairs],
                labels=[p[0] for p in pairs])


# (nx, ny) -> corner (x side, y side) -> (j, i) of the one shift that reaches
CORNER_AT = {(7, 5): {("low", "low"): (4, 6), ("high", "low"): (4, 0), ("low", "high"): (0, 6),
                      ("high", "high"): (0, 0)},
             (8, 6): {("low", "low"): (5, 7), ("high", "low"): (5, 0), ("low", "high"): (0, 7),
                      ("high", "high"): (0, 0)}}


@functools.lru_cache(maxsize=None)
def corner_case(nx, ny):
    """The reference in a corner cell of the grid, the query in the one cell from which a single
    shift of the 2-D window reaches it, then one cell beyond in x only and in y only."""
    scans, src, dst, expect, labels = [], [], [], [], []
    xs, ys = REACH_CELLS[nx], REACH_CELLS[ny]
    for (sx, sy), (j, i) in CORNER_AT[(nx, ny)].items():
        rx, qx, mx = (0, xs[0], xs[1]) if sx == "low" else (G16 - 1, xs[2], xs[3])
        ry, qy, my = (0, ys[0], ys[1]) if sy == "low" else (G16 - 1, ys[2], ys[3])
        r = len(scans)
        scans += [[at(rx, ry)], [at(qx, qy)], [at(mx, qy)], [at(qx, my)]]
        hit = np.zeros((ny, nx), np.int32)
        hit[j, i] = 2
        for q, e, what in ((r + 1, hit, "reach"), (r + 2, 0 * hit, "miss x"), (r + 3, 0 * hit, "miss y")):
            src.append(q)
            dst.append(r)
            expect.append(e)
            labels.append("%s-%s %s" % (sx, sy, what))
    return Case("corner-%dx%d" % (nx, ny), scans, src, dst, dict(UNIT, nx=nx, ny=ny), expect=expect, labels=labels)


# ------------------------------------------------------------------------------ overhang

OVERHANG_NX = (1, 2, 3, 5, 6, 7)
# the window row of a query whose last column lies just left of an occupied cell
OVERHANG_ROWS = {1: [1], 2: [0, 1], 3: [0, 0, 1], 5: [0, 0, 0, 0, 1], 6: [0, 0, 0, 0, 0, 1], 7: [0, 0, 0, 0, 0, 0, 1]}


@functools.lru_cache(maxsize=None)
def overhang_case(nx):
    """ny = 3, the query in cell (8, 8): the window's last column reads cell ``last``; the
    reference occupies the cells right of it, where the dword of the row's last slot reads on."""
    hx = nx // 2
    last = 8 + (nx - 1 - hx)
    edge = G16 - 1 - (nx - 1 - hx)       # the query cell whose last column is the grid's last cell
    scans = [[at(8, 8)], [at(last + 1, 8)], [at(last + 1, 8), at(last + 2, 8), at(last + 3, 8)],
             [at(G16 + hx, 8)], [at(G16 + nx, 8), at(0, 9)], [at(edge, 8)], [at(G16, 8)]]
    row = OVERHANG_ROWS[nx]
    one, zero = [row] * 3, [[0] * nx] * 3
    pairs = [("one cell right", 0, 1, one), ("three cells right", 0, 2, one), ("right clamp", 3, 4, zero),
             ("grid's last cell", 5, 6, one), ("one cell right again", 0, 1, one)]
    return Case("overhang-%d" % nx, scans, [p[1] for p in pairs], [p[2] for p in pairs], dict(UNIT, nx=nx, ny=3),
                expect=[p[3] for p in pairs], expect_index=[(0, 0, nx - 1), (0, 0, nx - 1), (0, 0, 0), (0, 0, nx - 1),
                                                            (0, 0, nx - 1)],
                expect_score=[1, 1, 0, 1, 1], labels=[p[0] for p in pairs])


# --------------------------------------------------------------------------- raster order

PAIR_OF_2 = [[0, 1, 1, 1, 1], [0, 1, 2, 2, 1], [0, 1, 1, 1, 1]]
ONE_POINT = [[0, 1, 1, 1, 0], [0, 1, 2, 1, 0], [0, 1, 1, 1, 0]]
EDGE_ONLY = [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]
NOTHING = [[0, 0, 0, 0, 0]] * 3
N_DUP = 600                # more than a workgroup's threads


@functools.lru_cache(maxsize=None)
def raster_case():
    """A 5 x 3 window around the query cell (8, 8), (0, 8) or (15, 8)."""
    far = (1e12, -1e12)
    scans = [[at(8, 8)], [at(0, 8)], [at(G16 - 1, 8)],
             [at(8, 8), at(9, 8)], [at(9, 8), at(8, 8)], [at(8, 8)] * N_DUP, [at(8, 8), at(9, 8)] * (N_DUP // 2),
             [at(-1, 8), at(G16, 8)], [at(8, 8), far], [far]]
    pairs = [("adjacent", 0, 3, PAIR_OF_2), ("adjacent swapped", 0, 4, PAIR_OF_2), ("600 duplicates", 0, 5, ONE_POINT),
             ("300 + 300 duplicates", 0, 6, PAIR_OF_2), ("cell -1", 1, 7, EDGE_ONLY), ("cell G", 2, 7, EDGE_ONLY),
             ("far reference alone", 0, 9, NOTHING), ("far reference beside a point", 0, 8, ONE_POINT)]
    return Case("raster", scans, [p[1] for p in pairs], [p[2] for p in pairs], dict(UNIT, nx=5, ny=3),
                expect=[p[3] for p in pairs], labels=[p[0] for p in pairs])


# ------------------------------------------------------------------------ cell boundaries

BOUNDARY_K = (0, G16 // 2, G16 - 1)
DYADIC = 0.125
# the cell of the value named, by the definition's two roundings floor((v - o) / res), o = -1:
#   k = 0   v = -1:     below is -1 - 2^-52, v - o = -2^-52 exactly: cell -1
#   k = 8   v = 0:      the subnormals on either side vanish in v + 1 = 1: cell 8, as does -0.0;
#                       -2^-53 is the first value whose sum 1 - 2^-53 stays below 1: cell 7
#   k = 15  v = 0.875:  0.875 - 2^-53 + 1 lies halfway and rounds to even, 1.875: cell 15;
#                       0.875 - 2^-52 gives 1.875 - 2^-52 exactly: cell 14
DYADIC_CELLS = {0: {"exact": 0, "below": -1, "above": 0},
                8: {"exact": 8, "below": 8, "above": 8, "-0.0": 8, "first below": 7},
                15: {"exact": 15, "below": 15, "above": 15, "first below": 14}}
DYADIC_EXTRA = {8: {"-0.0": -0.0, "first below": -2.0 ** -53}, 15: {"first below": 0.875 - 2.0 ** -52}}
# res = 0.05, o = -8 * 0.05 = -0.4, the boundary o + k * 0.05 as floating point gives it: 0.35 for
# k = 15, whose lower neighbour plus 0.4 rounds to the boundary's own sum and stays in cell 15
DEFAULT_CELLS = {0: {"exact": 0, "below": -1, "above": 0},
                 8: {"exact": 8, "below": 8, "above": 8},
                 15: {"exact": 15, "below": 15, "above": 15}}


def boundary_values(res, k):
    """{name: coordinate} around the lower edge of cell k of the 16-cell grid."""
    o = csm_ref.origin(G16, res)
    v = o + k * res
    out = {"exact": v, "below": float(np.nextafter(v, -np.inf)), "above": float(np.nextafter(v, np.inf))}
    if res == DYADIC:
        out.update(DYADIC_EXTRA.get(k, {}))
    return out


def row3(query_cell, ref_cell, G=G16):
    """The 3-shift row of one query point against one reference point, both by their cells,
    along one axis: 2 on the reference's cell, 1 beside it, 0 elsewhere and outside the grid."""
    out = []
    for c in (query_cell - 1, query_cell, query_cell + 1):
        d = abs(c - ref_cell)
        out.append(0 if not 0 <= c < G else 2 if d == 0 and 0 <= ref_cell < G else 1 if d == 1 else 0)
    return out


@functools.lru_cache(maxsize=None)
def boundary_case(res, axis):
    """Each boundary value as the query against a reference in the middle of cell k, and as the
    reference against a query there; the other coordinate in the middle of cell 8."""
    cells = DYADIC_CELLS if res == DYADIC else DEFAULT_CELLS
    mid = at(8, 8, G16, res)[1]
    scans, src, dst, expect, labels = [], [], [], [], []
    for k in BOUNDARY_K:
        centre = len(scans)
        scans.append([(at(k, 8, G16, res)[0], mid)])
        for name, v in boundary_values(res, k).items():
            scans.append([(v, mid)])
            cv = cells[k][name]
            for q, r, row in ((len(scans) - 1, centre, row3(cv, k)), (centre, len(scans) - 1, row3(k, cv))):
                src.append(q)
                dst.append(r)
                expect.append(row)
                labels.append("k=%d %s as %s" % (k, name, "query" if r == centre else "reference"))
    nx, ny = (3, 1) if axis == "x" else (1, 3)
    return Case("boundary-%g-%s" % (res, axis), scans if axis == "x" else _swap(scans), src, dst,
                dict(res=res, G=G16, n_theta=1, d_theta=0.0, nx=nx, ny=ny), expect=expect, labels=labels)


BOUNDARY_CASES = ((DYADIC, "x"), (DYADIC, "y"), (0.05, "x"), (0.05, "y"))


# --------------------------------------------------------------- contraction-sensitive points

def fl(q):
    """The double nearest the rational q (int / int division rounds correctly, ties to even)."""
    return float(Fraction(q))


def three_roundings(a, x, b, y, t, sign):
    """(a x) + sign (b y), each product and the sum rounded, then + t: the definition's X or Y."""
    return (a * x + sign * (b * y)) + t


def contracted(a, x, b, y, t, sign):
    """The two FMA forms of the same expression: the first product kept exact, the second one."""
    F = Fraction
    first = fl(F(a) * F(x) + F(sign * (b * y)))
    second = fl(F(a * x) + F(sign) * F(b) * F(y))
    return first + t, second + t


def cell_of(v, res=DYADIC, G=G16):
    return int(np.floor((v - csm_ref.origin(G, res)) / res))


N_CONTRACT = 6              # per coordinate


@functools.lru_cache(maxsize=None)
def contraction_points():
    """12 tuples (theta, x, y, tx0, ty0, coordinate, cell (cx, cy), contracted cells): a seeded
    search over random angles for points within a few ulps of a cell edge whose three-rounding X
    (the first 6) or Y (the last 6) lies in another cell than an FMA form of it; of each
    coordinate's 6 at least 3 are moved by either form."""
    rng = np.random.default_rng(20091)
    found = {"X": [], "Y": []}
    short = {"X": [N_CONTRACT // 2] * 2, "Y": [N_CONTRACT // 2] * 2}    # points still wanted per FMA form
    for _ in range(200000):
        if all(len(v) == N_CONTRACT for v in found.values()):
            break
        th = float(rng.uniform(-3.0, 3.0))
        c, s = float(np.cos(th)), float(np.sin(th))
        coord = "X" if len(found["X"]) < N_CONTRACT and len(found["X"]) <= len(found["Y"]) else "Y"
        lead = c if coord == "X" else s
        if abs(lead) < 0.3:
            continue
        m = int(rng.integers(3, 13))
        t = float(rng.uniform(-0.2, 0.2))
        other_t = float(rng.uniform(-0.05, 0.05))
        y = float(rng.uniform(-0.4, 0.4))
        edge = csm_ref.origin(G16, DYADIC) + m * DYADIC
        # X = (c x - s y) + tx0 or Y = (s x + c y) + ty0 on the edge: solve for x, then walk its ulps
        x0 = ((edge - t) + s * y) / c if coord == "X" else ((edge - t) - c * y) / s
        if abs(x0) > 0.9:
            continue
        x = x0
        for _ in range(4):
            x = float(np.nextafter(x, -np.inf))
        for _ in range(9):
            args = (c, x, s, y, t, -1.0) if coord == "X" else (s, x, c, y, t, 1.0)
            plain = cell_of(three_roundings(*args))
            forms = tuple(cell_of(v) for v in contracted(*args))
            wanted = [n for n in (0, 1) if forms[n] != plain and short[coord][n] > 0]
            if wanted:
                X = three_roundings(c, x, s, y, t if coord == "X" else other_t, -1.0)
                Y = three_roundings(s, x, c, y, t if coord == "Y" else other_t, 1.0)
                cx, cy = cell_of(X), cell_of(Y)
                if 1 <= cx < G16 - 1 and 1 <= cy < G16 - 1:
                    tx0, ty0 = (t, other_t) if coord == "X" else (other_t, t)
                    found[coord].append((th, x, y, tx0, ty0, coord, (cx, cy), forms))
                    short[coord][wanted[0]] -= 1
                    break
            x = float(np.nextafter(x, np.inf))
    assert all(len(v) == N_CONTRACT for v in found.values()), {k: len(v) for k, v in found.items()}
    return tuple(found["X"] + found["Y"])


CONTRACT_VOLUME = [[1, 1, 1], [1, 2, 1], [1, 1, 1]]


@functools.lru_cache(maxsize=None)
def contraction_case():
    """One pair per point: the query is the point, the centre its (theta, tx0, ty0), the
    reference the middle of the cell of the three-rounding result: a 3 x 3 window scores 2 in
    its centre, and 1 there if either coordinate lands one cell off."""
    pts = contraction_points()
    scans, src, dst, centre = [], [], [], []
    for th, x, y, tx0, ty0, _, (cx, cy), _ in pts:
        scans += [[(x, y)], [at(cx, cy, G16, DYADIC)]]
        src.append(len(scans) - 2)
        dst.append(len(scans) - 1)
        centre.append((th, tx0, ty0))
    n = len(pts)
    return Case("contraction", scans, src, dst, dict(res=DYADIC, G=G16, n_theta=1, d_theta=0.0, nx=3, ny=3),
                centre=centre, expect=[CONTRACT_VOLUME] * n, expect_index=[(0, 1, 1)] * n, expect_score=[2] * n,
                labels=["%s %d" % (p[5], k) for k, p in enumerate(pts)])


# ----------------------------------------------------------------------------- saturation

SATURATION_N = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 40000)
# reference cells (0, 6) and (5, 10); an 8 x 5 window (two dwords per row) around the query cell
# (3, 8), which reads the columns -1..6, and around (4, 8), which reads 0..7.  The first dwords
# of row 0 are [0, 2, 1, 0] and [2, 1, 0, 0]: the 2 shares its 16-bit pair with a 0, the 1 too
SATURATION_ONE = {3: [[0, 2, 1, 0, 0, 0, 0, 0],
                      [0, 1, 1, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 1, 1, 1],
                      [0, 0, 0, 0, 0, 1, 2, 1]],
                  4: [[2, 1, 0, 0, 0, 0, 0, 0],
                      [1, 1, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 1, 1, 1, 0],
                      [0, 0, 0, 0, 1, 2, 1, 0]]}
SATURATION_BEST = {3: (0, 0, 1), 4: (0, 0, 0)}


@functools.lru_cache(maxsize=None)
def saturation_case():
    """n copies of one query point for every n of SATURATION_N and both query cells: n times
    the one-point volume, up to 80,000 > 2^16 in a cell whose pair partner holds 0."""
    scans = [[at(0, 6), at(5, 10)]]
    src, expect, index, score, labels = [], [], [], [], []
    for n in SATURATION_N:
        for qx in (3, 4):
            scans.append([at(qx, 8)] * n)
            src.append(len(scans) - 1)
            expect.append(n * np.array(SATURATION_ONE[qx], np.int64))
            index.append(SATURATION_BEST[qx])
            score.append(2 * n)
            labels.append("n=%d cell %d" % (n, qx))
    return Case("saturation", scans, src, [0] * len(src), dict(UNIT, nx=8, ny=5), expect=expect, expect_index=index,
                expect_score=score, labels=labels)


# ----------------------------------------------------------------------------------- ties

@functools.lru_cache(maxsize=None)
def tie_small_case():
    """One query point in cell (8, 8), a 7 x 5 window (reads columns 5..11, rows 6..10), two
    reference points that two shifts reach: the smaller flat index wins."""
    scans = [[at(8, 8)], [at(6, 8), at(10, 8)], [at(8, 6), at(8, 10)], [at(10, 7), at(6, 9)]]
    return Case("tie-small", scans, [0, 0, 0], [1, 2, 3], dict(UNIT, nx=7, ny=5),
                expect_index=[(0, 2, 1), (0, 0, 3), (0, 1, 5)], expect_score=[2, 2, 2],
                labels=["two columns", "two rows", "later row, earlier column"])


@functools.lru_cache(maxsize=None)
def tie_angle_case():
    """Angles -pi, 0, pi: the query (2.5, 1.5) lands in the cell of (-2.5, -1.5) at the first
    and at the last angle, which other workgroups score: angle 0 wins."""
    return Case("tie-angle", [[(2.5, 1.5)], [(-2.5, -1.5)]], [0], [1],
                dict(res=1.0, G=G16, n_theta=3, d_theta=float(np.pi), nx=3, ny=3),
                expect=[[[1, 1, 1], [1, 2, 1], [1, 1, 1]], [[0] * 3] * 3, [[1, 1, 1], [1, 2, 1], [1, 1, 1]]],
                expect_index=[(0, 1, 1)], expect_score=[2], labels=["first and last angle"])


@functools.lru_cache(maxsize=None)
def tie_wave_case():
    """G = 64, a 32 x 16 window around the query cell (32, 32): 512 shifts, which byte gathers
    spread as flat % 256 over the threads (two slots each) and dword gathers as flat // 4 (one
    slot each).  Pair 0: maxima at flat 35 = (1, 3) and 327 = (10, 7): threads 35 and 71 (bytes),
    8 and 81 (dwords), waves 0 and 1.  Pair 1: maxima at flat 100 = (3, 4) and 300 = (9, 12):
    threads 100 and 44 (bytes; the larger index in the earlier wave), 25 and 75 (dwords)."""
    def ref(j, i):
        return at(32 + i - 16, 32 + j - 8, 64)
    scans = [[at(32, 32, 64)], [ref(1, 3), ref(10, 7)], [ref(9, 12), ref(3, 4)]]
    return Case("tie-wave", scans, [0, 0], [1, 2], dict(res=1.0, G=64, n_theta=1, d_theta=0.0, nx=32, ny=16),
                expect_index=[(0, 1, 3), (0, 3, 4)], expect_score=[2, 2], labels=["waves 0, 1", "waves 1, 0"])


@functools.lru_cache(maxsize=None)
def tie_pass_case():
    """G = 1200, an 8 x 1100 window around the query cell (600, 600): 8,800 shifts in three passes
    of byte gathers (R = 12) and 2,200 slots in two passes of dword gathers (R = 5).  Maxima in
    row 2 (the first pass) and row 1097 (the last): (2, 5) wins over (1097, 1)."""
    G = 1200
    scans = [[at(600, 600, G)], [at(600 + 1 - 4, 600 + 1097 - 550, G), at(600 + 5 - 4, 600 + 2 - 550, G)]]
    return Case("tie-pass", scans, [0], [1], dict(res=1.0, G=G, n_theta=1, d_theta=0.0, nx=8, ny=1100),
                expect_index=[(0, 2, 5)], expect_score=[2], labels=["first and last pass"])


# ---------------------------------------------------------------------------- empty scans

EMPTY_PARAMS = dict(res=0.1, G=64, n_theta=3, d_theta=0.2, nx=6, ny=5)
# pair -> what it is; scan 1 and scan 3 hold no point
EMPTY_PAIRS = (("ordinary", 0, 2), ("empty query", 1, 2), ("ordinary", 4, 0), ("empty reference", 0, 3),
               ("ordinary", 2, 4), ("both empty", 1, 3), ("scan against itself", 2, 2), ("ordinary", 4, 2))


@functools.lru_cache(maxsize=None)
def empty_case():
    """Five scans, the second and the fourth empty (``plicp.packed_scans`` takes such a set)."""
    rng = np.random.default_rng(5)
    base = rng.uniform(-2.5, 2.5, size=(40, 2))
    scans = [base[:25], np.zeros((0, 2)), base[10:40] + (0.12, -0.07), np.zeros((0, 2)), base[5:30] - (0.2, 0.1)]
    centre = [(0.1 * (b % 3 - 1), 0.05 * b, -0.03 * b) for b in range(len(EMPTY_PAIRS))]
    return Case("empty", scans, [p[1] for p in EMPTY_PAIRS], [p[2] for p in EMPTY_PAIRS], EMPTY_PARAMS, centre=centre,
                labels=[p[0] for p in EMPTY_PAIRS])


# ------------------------------------------------------------------------- instance sweep

def host_shape(nx, ny, width):
    """(nslot, passes, R) slam_csm_batch picks: slots of ``width`` shifts of one window row,
    passes of at most 256 * maxR slots, the slots spread evenly over the passes."""
    nslot = ny * -(-nx // width)
    passes = -(-nslot // (BLOCK * MAX_R[width]))
    return nslot, passes, -(-nslot // (BLOCK * passes))


def fill_level(nslot, passes, R):
    """"full": no idle slot; "barely": the last of the R groups of 256 holds one slot."""
    if passes != 1:
        return None
    return "full" if nslot == BLOCK * R else "barely" if nslot == BLOCK * (R - 1) + 1 else None


DEFAULT_WINDOW = (61, 61)
MULTI_PASS = ((50, 100), (64, 150), (64, 260), (8, 1100))


def sweep_windows():
    """(nx, ny) of every window of the sweep."""
    tall = [(1, ny) for R in range(1, 17) for ny in (BLOCK * (R - 1) + 1, BLOCK * R)]
    five = [(5, ny) for R in range(1, 9) for ny in (128 * (R - 1) + 1, 128 * R)]
    return tuple(tall + five + list(MULTI_PASS[:3]) + [DEFAULT_WINDOW])


def sweep_coverage():
    """{(width, R, fill level)} of the single-pass windows and {(width, passes)} of the others."""
    single, multi = set(), set()
    for nx, ny in sweep_windows() + MULTI_PASS[3:]:
        for w in WIDTHS:
            nslot, passes, R = host_shape(nx, ny, w)
            if passes == 1:
                if fill_level(nslot, passes, R):
                    single.add((w, R, fill_level(nslot, passes, R)))
            else:
                multi.add((w, passes))
    return single, multi


_single, _multi = sweep_coverage()
assert _single >= {(w, R, f) for w in WIDTHS for R in range(1, MAX_R[w] + 1) for f in ("full", "barely")}, _single
assert _multi >= {(w, p) for w in WIDTHS for p in (2, 3)}, _multi
assert host_shape(*DEFAULT_WINDOW, 4)[1:] == (1, 4) and host_shape(*DEFAULT_WINDOW, 1)[1:] == (1, 15)


def slot_rows(nx, ny, width, group):
    """The window rows of the first (group 0) or last (group -1) 256 slots of the launch."""
    row_slots = -(-nx // width)
    nslot = ny * row_slots
    lo, hi = (0, min(BLOCK, nslot)) if group == 0 else ((nslot - 1) // BLOCK * BLOCK, nslot)
    return lo // row_slots, (hi - 1) // row_slots


@functools.lru_cache(maxsize=None)
def sweep_case(nx, ny):
    """Two pairs for one window.  The default window: G = 512, res = 0.05, 8 angles, queries of
    200 points cut from references of 300.  Every other one: G just above ny, res = 0.1, two
    angles 0.4 / G apart, queries of 120 and 150 points and references of 200 and 260, uniform
    over the grid's height (3 % beyond it) and over a strip of nx + 2 cells (the whole width for
    nx >= 50), so that shifts of half the window's height still meet occupied cells."""
    rng = np.random.default_rng(1000 * nx + ny)
    if (nx, ny) == DEFAULT_WINDOW:
        refs = [rng.uniform(-10.0, 10.0, size=(300, 2)) for _ in range(2)]
        th = (0.07, -0.05)
        qs = []
        for r, a in zip(refs, th):
            p = r[rng.permutation(300)[:200]] + rng.normal(0, 0.02, size=(200, 2)) - (0.35, -0.4)
            qs.append(p @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]))
        params = dict(res=0.05, G=512, n_theta=8, d_theta=2 * np.pi / 240, nx=nx, ny=ny)
        return Case("sweep-default", qs + refs, [0, 1], [2, 3], params, centre=[(0.05, 0.1, -0.1), (-0.02, 0.3, -0.45)])
    G = max(32, ny + 16 + ny % 2)
    res = 0.1
    half = 0.5 * G * res
    wide = half * 1.03 if nx >= 50 else 0.5 * (nx + 2) * res

    def pts(n):
        return np.stack([rng.uniform(-wide, wide, n), rng.uniform(-1.03 * half, 1.03 * half, n)], axis=1)
    scans = [pts(120), pts(150), pts(200), pts(260)]
    params = dict(res=res, G=G, n_theta=2, d_theta=0.4 / G, nx=nx, ny=ny)
    return Case("sweep-%dx%d" % (nx, ny), scans, [0, 1], [2, 3], params,
                centre=[(0.0, 0.03, -0.02), (0.0, -0.04, 0.05)])


# ---------------------------------------------------------------------- grid decomposition

@functools.lru_cache(maxsize=None)
def grid_case():
    """B = 3 pairs, the production count of 240 angles, a 3 x 3 window: 720 workgroups."""
    rng = np.random.default_rng(11)
    ref = rng.uniform(-2.5, 2.5, size=(70, 2))
    scans = [ref[:50] + (0.05, -0.1), ref[20:70] - (0.1, 0.02), ref, ref[::-1][:45] * (1.0, -1.0)]
    return Case("grid", scans, [0, 1, 3], [2, 2, 0],
                dict(res=0.1, G=64, n_theta=240, d_theta=2 * np.pi / 240, nx=3, ny=3), centre=[(0.3, 0.1, -0.1), (-1.0, 0.0, 0.2), (2.0, -0.1, 0.0)])


def hand_cases():
    """Every case but the sweep's: small enough for the plain loops of tests/test_csm_cases.py."""
    out = [reach_case(n, axis) for n, axis in REACH_1D] + [corner_case(7, 5), corner_case(8, 6)]
    out += [overhang_case(nx) for nx in OVERHANG_NX] + [raster_case()]
    out += [boundary_case(res, axis) for res, axis in BOUNDARY_CASES]
    out += [contraction_case(), saturation_case(), tie_small_case(), tie_angle_case(), tie_wave_case(),
            tie_pass_case(), empty_case(), grid_case()]
    return out
