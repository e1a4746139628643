"""Hand-placed inputs for the localisation in a finished occupancy grid (no GPU;
no randomness but the seeded fills named below).

csrc/loc_kernels.hip treats a cell differently by the 128-row band and the
256-column block it lies in, a search by the window's size (which of the eight
``loc_search_kernel<R, T>`` it selects, how many passes), the table's entry width
and size and the scan's length against the LDS tile, and a refinement point by
the bilinear cell it falls in, the field's cap and the three pivots of the 3 x 3
solve.  The cases here put inputs on those positions by hand:

* the single-cell fields (``band_cells``, ``block_cells``) have the closed form
  ``min(d_cap^2, dr^2 + dc^2)``;
* ``search_host_shape`` restates the host's choice of (passes, R);
* the refinement cases that must land exactly on an edge use headings of
  exactly 0 (cos = 1, sin = 0), a cell width of 0.25 and coordinates that are
  short binary fractions, so ``u``, ``v`` and the cell they fall in are exact
  under every rounding order (tests/test_loc_cases.py proves it with
  ``fractions.Fraction``);
* every case is built once per process; its restatement result
  (``loc_ref.field`` / ``search`` / ``refine``) is computed once and shared
  read-only.

tests/test_loc_cases.py checks these inputs on the CPU;
tests/test_loc_paths_gpu.py runs them on the GPU.
"""
import functools

import numpy as np

import loc_ref

BAND = 128        # kLocBand: rows per thread of loc_col_kernel
BLOCK = 256       # kLocBlock: columns per workgroup of loc_row_kernel, threads everywhere
MAX_R = 8         # kLocMaxR: shifts per thread and pass
TILE = 4096       # kLocTile: query cells per LDS tile
TABLE_SWEEP = 4096 * BLOCK   # cells loc_table_kernel's launch covers before it strides
EDGE_CAPS = (1, 2, 20, 127, 128, 129)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def seeded_grid(H, W, seed, p=0.03):
    """tests/test_loc_gpu.py's ``_random``: unknown / free cells of every value, a share p occupied."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-128, 1, size=(H, W)).astype(np.int8)
    g[rng.random((H, W)) < p] = rng.integers(1, 128)
    return g


# ------------------------------------------------------------------------------ field

class FieldCase:
    def __init__(self, name, grid, d_cap, cell=None):
        self.name, self.grid, self.d_cap, self.cell = name, _ro(np.asarray(grid, np.int8)), d_cap, cell

    @functools.cached_property
    def ref(self):
        return _ro(loc_ref.field(self.grid, self.d_cap))

    def closed_form(self):
        """One occupied cell (r0, c0): min(d_cap^2, dr^2 + dc^2), written out."""
        r0, c0 = self.cell
        H, W = self.grid.shape
        r, c = np.mgrid[0:H, 0:W]
        return np.minimum(self.d_cap ** 2, (r - r0) ** 2 + (c - c0) ** 2).astype(np.uint16)


def _single(name, H, W, r, c, d_cap):
    g = np.zeros((H, W), np.int8)
    g[r, c] = 1
    return FieldCase(name, g, d_cap, (r, c))


SHAPES = tuple((H, 3) for H in (127, 128, 129, 256, 257)) + tuple((3, W) for W in (255, 256, 257, 511, 513))
SHAPE_CAP = 5


@functools.lru_cache(maxsize=None)
def shape_cases():
    """Grids one short of, at and one past one and two bands / column blocks: a seeded fill."""
    return tuple(FieldCase("shape-%dx%d" % (H, W), seeded_grid(H, W, 100 + H + W, p=0.04), SHAPE_CAP)
                 for H, W in SHAPES)


BAND_H, BAND_W = 300, 3        # bands 0..127, 128..255, 256..299
BLOCK_H, BLOCK_W = 3, 520      # blocks 0..255, 256..511, 512..519


def edge_positions(n, edges, d_cap):
    """0, n - 1, the two cells on either side of every edge e (e - 1, e) and the
    cells d_cap - 1, d_cap and d_cap + 1 away from either of those, inside [0, n)."""
    out = {0, n - 1}
    for e in edges:
        for k in (0, d_cap - 1, d_cap, d_cap + 1):
            out |= {e - 1 - k, e - k, e - 1 + k, e + k}
    return tuple(sorted(p for p in out if 0 <= p < n))


@functools.lru_cache(maxsize=None)
def band_cells(d_cap):
    """One occupied cell of a 300 x 3 grid at a time, in column 1, on every row that
    edge_positions names for the band edges 128 and 256."""
    return tuple(_single("band-cap%d-row%d" % (d_cap, r), BAND_H, BAND_W, r, 1, d_cap)
                 for r in edge_positions(BAND_H, (BAND, 2 * BAND), d_cap))


@functools.lru_cache(maxsize=None)
def block_cells(d_cap):
    """The same for the column-block edges 256 and 512 of a 3 x 520 grid, in row 1."""
    return tuple(_single("block-cap%d-col%d" % (d_cap, c), BLOCK_H, BLOCK_W, 1, c, d_cap)
                 for c in edge_positions(BLOCK_W, (BLOCK, 2 * BLOCK), d_cap))


HALO_COLS = (3, 300, 520, 700)    # 297 apart (above 255), 220 and 180 apart (below)


@functools.lru_cache(maxsize=None)
def halo_case():
    """d_cap = 255 on one row of 800 cells: block 1's halo of 2 x 255 entries covers
    the columns 1..766, over both neighbouring blocks."""
    g = np.zeros((1, 800), np.int8)
    g[0, list(HALO_COLS)] = 7
    return FieldCase("halo-255", g, 255)


# ----------------------------------------------------------------------------- search

def search_host_shape(nx, ny):
    """(passes, R) slam_loc_search picks: passes of at most 256 * 8 shifts, spread evenly."""
    nshift = nx * ny
    passes = -(-nshift // (BLOCK * MAX_R))
    return passes, -(-nshift // (BLOCK * passes))


class SearchCase:
    """B queries (scan idx[b], centre[b] = (theta0, x0, y0)) on one map with one window."""

    def __init__(self, name, grid, origin, cw, d_cap, scans, idx, centre, window):
        self.name, self.grid, self.cw, self.d_cap = name, _ro(grid), cw, d_cap
        self.origin = _ro(np.asarray(origin, float))
        self.scans = [_ro(np.asarray(s, np.float64).reshape(-1, 2)) for s in scans]
        self.idx, self.centre = _ro(np.asarray(idx, np.int64)), _ro(np.asarray(centre, np.float64).reshape(-1, 3))
        self.window = dict(window)

    @functools.cached_property
    def F(self):
        return _ro(loc_ref.field(self.grid, self.d_cap))

    @functools.cached_property
    def ref(self):
        """(costs (B, n_theta, ny, nx) int32, index (B, 3), cost (B,)) of the restatement."""
        out = [loc_ref.search(self.F, self.origin, self.cw, self.d_cap, self.scans[s], c, **self.window)
               for s, c in zip(self.idx, self.centre)]
        return _ro(np.stack([o[0] for o in out]), np.array([o[1][1:] for o in out]), np.array([o[1][0] for o in out]))

    def cells(self, b, k=None):
        """(cx, cy) of query b's points at angle bin k (the middle one by default)."""
        w = self.window
        rot = loc_ref.rotations(self.centre[b, 0], w["n_theta"], w["d_theta"])[w["n_theta"] // 2 if k is None else k]
        return loc_ref.cells(self.scans[self.idx[b]], rot[0], rot[1], self.centre[b, 1], self.centre[b, 2], self.origin,
                             self.cw)


SMALL_ORIGIN, SMALL_CW, SMALL_CAP = np.array([-5.3, -3.7]), 0.2, 6


@functools.lru_cache(maxsize=None)
def small_map():
    """tests/test_loc_gpu.py's 37 x 53 map of 0.2 m cells centred on the sensor."""
    return _ro(seeded_grid(37, 53, 7, p=0.06))


@functools.lru_cache(maxsize=None)
def scan61():
    from slamhip import synthetic
    s = synthetic.make_sequence(3, seed=1, n_beams=61).scans[0]
    assert s.shape == (61, 2)
    return _ro(np.array(s, np.float64))


# (nx, ny) -> the R it must select; 3 x 683 = 2,049 shifts need two passes of R = 5
R_SHAPES = {(16, 16): (1, 1), (257, 1): (1, 2), (27, 19): (1, 3), (32, 32): (1, 4), (35, 33): (1, 5), (39, 37): (1, 6),
            (41, 43): (1, 7), (64, 32): (1, 8), (3, 683): (2, 5)}


@functools.lru_cache(maxsize=None)
def r_case(nx, ny):
    return SearchCase("R-%dx%d" % (nx, ny), small_map(), SMALL_ORIGIN, SMALL_CW, SMALL_CAP, [scan61()], [0, 0],
                      [[0.10, 0.30, -0.20], [-0.20, -5.25, -3.65]], dict(n_theta=2, d_theta=0.05, nx=nx, ny=ny, step=1))


# windows wider than the map: (step, nx, ny) with nx step > 53 and ny step > 37, even and odd
WIDE_WINDOWS = ((1, 54, 38), (1, 55, 39), (4, 14, 10), (4, 15, 11))


@functools.lru_cache(maxsize=None)
def wide_case(step, nx, ny):
    return SearchCase("wide-%d-%dx%d" % (step, nx, ny), small_map(), SMALL_ORIGIN, SMALL_CW, SMALL_CAP, [scan61()],
                      [0, 0], [[0.10, 0.30, -0.20], [0.05, 5.2, 0.35]],
                      dict(n_theta=1, d_theta=0.05, nx=nx, ny=ny, step=step))


GUARD_CAPS = (15, 16)     # the largest d_cap whose squares fit a byte, and the first that does not


@functools.lru_cache(maxsize=None)
def guard_case(d_cap):
    """Three occupied cells in one corner of a 37 x 53 map of 0.25 m cells: most cells
    lie at the cap.  The query's points are cell centres at heading 0: on occupied
    cells, on cells below the cap, on cells at exactly d_cap^2 and beyond the map."""
    g = np.zeros((37, 53), np.int8)
    g[2, 3] = g[5, 1] = g[4, 2] = 9
    origin, cw = np.array([-2.0, -1.0]), 0.25
    cells = [(3, 2), (1, 5), (2, 4), (10, 8), (4, 12), (20, 2), (3 + d_cap, 2), (3, 2 + d_cap), (40, 30), (52, 36),
             (30, 20), (3 + d_cap, 4), (-1, 5), (53, 10), (10, -1), (10, 37), (200, 200), (-300, 7)]
    pts = np.array([(origin[0] + (c + 0.5) * cw, origin[1] + (r + 0.5) * cw) for c, r in cells])
    return SearchCase("guard-%d" % d_cap, g, origin, cw, d_cap, [pts], [0], [[0.0, 0.0, 0.0]],
                      dict(n_theta=1, d_theta=0.0, nx=3, ny=3, step=1))


BIG_H, BIG_W, BIG_CAP = 1000, 1100, 4


@functools.lru_cache(maxsize=None)
def big_case():
    """A 1,000 x 1,100 map with occupied cells near the far corner and one near the
    origin; a 3 x 3 x 3 window centred near the far corner: the bordered table has
    1,006 x 1,106 cells and every cell the query reads lies past the first
    1,048,576 of them, which loc_table_kernel fills on the second trip of its loop."""
    g = np.zeros((BIG_H, BIG_W), np.int8)
    occ = [(990, 1090), (985, 1080), (992, 1075), (978, 1093), (981, 1084), (996, 1088)]
    for r, c in occ + [(3, 4)]:
        g[r, c] = 11
    origin, cw = np.array([-8.0, -4.0]), 0.25
    # the scan, in the sensor frame at the centre's cell (980, 1080): offsets in cells
    offs = [(r - 980 + dr, c - 1080 + dc) for r, c in occ for dr, dc in ((0, 0), (1, 2), (-2, 1))]
    pts = np.array([(dc * cw, dr * cw) for dr, dc in offs])
    centre = [[0.0, origin[0] + 1080.5 * cw, origin[1] + 980.5 * cw]]
    return SearchCase("big-table", g, origin, cw, BIG_CAP, [pts], [0], centre,
                      dict(n_theta=3, d_theta=0.2, nx=3, ny=3, step=1))


TILE_SIZES = (4095, 4096, 4097, 8193)


@functools.lru_cache(maxsize=None)
def tile_case():
    """Scans of one point short of, exactly, one past one LDS tile and one past two,
    seeded uniform over the small map (a little beyond it), a 3 x 3 window."""
    rng = np.random.default_rng(41)
    scans = [rng.uniform(-5.5, 5.5, size=(n, 2)) * (1.0, 0.7) for n in TILE_SIZES]
    return SearchCase("tiles", small_map(), SMALL_ORIGIN, SMALL_CW, SMALL_CAP, scans, range(len(TILE_SIZES)),
                      [[0.2, 0.1, -0.1]] * len(TILE_SIZES), dict(n_theta=2, d_theta=0.1, nx=3, ny=3, step=1))


EXTREMES = np.array([(1e12, -3.0), (1e308, 1e308), (-1e308, 1e308)])


@functools.lru_cache(maxsize=None)
def extreme_case():
    """Finite points whose map coordinates overflow: they count d_cap^2 in every bin."""
    pts = np.concatenate([scan61()[:20], EXTREMES, scan61()[20:30]])
    return SearchCase("extremes", small_map(), SMALL_ORIGIN, SMALL_CW, SMALL_CAP, [pts, scan61()[:30]], [0, 1],
                      [[0.7, 0.3, -0.2], [0.7, 0.3, -0.2]], dict(n_theta=5, d_theta=0.6, nx=5, ny=4, step=2))


# ------------------------------------------------------------------------- refinement

class Query:
    def __init__(self, name, pts, start, **params):
        self.name, self.pts = name, _ro(np.asarray(pts, np.float64).reshape(-1, 2))
        self.start, self.params = _ro(np.asarray(start, np.float64)), params


class RefineCase:
    """Queries (scan, start pose (x, y, theta), refinement parameters) on one map."""

    def __init__(self, name, grid, origin, cw, d_cap, queries):
        self.name, self.grid, self.origin, self.cw, self.d_cap = name, _ro(np.asarray(grid, np.int8)), \
            _ro(np.asarray(origin, float)), cw, d_cap
        self.queries = tuple(queries)

    @functools.cached_property
    def F(self):
        return _ro(loc_ref.field(self.grid, self.d_cap))

    def refine(self, q, rng=None):
        return loc_ref.refine(self.F, self.origin, self.cw, self.d_cap, q.pts, q.start,
                              **{**loc_ref.REFINE_DEFAULTS, **q.params}, rng=rng)

    @functools.cached_property
    def ref(self):
        """The restatement's dict per query."""
        out = tuple(self.refine(q) for q in self.queries)
        for r in out:
            r["pose"].setflags(write=False)
        return out

    def linearise(self, q, pose=None):
        return loc_ref.linearise(self.F, self.origin, self.cw, self.d_cap, q.pts, q.start if pose is None else pose)

    def launches(self):
        """The queries grouped by their parameters: [(params, [query index])], one launch each."""
        groups = {}
        for n, q in enumerate(self.queries):
            groups.setdefault(tuple(sorted(q.params.items())), []).append(n)
        return [(dict(k), v) for k, v in groups.items()]


SIZES = (1, 2, 255, 256, 257, 511, 513, 1000)
SUB_CELL = ((0.0, 0.0), (0.02, 0.01), (-0.03, 0.02), (0.01, -0.04), (-0.02, -0.03))   # m, cells of 0.1 m
SIZE_START = (0.07, -0.06, 0.025)   # within 0.1 m and 0.03 rad of the truth


@functools.lru_cache(maxsize=None)
def cloud():
    """1,110 points in the sensor frame of loc_ref.refine_case's truth: the centre of
    each of the 222 occupied cells plus each of five fixed sub-cell offsets, in an
    order (stride 41, coprime to 1,110) in which every cut covers the whole box."""
    g, origin, cw, d_cap, _, truth = loc_ref.refine_case()
    rr, cc = np.nonzero(g > 0)
    assert len(rr) == 222
    w = np.array([(origin[0] + (c + 0.5) * cw + ox, origin[1] + (r + 0.5) * cw + oy)
                  for ox, oy in SUB_CELL for r, c in zip(rr, cc)])
    w = w[(np.arange(len(w)) * 41) % len(w)]
    c, s = np.cos(truth[2]), np.sin(truth[2])
    dx, dy = w[:, 0] - truth[0], w[:, 1] - truth[1]
    return _ro(np.stack([c * dx + s * dy, -s * dx + c * dy], axis=1))


@functools.lru_cache(maxsize=None)
def size_case():
    g, origin, cw, d_cap, _, truth = loc_ref.refine_case()
    return RefineCase("sizes", g, origin, cw, d_cap,
                      [Query("n%d" % n, cloud()[:n], truth + SIZE_START) for n in SIZES])


@functools.lru_cache(maxsize=None)
def limit_case():
    """The 257-point cut with max_iters at and one below the restatement's count N."""
    g, origin, cw, d_cap, _, truth = loc_ref.refine_case()
    n = size_case().ref[SIZES.index(257)]["iters"]
    return RefineCase("limit", g, origin, cw, d_cap,
                      [Query("N", cloud()[:257], truth + SIZE_START, max_iters=n),
                       Query("N-1", cloud()[:257], truth + SIZE_START, max_iters=n - 1)])


# The exact maps: 24 x 32 cells of 0.25 m from (-1, -0.5); poses with heading exactly 0.
XH, XW, XCW = 24, 32, 0.25
XORIGIN = np.array([-1.0, -0.5])
XPOSE = np.array([0.75, 0.5, 0.0])


def at(u, v, pose=XPOSE):
    """The scan point (sensor frame, heading 0) whose bilinear coordinates are (u, v)."""
    return (XORIGIN[0] + (u + 0.5) * XCW - pose[0], XORIGIN[1] + (v + 0.5) * XCW - pose[1])


def _walls(rows=(), cols=(), cells=()):
    g = np.zeros((XH, XW), np.int8)
    for r in rows:
        g[r, :] = 5
    for c in cols:
        g[:, c] = 5
    for r, c in cells:
        g[r, c] = 5
    return g


PIVOTS = ("dd0", "dd1", "dd2")


@functools.lru_cache(maxsize=None)
def pivot_case():
    """One query per pivot of the LDL^T solve, each with exact zeros:
    dd0: a full-width wall on row 12 only, so the field depends on the row alone and jx = 0;
    dd1: a full-height wall on column 16 only, jy = 0;
    dd2: both walls and the two points (a, 0) and (0, b), each next to one wall and more than
         d_cap cells from the other: jt = 0 for both, H = diag(jx^2, jy^2, 0)."""
    spread = [at(u, v) for u, v in ((3.25, 10.5), (9.5, 13.25), (14.75, 11.0), (20.0, 12.75), (27.5, 9.25))]
    spread_t = [at(u, v) for v, u in ((3.25, 14.5), (9.5, 17.25), (14.75, 15.0), (20.0, 16.75), (22.5, 13.25))]
    # dd2: the sensor sits on (u, v) = (4, 2): (a, 0) lies on v = 2, next to the wall on column 16,
    # and (0, b) on u = 4, next to the wall on row 12; d_cap = 6 keeps the other wall out of reach
    pose = np.array([XORIGIN[0] + 4.5 * XCW, XORIGIN[1] + 2.5 * XCW, 0.0])
    two = [at(14.75, 2.0, pose), at(4.0, 10.5, pose)]
    return (RefineCase("pivot-dd0", _walls(rows=(12,)), XORIGIN, XCW, 6, [Query("dd0", spread, XPOSE)]),
            RefineCase("pivot-dd1", _walls(cols=(16,)), XORIGIN, XCW, 6, [Query("dd1", spread_t, XPOSE)]),
            RefineCase("pivot-dd2", _walls(rows=(12,), cols=(16,)), XORIGIN, XCW, 6, [Query("dd2", two, pose)]))


def box():
    """Walls one cell inside the border: rows 1 and 22, columns 1 and 30."""
    return _walls(rows=(1, XH - 2), cols=(1, XW - 2))


BOX_CAP = 4
ORDINARY = ((1.25, 6.0), (1.25, 15.0), (29.75, 9.0), (29.75, 18.0), (8.0, 1.25), (20.0, 1.25), (11.0, 21.75),
            (24.0, 21.75))    # eight points a quarter cell off the four walls
# (u, v) of the point under test -> whether its bilinear cell is inside the grid
BOUNDS = {"fu=-1": ((-0.5, 11.5), False), "fu=0,a=0": ((0.0, 11.5), True), "fu=0": ((0.75, 11.5), True),
          "fu=W-2,a=0": ((XW - 2.0, 11.5), True), "fu=W-2": ((XW - 1.5, 11.5), True),
          "fu=W-1,a=0": ((XW - 1.0, 11.5), False),
          "fv=-1": ((15.5, -0.5), False), "fv=0,b=0": ((15.5, 0.0), True), "fv=0": ((15.5, 0.75), True),
          "fv=H-2,b=0": ((15.5, XH - 2.0), True), "fv=H-2": ((15.5, XH - 1.5), True),
          "fv=H-1,b=0": ((15.5, XH - 1.0), False)}


@functools.lru_cache(maxsize=None)
def bounds_case():
    """One point on each inclusive bound of the bilinear cell and one cell beyond it, each
    with the eight ordinary inliers; then all the inside ones and all the outside ones
    together.  max_iters = 1: the inliers reported are those of the start pose."""
    ordinary = [at(u, v) for u, v in ORDINARY]
    qs = [Query(name, [at(*uv)] + ordinary, XPOSE, max_iters=1) for name, (uv, _) in BOUNDS.items()]
    qs.append(Query("all-in", [at(*uv) for uv, ok in BOUNDS.values() if ok] + ordinary, XPOSE, max_iters=1))
    qs.append(Query("all-out", [at(*uv) for uv, ok in BOUNDS.values() if not ok] + ordinary, XPOSE, max_iters=1))
    return RefineCase("bounds", box(), XORIGIN, XCW, BOX_CAP, qs)


CAP_CELL = (12, 20)      # the lone occupied cell (row, column) of the cap case, d_cap = 2
THREE_AT_CAP = ((21.5, 13.5), (18.5, 10.5), (21.25, 10.5), (18.5, 13.75))    # one corner holds 2, three hold 4
ALL_AT_CAP = ((25.5, 17.5), (22.5, 13.5), (21.5, 14.5), (17.5, 10.25))
CAP_ORDINARY = ((2.25, 8.0), (2.25, 17.0), (1.75, 12.5), (1.5, 20.0), (9.0, 2.25), (22.0, 2.25), (14.5, 1.75),
                (27.0, 1.5))


@functools.lru_cache(maxsize=None)
def cap_case():
    """d_cap = 2 around one lone cell: the bilinear cells diagonal to it have exactly three
    corners at the cap (included), the next ones all four (skipped)."""
    g = _walls(rows=(2,), cols=(2,), cells=(CAP_CELL,))
    pts = [at(u, v) for u, v in THREE_AT_CAP + ALL_AT_CAP + CAP_ORDINARY]
    return RefineCase("cap", g, XORIGIN, XCW, 2, [Query("cap", pts, XPOSE, max_iters=1)])


FRACTIONS = ((0.5, False), (0.5000001, True), (0.625, True))     # min_inlier_frac -> TOO_FEW
FRAC_INLIERS = ((1.25, 6.0), (29.75, 18.0), (8.0, 1.25), (24.0, 21.75))


@functools.lru_cache(maxsize=None)
def fraction_case():
    """Eight points, four on the field; the outliers are the three extreme points and one
    point in the middle of the box, more than d_cap cells from every wall."""
    pts = np.array([at(u, v) for u, v in FRAC_INLIERS] + [tuple(e) for e in EXTREMES] + [at(15.5, 11.5)])
    return RefineCase("fraction", box(), XORIGIN, XCW, BOX_CAP,
                      [Query("frac=%r" % f, pts, XPOSE, min_inlier_frac=f) for f, _ in FRACTIONS])


@functools.lru_cache(maxsize=None)
def after_step_case():
    """A status other than CONVERGED / MAX_ITERS after a step has been taken.

    too-few: the eight ordinary points one cell left of where they belong and a ninth at
    u = 30.5 in the last bilinear cell; min_inlier_frac = 1.  The step moves everything about
    a cell to the right, the ninth point leaves the grid, 8 < 9.

    singular: a full-height wall on column 8 and the short wall on row 12, columns 22..24,
    d_cap = 3.  Forty points a cell and a half left of the long wall and two points off the short
    wall's right end, above and below it; the first step moves the scan more than a cell to the right, the two
    points leave the short wall's reach (all four corners at the cap), and what is left
    sees the long wall only: jy = 0 exactly, H11 = 0, the dd1 exit, at iters = 1."""
    start = XPOSE - (1.0 * XCW, 0.0, 0.0)
    pts = [at(u, v) for u, v in ORDINARY + ((31.5, 11.5),)]
    too_few = RefineCase("after-step-too-few", box(), XORIGIN, XCW, BOX_CAP,
                         [Query("too-few", pts, start, min_inlier_frac=1.0)])
    g = _walls(cols=(8,), cells=[(12, c) for c in (22, 23, 24)])
    left = [at(8.0, 1.5 + 0.5 * k) for k in range(40)]
    end = [at(28.0, 11.25), at(28.0, 12.75)]
    singular = RefineCase("after-step-singular", g, XORIGIN, XCW, 3,
                          [Query("singular", left + end, XPOSE - (1.5 * XCW, 0.0, 0.0))])
    return too_few, singular


def refine_cases():
    """Every refinement case that goes to the GPU."""
    return (size_case(), limit_case()) + pivot_case() + (bounds_case(), cap_case(), fraction_case()) + after_step_case()
