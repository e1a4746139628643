"""Hand-placed inputs for the occupancy-grid mapper (no GPU, no randomness).

csrc/grid_kernels.hip treats a beam differently by where it starts, where it
ends, which 256-beam block and which scan it belongs to, and a cell by which
events reach it and in what order.  The cases here put beams on those
positions by hand:

* every case but the rotated one uses headings of exactly 0 (cos = 1, sin = 0),
  a cell width of 0.25 or 1.0 and coordinates that are short binary fractions,
  so global points and cell indices are exact under every rounding order and
  do not depend on the host's BLAS (tests/test_grid_cases.py proves it with
  rational arithmetic);
* ``walk`` is an instrumented restatement of the reference's beam walk that
  records ``(beam index, step, hit)`` per cell, ``closed_form`` the kernel file
  header's per-cell rule on those events, ``relations`` what a case contains
  (untouched / miss-only / both-last-hit / both-last-miss cells, cells whose
  last two beams disagree across a 256-beam block or across scans, cells one
  beam decides alone, saturated cells,
  beams that leave the grid, robots outside it, zero-length beams);
* ``case(name)`` builds a case once per process; its oracle result
  (``GridCase.ref``) is computed once and shared read-only.

tests/test_grid_cases.py checks these inputs on the CPU; tests/test_grid_gpu.py
runs them on the GPU.
"""
import functools
from collections import Counter

import numpy as np

import grid_ref
import occupancy_oracle as oo

START_VALUES = (-128, -127, -2, -1, 0, 1, 2, 126, 127)
ODDS = ((1, 1), (3, 1), (5, 2), (1, 127), (127, 127))
RAGGED_LENS = (0, 1, 63, 64, 65, 0, 255, 256, 257, 1, 0)
COUNTS = (1, 255, 256, 257, 512)
BLOCK = 256                 # kGridBlock: beams per workgroup of grid_rays_kernel


class Geo:
    """A grid placement: H x W cells of width w from (min_x, min_y)."""

    def __init__(self, H, W, min_x, min_y, w):
        self.H, self.W, self.min_x, self.min_y, self.w = H, W, min_x, min_y, w

    def c(self, cx, cy):
        """Centre of cell (column cx, row cy); cells outside the grid are fine."""
        return (self.min_x + (cx + 0.5) * self.w, self.min_y + (cy + 0.5) * self.w)


class GridCase:
    """poses (S, 3), scans [(n_s, 2)], and either a grid placement with a start
    grid (``update_occupancy_grid``) or minimum extents (``produce_occupancy_grid``)."""

    def __init__(self, name, poses, scans, geo=None, odds=(3, 1), start=None, produce=None, w=None, named=None):
        self.name = name
        self.poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        self.scans = [np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in scans]
        assert len(self.poses) == len(self.scans)
        self.k_hit, self.k_miss = odds
        self.produce = produce                          # None or (min_width, min_height)
        self.geo = geo
        self.w = geo.w if geo is not None else w
        self.named = named or {}
        if produce is None:
            self.start = np.zeros((geo.H, geo.W), dtype=np.int8) if start is None else np.asarray(start, np.int8)
            assert self.start.shape == (geo.H, geo.W)
        else:
            self.start = None
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.scans])]).astype(np.int64)
        self.P = int(self.off[-1])
        for a in (self.poses, *self.scans, *([] if self.start is None else [self.start])):
            a.setflags(write=False)

    @functools.cached_property
    def gpts(self):
        """Global points by the exact restatement (tests/grid_ref.py)."""
        g = grid_ref.global_points_exact(self.poses, self.scans)
        for a in g:
            a.setflags(write=False)
        return g

    def geometry(self):
        """(H, W, min_x, min_y): given, or the reference's arithmetic on the points."""
        if self.produce is None:
            return self.geo.H, self.geo.W, self.geo.min_x, self.geo.min_y
        min_x, min_y, W, H = oo.geometry(self.gpts, self.w, *self.produce)
        return H, W, min_x, min_y

    def bounds(self):
        """(min x, max x, min y, max y) of the global points."""
        a = np.concatenate(self.gpts)
        return np.array([a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()])

    @functools.cached_property
    def ref(self):
        """The oracle's (grid, (min_x, min_y)); read-only."""
        if self.produce is None:
            g = oo.update(self.start.copy(), self.poses, self.scans, self.w, self.geo.min_x, self.geo.min_y,
                          self.k_hit, self.k_miss)
            origin = (self.geo.min_x, self.geo.min_y)
        else:
            g, origin = oo.produce(self.poses, self.scans, self.w, min_width=self.produce[0],
                                   min_height=self.produce[1], k_hit=self.k_hit, k_miss=self.k_miss)
        g.setflags(write=False)
        return g, origin

    def scan_of(self, g):
        return int(np.searchsorted(self.off, g, side="right")) - 1


def _build(name, geo, specs, **kw):
    """specs: [((robot x, robot y), [(end x, end y), ...])] in GLOBAL coordinates,
    heading 0: the scan holds end - robot."""
    poses, scans = [], []
    for (rx, ry), ends in specs:
        poses.append((rx, ry, 0.0))
        scans.append(np.array([(ex - rx, ey - ry) for ex, ey in ends], dtype=np.float64).reshape(-1, 2))
    return GridCase(name, poses, scans, geo=geo, **kw)


def tiled_start(H, W):
    """START_VALUES[(x + 2 y) % 9]: every value in every row and column band."""
    y, x = np.mgrid[0:H, 0:W]
    return np.array(START_VALUES, dtype=np.int8)[(x + 2 * y) % 9]


# ---- the instrumented beam walk ---------------------------------------------


def cell(p, mn, w):
    """global_position_to_grid_cell on one coordinate, in double arithmetic."""
    return int(np.floor((np.float64(p) - np.float64(mn)) / np.float64(w)))


class Walk:
    def __init__(self, events, beams, shape):
        self.events, self.beams, self.shape = events, beams, shape


def walk(c):
    """The reference's bresenham_update for every beam in order, recording per
    cell (row, column) the events (beam, step, hit) instead of changing values,
    and per beam where it starts, ends and stops."""
    H, W, min_x, min_y = c.geometry()
    w = c.w
    events, beams = {}, []
    g = 0

    def inside(x, y):
        return 0 <= x < W and 0 <= y < H
    for s, (pose, pts) in enumerate(zip(c.poses, c.gpts)):
        rx, ry = cell(pose[0], min_x, w), cell(pose[1], min_y, w)
        for p in pts:
            x0, y0 = rx, ry
            x1, y1 = cell(p[0], min_x, w), cell(p[1], min_y, w)
            dx, dy = abs(x1 - x0), -abs(y1 - y0)
            sx, sy = (1 if x1 > x0 else -1), (1 if y1 > y0 else -1)
            err, step = dx + dy, 0
            b = {"g": g, "scan": s, "start": (x0, y0), "end": (x1, y1), "robot_outside": not inside(x0, y0),
                 "zero_length": (x0, y0) == (x1, y1) and inside(x0, y0), "tie_x": False, "tie_y": False,
                 "last_cell": None}
            while inside(x0, y0):
                events.setdefault((y0, x0), []).append((g, step, 0))
                b["last_cell"] = (x0, y0)
                step += 1
                e2 = 2 * err
                b["tie_x"] |= e2 == dy
                b["tie_y"] |= e2 == dx
                if e2 >= dy:
                    if x0 == x1:
                        break
                    err += dy
                    x0 += sx
                if e2 <= dx:
                    if y0 == y1:
                        break
                    err += dx
                    y0 += sy
            b["hit"] = inside(x0, y0)
            if b["hit"]:
                events[(y0, x0)].append((g, step, 1))
            b["exits"] = not b["robot_outside"] and not b["hit"]
            b["steps"] = step
            beams.append(b)
            g += 1
    return Walk(events, beams, (H, W))


def closed_form(g0, ev, k_hit, k_miss):
    """The kernel file header's rule; max(ev) orders events as the kernel's
    key g << 24 | step << 1 | hit does."""
    m = sum(1 for e in ev if not e[2])
    h = len(ev) - m
    if m == 0 and h == 0:
        return g0
    if h == 0:
        return -128 if g0 > 0 else max(g0 - m * k_miss, -128)
    if m == 0:
        return 127 if g0 < 0 else min(g0 + h * k_hit, 127)
    return 127 if max(ev)[2] else -128


def expected_grid(c, wk=None):
    """closed_form on every cell of the start grid (zeros for a produce case)."""
    wk = wk or walk(c)
    H, W = wk.shape
    out = np.zeros((H, W), dtype=np.int8) if c.start is None else c.start.copy()
    for (y, x), ev in wk.events.items():
        out[y, x] = closed_form(int(out[y, x]), ev, c.k_hit, c.k_miss)
    return out


def deciders(ev):
    """(winner, rival) of a cell: its last event, and the last event of any
    OTHER beam (None if one beam alone touches the cell).  The cell is contested
    when the rival is of the other kind: ordering those two beams wrongly flips it."""
    win = max(ev)
    rest = [e for e in ev if e[0] != win[0]]
    return win, (max(rest) if rest else None)


def relations(c, wk=None):
    """Counter of what the case contains: cells by relation, beams by kind."""
    wk = wk or walk(c)
    H, W = wk.shape
    r = Counter()
    start = np.zeros((H, W), dtype=np.int8) if c.start is None else c.start
    r["untouched"] = H * W - len(wk.events)
    for (y, x), ev in wk.events.items():
        g0 = int(start[y, x])
        m = sum(1 for e in ev if not e[2])
        h = len(ev) - m
        if m and not h:
            r["miss only"] += 1
            if g0 > 0:
                r["miss on a positive cell"] += 1
            elif g0 - m * c.k_miss < -128:
                r["saturated below"] += 1
        elif h and not m:
            r["hit only"] += 1
        else:
            r["both, last a hit" if max(ev)[2] else "both, last a miss"] += 1
            win, rival = deciders(ev)
            if rival is None:
                r["decided within one beam"] += 1
            elif rival[2] != win[2]:
                r["contested"] += 1
                if win[0] // BLOCK != rival[0] // BLOCK:
                    r["decided across a block boundary"] += 1
                if c.scan_of(win[0]) != c.scan_of(rival[0]):
                    r["decided across scans"] += 1
        if h and g0 + h * c.k_hit > 127:
            r["saturated above"] += 1
    for b in wk.beams:
        for k in ("exits", "robot_outside", "zero_length"):
            if b[k]:
                r["beam " + k.replace("_", " ")] += 1
    return r


# ---- the cases --------------------------------------------------------------


def ring(r):
    """The 8 r cells of the square ring of radius r around (0, 0), counter-clockwise from (r, -r)."""
    if r == 0:
        return [(0, 0)]
    out = [(r, d) for d in range(-r, r)] + [(-d, r) for d in range(-r, r)]
    out += [(-r, -d) for d in range(-r, r)] + [(d, -r) for d in range(-r, r)]
    return out


def star(H, W):
    """One robot cell at the centre; endpoints on every cell of the rings of
    radius 3, 7 (all octants, both axes, the diagonals, every slope) and 4 (the
    error term ties, e2 == dy or e2 == dx, only where the longer side is even:
    rings 3 and 7 have not one tie, ring 4 has 24), the zero-length beam, the
    ring of radius 40 (far outside: exits through all four borders) and three
    times the vector to each corner cell (exits through the corners).  Order:
    ring 3, the exiting beams, rings 7 and 4, the zero-length beam, so ring 3's
    endpoints end on a miss and the other rings' on a hit.  One scan: S = 1."""
    geo = Geo(H, W, -2.0, -1.5, 0.25)
    rx, ry = W // 2, H // 2
    offs = ring(3) + ring(40) + [(3 * (cx - rx), 3 * (cy - ry)) for cx in (0, W - 1) for cy in (0, H - 1)]
    offs += ring(7) + ring(4) + [(0, 0)]
    return _build(f"star-{H}x{W}", geo, [(geo.c(rx, ry), [geo.c(rx + a, ry + b) for a, b in offs])])


def ragged():
    """Scans of RAGGED_LENS beams (962 in all) on 24 x 40: robots at the centre,
    in the four corner cells and in one cell outside; the empty scans' poses
    are in-grid cells no other scan uses.  Endpoints step through a box three
    cells wider than the grid on every side.  Tiled start grid, odds (5, 2)."""
    H, W = 24, 40
    geo = Geo(H, W, -2.0, -1.5, 0.25)
    robots = [(7, 5), (-3, 10), (0, 0), (W - 1, 0), (0, H - 1), (33, 17), (W - 1, H - 1), (W // 2, H // 2),
              (W // 2 - 1, H // 2 + 1), (W // 2, H // 2), (11, 20)]
    specs = []
    for s, (n, rc) in enumerate(zip(RAGGED_LENS, robots)):
        ends = [geo.c((7 * j + 3 * s) % (W + 6) - 3, (5 * j + 11 * s) % (H + 6) - 3) for j in range(n)]
        specs.append((geo.c(*rc), ends))
    return _build("ragged", geo, specs, odds=(5, 2), start=tiled_start(H, W))


def counts(P):
    """P beams in total (two scans once P > 1); the last beam alone ends on,
    and alone touches, the corner cell (W - 1, H - 1)."""
    H, W = 24, 40
    geo = Geo(H, W, -2.0, -1.5, 0.25)
    ends = [geo.c((7 * g) % (W - 1), (5 * g) % (H - 1)) for g in range(P - 1)] + [geo.c(W - 1, H - 1)]
    n0 = P // 3
    specs = [(geo.c(W // 2, H // 2), ends[:n0]), (geo.c(W // 2 + 1, H // 2), ends[n0:])] if P > 1 else \
        [(geo.c(W // 2, H // 2), ends)]
    return _build(f"count-{P}", geo, specs)


S300_EXTREMES = {260: (0, (-1.125, 1.0)), 269: (1, (4.375, 0.5)), 281: (0, (1.0, -0.875)), 299: (2, (1.5, 3.625))}


def s300():
    """300 scans of (1, 2, 0, 3)[s % 4] beams (75 of them empty).  All points
    lie in [0.125, 2.875] x [0.125, 2.125] but four, the extreme ones, which sit
    in scans 260, 269, 281 and in the last beam of the last scan: the bounds,
    hence the produced grid, are right only if grid_bounds_kernel's strided loop
    reaches s >= 256 and the empty scans' +-inf block bounds do no harm."""
    poses, scans = [], []
    for s in range(300):
        rx, ry = 0.25 * (s % 7) + 0.125, 0.25 * (s % 5) + 0.125
        ends = [(0.125 + 0.25 * ((3 * s + 5 * j) % 12), 0.125 + 0.25 * ((s + 7 * j) % 9))
                for j in range((1, 2, 0, 3)[s % 4])]
        if s in S300_EXTREMES:
            j, p = S300_EXTREMES[s]
            ends[j] = p
        poses.append((rx, ry, 0.0))
        scans.append(np.array([(ex - rx, ey - ry) for ex, ey in ends]).reshape(-1, 2))
    return GridCase("s300", poses, scans, produce=(0, 0), w=0.25)


# name -> ((column, row) of the cell, beam of the first event, beam of the second, result)
DUELS = {
    "lanes: hit by 10, miss by 11": ((24, 12), 10, 11, -128),
    "lanes: miss by 12, hit by 13": ((16, 12), 12, 13, 127),
    "blocks: hit by 255, miss by 256": ((20, 16), 255, 256, -128),
    "blocks: miss by 511, hit by 512": ((20, 8), 511, 512, 127),
    "scans: hit by the last beam of scan 1, miss by the first of scan 3": ((5, 6), 522, 523, -128),
    "one beam: miss at step 5, hit at step 6": ((25, 17), 100, 100, 127),
}


def duels():
    """Cells decided by two named beams (DUELS).  Scan 0 (robot (20, 12), beams
    0..519) holds the duels of neighbouring lanes and of the block boundaries
    255|256 and 511|512, each along its own direction; every other beam of it
    is zero-length and touches the robot's cell only.  Scan 1 (beams 520..522)
    ends on (5, 6), scan 2 is empty, scan 3's first beam (523) crosses (5, 6)."""
    H, W = 24, 40
    geo = Geo(H, W, -2.0, -1.5, 0.25)
    r0 = (20, 12)
    ends0 = {10: (24, 12), 11: (27, 12), 12: (13, 12), 13: (16, 12), 100: (25, 17), 255: (20, 16), 256: (20, 19),
             511: (20, 5), 512: (20, 8)}
    specs = [(geo.c(*r0), [geo.c(*ends0.get(g, r0)) for g in range(520)]),
             (geo.c(5, 2), [geo.c(5, 2), geo.c(5, 2), geo.c(5, 6)]),
             (geo.c(30, 20), []),
             (geo.c(2, 6), [geo.c(9, 6), geo.c(2, 6)])]
    return _build("duels", geo, specs, named=DUELS)


LONG_W = 32800


def long_row():
    """A 1 x 32,800 grid (the one case larger than a few thousand cells): beam 0
    walks the whole row, so it reaches cell 32,790 at step 32,790 >= 2^15; beam 1
    (another scan) ends there six steps from its robot.  The later beam's hit
    must win although its step is smaller: the beam index has to sit above
    every step in the event key."""
    geo = Geo(1, LONG_W, 0.0, 0.0, 1.0)
    return _build("long-row", geo, [(geo.c(0, 0), [geo.c(LONG_W - 1, 0)]),
                                    (geo.c(LONG_W - 20, 0), [geo.c(LONG_W - 10, 0)])])


def saturation(n, k_hit, k_miss, vertical):
    """n identical beams from cell 1 to cell 12 of a 1 x 17 (or 17 x 1) grid
    whose start values run through START_VALUES."""
    H, W = (17, 1) if vertical else (1, 17)
    geo = Geo(H, W, -3.0, 5.0, 1.0)
    at = (lambda i: geo.c(0, i)) if vertical else (lambda i: geo.c(i, 0))
    start = np.array([START_VALUES[i % 9] for i in range(17)], dtype=np.int8).reshape(H, W)
    return _build(f"saturation-{n}x({k_hit},{k_miss})-{H}x{W}", geo, [(at(1), [at(12)] * n)], odds=(k_hit, k_miss),
                  start=start)


SATURATION = ((130, 1, 1, False), (2, 1, 127, True), (3, 127, 127, False), (130, 1, 1, True))


def start_values(odds):
    """18 x 24, row y starting at START_VALUES[y % 9]; scan y (robot (2, y)) ends
    on (6, y), then on (10, y): columns 2..5 two misses, 6 hit then miss, 7..9 one
    miss, 10 miss then hit, the rest untouched.  Every relation meets every value."""
    H, W = 18, 24
    geo = Geo(H, W, 1.0, -3.0, 0.25)
    start = np.repeat(np.array([START_VALUES[y % 9] for y in range(H)], dtype=np.int8)[:, None], W, axis=1)
    specs = [(geo.c(2, y), [geo.c(6, y), geo.c(10, y)]) for y in range(H)]
    return _build(f"start-({odds[0]},{odds[1]})", geo, specs, odds=odds, start=start)


def tiny(kind):
    """Grids of one row, one column or one cell, with results known by hand (TINY_EXPECTED)."""
    if kind not in ("1x17", "17x1"):
        geo = Geo(1, 1, 0.5, -0.25, 0.25)
        here, away = geo.c(0, 0), geo.c(3, 0)
        ends = {"1x1-zero": [here], "1x1-exit": [away], "1x1-hit-then-miss": [here, away]}[kind]
        return _build("tiny-" + kind, geo, [(here, ends)])
    H, W = (1, 17) if kind == "1x17" else (17, 1)
    geo = Geo(H, W, -1.0, 2.0, 1.0)
    at = (lambda i: geo.c(i, 0)) if kind == "1x17" else (lambda i: geo.c(0, i))
    return _build("tiny-" + kind, geo, [(at(2), [at(9)])])


_LINE = [0, 0, -1, -1, -1, -1, -1, -1, -1, 127, 0, 0, 0, 0, 0, 0, 0]
TINY_EXPECTED = {
    "1x1-zero": [[127]],               # miss (0 -> -1), then the hit on a negative cell -> 127
    "1x1-exit": [[-1]],                # one miss, the walk leaves the grid: no hit
    "1x1-hit-then-miss": [[-128]],     # 127 after beam 0; beam 1's miss on a positive cell -> -128
    "1x17": [_LINE],                   # cells 2..8 one miss; cell 9 miss, then hit -> 127
    "17x1": [[v] for v in _LINE],
}


def borders():
    """5 x 7 cells of 0.25 from (-0.5, -0.75); the pose is (0, 0, 0), so global
    = local exactly and the robot stands in cell (2, 3).  Endpoints exactly on
    min, on two interior borders and on min + W w (H w), and one ulp on either
    side of each, in x (at row 1's centre) and in y (at column 5's centre).
    ``p - min`` is exact for the interior border below 0 (-0.25, -0.5 in y) and
    rounds for the one above (0.25, 0.0 in y) and for min + H w in y: there the
    point one ulp below the border lands in the cell above it (outside, for
    min + H w), in the reference as here (BORDER_CELLS)."""
    geo = Geo(5, 7, -0.5, -0.75, 0.25)
    pts = []
    for t in (-0.5, -0.25, 0.25, 1.25):
        pts += [(np.nextafter(t, -np.inf), -0.375), (t, -0.375), (np.nextafter(t, np.inf), -0.375)]
    for t in (-0.75, -0.5, 0.0, 0.5):
        pts += [(0.875, np.nextafter(t, -np.inf)), (0.875, t), (0.875, np.nextafter(t, np.inf))]
    return GridCase("borders", [(0.0, 0.0, 0.0)], [np.array(pts)], geo=geo)


# cell (column, row) of every endpoint of borders(): below, on, above each border
BORDER_CELLS = [(-1, 1), (0, 1), (0, 1), (0, 1), (1, 1), (1, 1), (3, 1), (3, 1), (3, 1), (6, 1), (7, 1), (7, 1),
                (5, -1), (5, 0), (5, 0), (5, 0), (5, 1), (5, 1), (5, 3), (5, 3), (5, 3), (5, 5), (5, 5), (5, 5)]


def _around(cx, cy, r):
    return [(cx + a * r, cy + b * r) for a, b in ring(1)]


PRODUCE = {
    # name: (poses, scans in GLOBAL coordinates per robot, min_width, min_height)
    "single-away": ([(0.0, 0.0)], [[(0.5, 0.25)]], 0, 0),          # 1 x 1, the robot outside it
    "single-self": ([(0.5, 0.25)], [[(0.5, 0.25)]], 0, 0),         # 1 x 1, a zero-length beam
    "collinear-x": ([(1.0, 0.0)], [[(0.25 * k, 0.0) for k in range(10)]], 0, 0),
    "collinear-y": ([(-0.5, 0.75)], [[(-0.5, 0.25 * k) for k in range(7)]], 0, 0),
    "min-larger": ([(0.0, 0.0)], [_around(0.0, 0.0, 1.0)], 4.0, 3.0),
    "min-equal": ([(0.0, 0.0)], [_around(0.0, 0.0, 1.0)], 2.25, 2.25),
    "min-smaller": ([(0.0, 0.0)], [_around(0.0, 0.0, 1.0)], 1.0, 0.5),
    "min-mixed": ([(0.0, 0.0)], [_around(0.0, 0.0, 1.0)], 5.5, 0.5),
    # scan 0's robot lies outside the grid its own points span with scan 1's
    "robot-outside": ([(0.0, 0.0), (2.5, 2.5)], [_around(2.5, 2.5, 0.5), _around(2.5, 2.5, 0.25)], 0, 0),
}


def produce_case(name):
    robots, ends, mw, mh = PRODUCE[name]
    poses = [(rx, ry, 0.0) for rx, ry in robots]
    scans = [np.array([(ex - rx, ey - ry) for ex, ey in e]).reshape(-1, 2) for (rx, ry), e in zip(robots, ends)]
    return GridCase("produce-" + name, poses, scans, produce=(mw, mh), w=0.25)


def rotated():
    """(poses, scans) with headings +-0.1, pi / 2, 3 and others and coordinates
    up to 1e3: input of the global-point comparison only (no grid)."""
    headings = (0.1, -0.1, np.pi / 2, 3.0, -np.pi / 2, np.pi, 1e-9, 0.7853981633974483, -2.5)
    vals = (0.0, 1.0, -1.0, 0.1, -0.1, 1.0 / 3.0, 1e-3, 7.25, -123.456, 999.999, 1e3, -1e3, 2.0 ** -30, 31.4159)
    poses, scans = [], []
    for i, th in enumerate(headings):
        poses.append((vals[(3 * i + 5) % len(vals)], vals[(5 * i + 2) % len(vals)], th))
        scans.append(np.array([(x, vals[(k + 3 * i + j) % len(vals)]) for k, x in enumerate(vals) for j in (0, 4, 9)]))
    return np.array(poses), scans


_BUILDERS = {}
for _H, _W in ((24, 40), (40, 24)):
    _BUILDERS[f"star-{_H}x{_W}"] = functools.partial(star, _H, _W)
_BUILDERS["ragged"] = ragged
for _P in COUNTS:
    _BUILDERS[f"count-{_P}"] = functools.partial(counts, _P)
_BUILDERS["duels"] = duels
_BUILDERS["long-row"] = long_row
for _a in SATURATION:
    _BUILDERS["saturation-%dx(%d,%d)-%s" % (_a[0], _a[1], _a[2], "17x1" if _a[3] else "1x17")] = \
        functools.partial(saturation, *_a)
for _o in ODDS:
    _BUILDERS["start-(%d,%d)" % _o] = functools.partial(start_values, _o)
for _k in TINY_EXPECTED:
    _BUILDERS["tiny-" + _k] = functools.partial(tiny, _k)
_BUILDERS["borders"] = borders
for _n in PRODUCE:
    _BUILDERS["produce-" + _n] = functools.partial(produce_case, _n)
_BUILDERS["s300"] = s300

NAMES = tuple(_BUILDERS)
UPDATE_NAMES = tuple(n for n in NAMES if not (n.startswith("produce-") or n == "s300"))
PRODUCE_NAMES = tuple(n for n in NAMES if n not in UPDATE_NAMES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c
