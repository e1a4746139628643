"""CPU checks of the inputs of tests/test_grid_gpu.py (tests/grid_cases.py).

The GPU tests compare the HIP mapper with ``occupancy_oracle`` on hand-placed
cases; here every case is shown to be what it claims: (1) the kernel file
header's closed form, applied to the events an instrumented beam walk records,
equals the oracle on every cell; (2) the relations a case is named for are
present, with their counts (RELATIONS: a case cannot silently stop containing
them); (3) the ordering duels are decided by the beams they name; (4) every
coordinate of a heading-0 case is exact (rational arithmetic gives the same
doubles); (5) the tiniest cases equal grids worked out by hand.

No cell of any case has a hit without a miss: a beam's walk records a miss on
the cell it stops on before the hit, and a walk that leaves the grid records
no hit.  The ``m == 0`` (hit-only) branch of grid_finalize_kernel is therefore
unreachable from ``slam_grid_update_i8``; it stays as the header states it.

Likewise a walk never visits a cell twice, so one beam gives a cell at most one
miss and then at most one hit: the ``step`` field of the kernel's event key
orders nothing the hit bit does not order already.  It must only stay below
the beam index (case ``long-row``).

``grid_ref.global_points_exact`` (the device's global-point rule in rational
arithmetic, no BLAS) is checked bit for bit against the reference's recorded
global points; that test never skips.
"""
from fractions import Fraction

import numpy as np
import pytest

import grid_cases as gc
import grid_ref
import occupancy_oracle as oo

# every non-zero relation count of every case (grid_cases.relations)
RELATIONS = {
    'star-24x40': {'beam exits': 324, 'beam zero length': 1, 'both, last a hit': 89, 'both, last a miss': 24,
                   'contested': 89, 'decided across a block boundary': 36, 'miss only': 847},
    'star-40x24': {'beam exits': 324, 'beam zero length': 1, 'both, last a hit': 89, 'both, last a miss': 24,
                   'contested': 89, 'decided across a block boundary': 38, 'miss only': 847},
    'ragged': {'beam exits': 312, 'beam robot outside': 1, 'beam zero length': 2, 'both, last a hit': 82,
               'both, last a miss': 245, 'contested': 85, 'decided across a block boundary': 8,
               'decided across scans': 9, 'miss on a positive cell': 286, 'miss only': 630, 'saturated above': 71,
               'saturated below': 141, 'untouched': 3},
    'count-1': {'both, last a hit': 1, 'decided within one beam': 1, 'miss only': 19, 'untouched': 940},
    'count-255': {'beam zero length': 2, 'both, last a hit': 130, 'both, last a miss': 125, 'contested': 101,
                  'decided across scans': 38, 'decided within one beam': 83, 'miss only': 457, 'untouched': 248},
    'count-256': {'beam zero length': 2, 'both, last a hit': 130, 'both, last a miss': 126, 'contested': 102,
                  'decided across scans': 38, 'decided within one beam': 83, 'miss only': 456, 'untouched': 248},
    'count-257': {'beam zero length': 2, 'both, last a hit': 131, 'both, last a miss': 126, 'contested': 103,
                  'decided across a block boundary': 1, 'decided across scans': 38, 'decided within one beam': 83,
                  'miss only': 455, 'untouched': 248},
    'count-512': {'beam zero length': 2, 'both, last a hit': 205, 'both, last a miss': 307, 'contested': 191,
                  'decided across a block boundary': 66, 'decided across scans': 46, 'decided within one beam': 98,
                  'miss only': 303, 'untouched': 145},
    'duels': {'beam zero length': 514, 'both, last a hit': 10, 'both, last a miss': 4, 'contested': 7,
              'decided across a block boundary': 2, 'decided across scans': 1, 'decided within one beam': 6,
              'miss only': 32, 'saturated above': 1, 'untouched': 914},
    'long-row': {'both, last a hit': 2, 'contested': 1, 'decided across scans': 1, 'decided within one beam': 1,
                 'miss only': 32798},
    'saturation-130x(1,1)-1x17': {'both, last a hit': 1, 'miss on a positive cell': 4, 'miss only': 11,
                                  'saturated above': 1, 'saturated below': 7, 'untouched': 5},
    'saturation-2x(1,127)-17x1': {'both, last a hit': 1, 'miss on a positive cell': 4, 'miss only': 11,
                                  'saturated below': 7, 'untouched': 5},
    'saturation-3x(127,127)-1x17': {'both, last a hit': 1, 'miss on a positive cell': 4, 'miss only': 11,
                                    'saturated above': 1, 'saturated below': 7, 'untouched': 5},
    'saturation-130x(1,1)-17x1': {'both, last a hit': 1, 'miss on a positive cell': 4, 'miss only': 11,
                                  'saturated above': 1, 'saturated below': 7, 'untouched': 5},
    'start-(1,1)': {'both, last a hit': 18, 'both, last a miss': 18, 'contested': 18, 'decided within one beam': 18,
                    'miss on a positive cell': 56, 'miss only': 126, 'saturated above': 4, 'saturated below': 22,
                    'untouched': 270},
    'start-(3,1)': {'both, last a hit': 18, 'both, last a miss': 18, 'contested': 18, 'decided within one beam': 18,
                    'miss on a positive cell': 56, 'miss only': 126, 'saturated above': 8, 'saturated below': 22,
                    'untouched': 270},
    'start-(5,2)': {'both, last a hit': 18, 'both, last a miss': 18, 'contested': 18, 'decided within one beam': 18,
                    'miss on a positive cell': 56, 'miss only': 126, 'saturated above': 8, 'saturated below': 28,
                    'untouched': 270},
    'start-(1,127)': {'both, last a hit': 18, 'both, last a miss': 18, 'contested': 18,
                      'decided within one beam': 18, 'miss on a positive cell': 56, 'miss only': 126,
                      'saturated above': 4, 'saturated below': 58, 'untouched': 270},
    'start-(127,127)': {'both, last a hit': 18, 'both, last a miss': 18, 'contested': 18,
                        'decided within one beam': 18, 'miss on a positive cell': 56, 'miss only': 126,
                        'saturated above': 16, 'saturated below': 58, 'untouched': 270},
    'tiny-1x1-zero': {'beam zero length': 1, 'both, last a hit': 1, 'decided within one beam': 1},
    'tiny-1x1-exit': {'beam exits': 1, 'miss only': 1},
    'tiny-1x1-hit-then-miss': {'beam exits': 1, 'beam zero length': 1, 'both, last a miss': 1, 'contested': 1},
    'tiny-1x17': {'both, last a hit': 1, 'decided within one beam': 1, 'miss only': 7, 'untouched': 9},
    'tiny-17x1': {'both, last a hit': 1, 'decided within one beam': 1, 'miss only': 7, 'untouched': 9},
    'borders': {'beam exits': 7, 'both, last a hit': 6, 'both, last a miss': 1, 'miss only': 12, 'untouched': 16},
    'produce-single-away': {'beam robot outside': 1, 'untouched': 1},
    'produce-single-self': {'beam zero length': 1, 'both, last a hit': 1, 'decided within one beam': 1},
    'produce-collinear-x': {'beam zero length': 1, 'both, last a hit': 5, 'both, last a miss': 5, 'contested': 4,
                            'decided within one beam': 2},
    'produce-collinear-y': {'beam zero length': 1, 'both, last a hit': 4, 'both, last a miss': 3, 'contested': 3,
                            'decided within one beam': 2},
    'produce-min-larger': {'both, last a hit': 8, 'decided within one beam': 8, 'miss only': 25, 'untouched': 159},
    'produce-min-equal': {'both, last a hit': 8, 'decided within one beam': 8, 'miss only': 25, 'untouched': 48},
    'produce-min-smaller': {'both, last a hit': 8, 'decided within one beam': 8, 'miss only': 25, 'untouched': 48},
    'produce-min-mixed': {'both, last a hit': 8, 'decided within one beam': 8, 'miss only': 25, 'untouched': 165},
    'produce-robot-outside': {'beam robot outside': 8, 'both, last a hit': 8, 'decided within one beam': 8,
                              'miss only': 1, 'untouched': 16},
    's300': {'beam zero length': 4, 'both, last a hit': 38, 'both, last a miss': 20, 'contested': 25,
             'decided across scans': 25, 'decided within one beam': 4, 'miss only': 51, 'untouched': 328},
}

# the relations the issue names, and the case that must hold each (count in RELATIONS)
NAMED_FOR = {
    'untouched': 'duels', 'miss only': 'star-24x40', 'both, last a hit': 'duels', 'both, last a miss': 'duels',
    'decided across a block boundary': 'duels', 'decided across scans': 'duels', 'decided within one beam': 'duels',
    'saturated below': 'saturation-130x(1,1)-1x17', 'saturated above': 'saturation-130x(1,1)-1x17',
    'beam exits': 'star-24x40', 'beam robot outside': 'ragged', 'beam zero length': 'star-24x40',
}

# (H, W, min_x, min_y) the reference's arithmetic gives each produce case
PRODUCE_GEOMETRY = {
    'produce-single-away': (1, 1, 0.375, 0.125), 'produce-single-self': (1, 1, 0.375, 0.125),
    'produce-collinear-x': (1, 10, -0.125, -0.125), 'produce-collinear-y': (7, 1, -0.625, -0.125),
    'produce-min-larger': (12, 16, -2.0, -1.5), 'produce-min-equal': (9, 9, -1.125, -1.125),
    'produce-min-smaller': (9, 9, -1.125, -1.125), 'produce-min-mixed': (9, 22, -2.75, -1.125),
    'produce-robot-outside': (5, 5, 1.875, 1.875), 's300': (19, 23, -1.25, -1.0),
}


@pytest.mark.parametrize("name", gc.NAMES)
def test_closed_form_equals_oracle(name):
    """Events of the instrumented walk + the closed form == the oracle's
    sequential int8 updates, on every cell; no cell has a hit without a miss."""
    c = gc.case(name)
    wk = gc.walk(c)
    ref, origin = c.ref
    H, W, min_x, min_y = c.geometry()
    assert ref.shape == (H, W) == wk.shape and ref.dtype == np.int8
    assert origin == (min_x, min_y)
    assert np.array_equal(gc.expected_grid(c, wk), ref)
    for ev in wk.events.values():
        assert any(not e[2] for e in ev)                    # never hit-only
        per_beam = {}
        for g, step, hit in ev:
            per_beam.setdefault(g, []).append((step, hit))
        # one beam: at most a miss, then at most a hit one step later
        assert all(v in ([(k, 0)], [(k, 0), (k + 1, 1)]) for v in per_beam.values() for k in [v[0][0]])
    assert len(wk.beams) == c.P and all(b["steps"] <= H + W for b in wk.beams)


@pytest.mark.parametrize("name", gc.NAMES)
def test_relations(name):
    got = {k: v for k, v in gc.relations(gc.case(name)).items() if v}
    assert got == RELATIONS[name]
    assert "hit only" not in got


def test_every_relation_is_named():
    assert set(RELATIONS) == set(gc.NAMES)
    for rel, name in NAMED_FOR.items():
        assert RELATIONS[name].get(rel, 0) > 0, (rel, name)


@pytest.mark.parametrize("name", gc.NAMES)
def test_coordinates_exact(name):
    """Heading 0: the global points are the exact sums pose + point (no
    rounding anywhere), the oracle's BLAS product gives the same doubles, and
    (but for the one-ulp points of ``borders``) the cell indices are the exact
    floor((p - min) / w)."""
    c = gc.case(name)
    assert np.all(c.poses[:, 2] == 0.0) and c.w in (0.25, 1.0)
    exact = grid_ref.global_points_rational(c.poses, c.scans)
    H, W, min_x, min_y = c.geometry()
    for got, want, blas in zip(c.gpts, exact, oo.global_points(c.poses, c.scans)):
        assert np.array_equal(got, blas)
        for (gx, gy), (fx, fy) in zip(got.tolist(), want):
            assert Fraction(gx) == fx and Fraction(gy) == fy
            if name != "borders":
                assert gc.cell(gx, min_x, c.w) == (fx - Fraction(min_x)) // Fraction(c.w)
                assert gc.cell(gy, min_y, c.w) == (fy - Fraction(min_y)) // Fraction(c.w)


@pytest.mark.parametrize("kind", list(gc.TINY_EXPECTED))
def test_tiny_grids_by_hand(kind):
    c = gc.case("tiny-" + kind)
    assert c.ref[0].tolist() == gc.TINY_EXPECTED[kind]
    assert c.ref[0].shape == {"1x17": (1, 17), "17x1": (17, 1)}.get(kind, (1, 1))


def test_duels():
    """Each duel's cell is reached by exactly the events it names; its result
    is written out by hand in grid_cases.DUELS."""
    c = gc.case("duels")
    wk = gc.walk(c)
    assert c.off.tolist() == [0, 520, 523, 523, 525]            # scan 2 is empty
    assert [b["g"] for b in wk.beams if not b["zero_length"]] == [10, 11, 12, 13, 100, 255, 256, 511, 512, 522, 523]
    for name, ((x, y), first, second, value) in gc.DUELS.items():
        ev = sorted(wk.events[(y, x)])
        win, rival = gc.deciders(ev)
        assert c.ref[0][y, x] == value == (127 if win[2] else -128), name
        if first == second:                                     # one beam alone: miss at k, hit at k + 1
            assert ev == [(first, 5, 0), (first, 6, 1)] and rival is None, name
            continue
        assert win[0] == second and rival[0] == first and win[2] != rival[2], name
        assert {e[0] for e in ev} == {first, second}, name
    d = gc.DUELS
    blocks = [k for k in d if k.startswith("blocks")]
    assert all(d[k][1] // gc.BLOCK + 1 == d[k][2] // gc.BLOCK and d[k][2] == d[k][1] + 1 for k in blocks)
    lanes = [k for k in d if k.startswith("lanes")]
    assert all(d[k][1] // 64 == d[k][2] // 64 and d[k][2] == d[k][1] + 1 for k in lanes)
    k = next(k for k in d if k.startswith("scans"))
    assert (c.scan_of(d[k][1]), c.scan_of(d[k][2])) == (1, 3)
    assert d[k][1] == c.off[2] - 1 and d[k][2] == c.off[3]      # last beam of scan 1, first of scan 3
    # the empty scan's pose is nobody else's: a search that lands on it moves beam 523
    assert not any(np.array_equal(c.poses[2], c.poses[s]) for s in (0, 1, 3))


@pytest.mark.parametrize("name", ["star-24x40", "star-40x24"])
def test_star_directions(name):
    c = gc.case(name)
    wk = gc.walk(c)
    H, W = wk.shape
    assert len(c.scans) == 1 and c.P == 24 + 320 + 4 + 56 + 32 + 1
    inner = [b for b in wk.beams if b["hit"]]
    assert len(inner) == 24 + 56 + 32 + 1

    def direction(b):
        dx, dy = b["end"][0] - b["start"][0], b["end"][1] - b["start"][1]
        return (np.sign(dx), np.sign(dy), np.sign(abs(dx) - abs(dy)))
    # 8 open octants, 4 axis directions, 4 diagonals, and the zero-length beam
    assert len({direction(b) for b in inner}) == 8 + 4 + 4 + 1
    assert sum(b["tie_x"] for b in inner) == 13 and sum(b["tie_y"] for b in inner) == 13       # ring 4, zero length
    # every slope dy / dx with |dx|, |dy| <= 7, both signs
    vectors = {(b["end"][0] - b["start"][0], b["end"][1] - b["start"][1]) for b in inner}
    assert vectors == set(gc.ring(7) + gc.ring(4) + gc.ring(3) + [(0, 0)])
    out = [b for b in wk.beams if b["exits"]]
    last = {b["last_cell"] for b in out}
    assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= last             # through the corners
    for side in (lambda p: p[0] == 0, lambda p: p[0] == W - 1, lambda p: p[1] == 0, lambda p: p[1] == H - 1):
        assert sum(side(p) for p in last) >= 10
    assert all(not (0 <= b["end"][0] < W and 0 <= b["end"][1] < H) for b in out)


def test_ragged_structure():
    c = gc.case("ragged")
    wk = gc.walk(c)
    H, W = wk.shape
    assert tuple(len(s) for s in c.scans) == gc.RAGGED_LENS and c.P == 962
    starts = [next((b["start"] for b in wk.beams if b["scan"] == s), None) for s in range(len(c.scans))]
    assert starts[1] == (-3, 10)                                                # the robot outside
    assert {starts[2], starts[3], starts[4], starts[6]} == {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    assert starts[7] == starts[9] == (W // 2, H // 2)
    outside = [b for b in wk.beams if b["robot_outside"]]
    assert len(outside) == 1 and 0 <= outside[0]["end"][0] < W and 0 <= outside[0]["end"][1] < H
    assert outside[0]["last_cell"] is None                                      # contributes nothing
    # an empty scan's pose differs from the next non-empty scan's
    for s in (0, 5):
        assert not np.array_equal(c.poses[s], c.poses[s + 1])
    assert set(np.unique(c.start).tolist()) == set(gc.START_VALUES)


@pytest.mark.parametrize("P", gc.COUNTS)
def test_counts_last_beam(P):
    c = gc.case(f"count-{P}")
    wk = gc.walk(c)
    H, W = wk.shape
    assert c.P == P
    n = wk.beams[-1]["steps"]
    assert sorted(wk.events[(H - 1, W - 1)]) == [(P - 1, n - 1, 0), (P - 1, n, 1)]
    assert c.ref[0][H - 1, W - 1] == 127


def test_s300_structure():
    c = gc.case("s300")
    assert len(c.scans) == 300 and sum(len(s) == 0 for s in c.scans) == 75 and len(c.scans[299]) == 3
    b = c.bounds()
    assert b.tolist() == [-1.125, 4.375, -0.875, 3.625]
    head = np.concatenate(c.gpts[:256])
    # no extreme is reachable from the first 256 scans, nor from any scan but its own
    assert head[:, 0].min() > b[0] and head[:, 0].max() < b[1] and head[:, 1].min() > b[2] and head[:, 1].max() < b[3]
    for q, (s, col, pick) in enumerate([(260, 0, np.min), (269, 0, np.max), (281, 1, np.min), (299, 1, np.max)]):
        rest = np.concatenate([g for i, g in enumerate(c.gpts) if i != s])
        assert pick(c.gpts[s][:, col]) == b[q] and pick(rest[:, col]) != b[q]
    assert c.gpts[299][-1, 1] == b[3]                            # the very last beam
    assert any(len(c.scans[s]) == 0 for s in range(256, 300))


def test_long_row_steps():
    """Beam 0 reaches the contested cell at a step >= 2^15; the result there is the later beam's hit."""
    c = gc.case("long-row")
    wk = gc.walk(c)
    x = gc.LONG_W - 10
    assert sorted(wk.events[(0, x)]) == [(0, x, 0), (1, 10, 0), (1, 11, 1)] and x >= 1 << 15
    row = c.ref[0][0]
    assert row[-25:].tolist() == [-1] * 5 + [-2] * 10 + [127] + [-1] * 8 + [127]
    assert np.all(row[:-25] == -1)


@pytest.mark.parametrize("odds", gc.ODDS)
def test_start_values_meet_every_relation(odds):
    c = gc.case("start-(%d,%d)" % odds)
    wk = gc.walk(c)
    met = set()
    H, W = wk.shape
    for y in range(H):
        for x in range(W):
            ev = wk.events.get((y, x), [])
            m = sum(1 for e in ev if not e[2])
            h = len(ev) - m
            rel = "untouched" if not ev else "miss" if not h else "last hit" if max(ev)[2] else "last miss"
            met.add((rel, int(c.start[y, x])))
    assert met == {(r, v) for r in ("untouched", "miss", "last hit", "last miss") for v in gc.START_VALUES}
    assert (c.k_hit, c.k_miss) == odds


def test_saturation_values():
    """By hand: 130 misses of 1 take every start value <= 0 to -128, one miss
    takes a positive one there; the endpoint (start -1) ends on its hit."""
    for n, kh, km, vertical in gc.SATURATION:
        c = gc.case("saturation-%dx(%d,%d)-%s" % (n, kh, km, "17x1" if vertical else "1x17"))
        got = c.ref[0].reshape(-1).tolist()
        assert got == [-128] + [-128] * 11 + [127] + list(gc.START_VALUES[4:8]), c.name
        assert n * km > 128


def test_borders_cells():
    c = gc.case("borders")
    wk = gc.walk(c)
    assert [b["end"] for b in wk.beams] == gc.BORDER_CELLS
    assert {b["start"] for b in wk.beams} == {(2, 3)}
    assert [b["exits"] for b in wk.beams] == [not (0 <= x < 7 and 0 <= y < 5) for x, y in gc.BORDER_CELLS]


@pytest.mark.parametrize("name", gc.PRODUCE_NAMES)
def test_produce_geometry(name):
    c = gc.case(name)
    assert tuple(c.geometry()) == PRODUCE_GEOMETRY[name]
    if name == "produce-robot-outside":
        wk = gc.walk(c)
        assert all(b["robot_outside"] == (b["scan"] == 0) for b in wk.beams)
        assert all(e[0] >= 8 for ev in wk.events.values() for e in ev)          # scan 0 leaves the grid untouched
    if name == "produce-single-away":
        assert c.ref[0].tolist() == [[0]]
    if name == "produce-single-self":
        assert c.ref[0].tolist() == [[127]]
    if name == "produce-collinear-x":
        assert c.ref[0].tolist() == [[127, 127, 127, 127, -128, -128, -128, -128, -128, 127]]


def test_shapes_present():
    shapes = {gc.walk(gc.case(n)).shape for n in gc.UPDATE_NAMES}
    assert {(1, 1), (1, 17), (17, 1), (24, 40), (40, 24), (5, 7)} <= shapes


def _fixture_case(g, c):
    off, pts = g[f"off_{c}"], g[f"pts_{c}"]
    return g[f"poses_{c}"], [pts[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_exact_global_points_vs_reference_fixtures(golden):
    """fma(c, x, -s y) + px, spelled with rational arithmetic, equals the
    reference's recorded global points bit for bit, on any NumPy / BLAS build."""
    g = golden("grid_ref.npz")
    n = 0
    for c in range(int(g["n_cases"])):
        poses, scans = _fixture_case(g, c)
        got = np.concatenate(grid_ref.global_points_exact(poses, scans))
        assert np.array_equal(got, g[f"gpts_{c}"]), c
        n += len(got)
    assert n == 2654


def test_rotated_case_is_inexact():
    """The rotated inputs do round: the fused product differs from the plain one somewhere."""
    poses, scans = gc.rotated()
    assert {0.1, -0.1, np.pi / 2, 3.0} <= set(poses[:, 2].tolist())
    assert max(np.abs(np.concatenate(scans)).max(), np.abs(poses[:, :2]).max()) == 1e3
    fused = np.concatenate(grid_ref.global_points_exact(poses, scans))
    plain = np.concatenate([np.stack([np.cos(p[2]) * s[:, 0] - np.sin(p[2]) * s[:, 1] + p[0],
                                      np.sin(p[2]) * s[:, 0] + np.cos(p[2]) * s[:, 1] + p[1]], axis=1)
                            for p, s in zip(poses, scans)])
    assert 10 <= (fused != plain).sum() and np.abs(fused - plain).max() < 1e-12


def test_no_points_is_a_value_error():
    """Scans without a single point: the reference's np.min of an empty array
    raises ValueError, and so does the drop-in (before touching the device)."""
    import src.produce_occupancy_grid as pog
    for kw in ({}, {"min_width": 2.0, "min_height": 1.0}):
        with pytest.raises(ValueError):
            pog.produce_occupancy_grid(np.zeros((2, 3)), [np.zeros((0, 2)), np.zeros((0, 2))], 0.25, **kw)
    with pytest.raises(ValueError):
        oo.produce(np.zeros((2, 3)), [np.zeros((0, 2)), np.zeros((0, 2))], 0.25)
