"""GPU tests of the proximity loop-closure search (csrc/lcd_kernels.hip,
slamhip.lcd) and of the stage and command-line switch that use it.

The yardstick is the host rule ``src.loop_closure_detection.proximity_candidates``
(the N x N cdist matrix), which tests/test_loop_closure.py pins to the
reference's loop.  Every comparison is exact: the lists of (i, j) are equal,
the distances are the bits of ``np.sqrt(dx * dx + dy * dy)``.
"""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "scripts"))

pytestmark = pytest.mark.gpu


def _host(poses, mdp=2, md=1):
    import src.loop_closure_detection as host
    return host.proximity_candidates(np.asarray(poses, dtype=np.float64), mdp, md)


def _check_rows(poses, mdp):
    """nearest_after against the host matrix, row by row: the first argmin of
    the rounded distances and its bits."""
    from slamhip import lcd
    poses = np.asarray(poses, dtype=np.float64)
    start, n_rows = lcd.path_starts(poses, mdp)
    j, d = lcd.nearest_after(poses, start, n_rows)
    dx = poses[:, None, 0] - poses[None, :, 0]
    dy = poses[:, None, 1] - poses[None, :, 1]
    D = np.sqrt(dx * dx + dy * dy)
    want_j = np.array([s + np.argmin(D[i, s:]) for i, s in enumerate(start[:n_rows])], dtype=np.int64)
    assert j.dtype == np.int64 and np.array_equal(j, want_j)
    assert np.array_equal(d.view(np.uint64), D[np.arange(n_rows), want_j].view(np.uint64))
    return n_rows


def lap_poses(n, seed=11, radius=3.0, step=0.05):
    """Laps of a circle: a radial offset N(0, 0.04) per lap, xy noise N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    s = np.arange(n) * step
    per_lap = 2 * np.pi * radius
    lap = (s // per_lap).astype(int)
    r = radius + rng.normal(0.0, 0.04, size=lap.max() + 1)[lap]
    a = s / radius
    xy = np.stack([r * np.cos(a), r * np.sin(a)], axis=1) + rng.normal(0.0, 0.01, size=(n, 2))
    return np.c_[xy, a]


@pytest.mark.parametrize("n, mdp, md, count", [(257, 2, 1, 0), (700, 2, 1, 191), (2000, 2, 1, 1493),
                                               (700, 5, 0.3, None), (700, 1, 2.5, None)])
def test_loop_sequences(n, mdp, md, count):
    """Sizes that are no multiple of the wave, the row block (256) or the LDS
    tile (1,024); 2,000 poses span two column chunks; the tail rows have
    start == N."""
    from slamhip import lcd, synthetic
    poses = synthetic.make_loop_sequence(n, seed=3, n_beams=11).odometry
    want = _host(poses, mdp, md)
    if count is not None:
        assert len(want) == count
    assert lcd.proximity_candidates_device(poses, mdp, md) == want
    assert 0 < _check_rows(poses, mdp) < n   # every row searched, also where there is no candidate


def test_many_chunks_and_row_blocks():
    """6,001 poses: 24 row blocks of 256 rows over 6 column chunks of one
    1,024-column tile each (the chunk grows past 1,024 columns only above
    16,384 poses), so most row blocks merge several chunks, skip the chunks left
    of their starts and take both the masked and the open tile loop."""
    from slamhip import lcd
    poses = lap_poses(6001)
    want = _host(poses)
    assert len(want) == 5643 and want[-1] == (0, 4147)
    assert lcd.proximity_candidates_device(poses) == want
    _check_rows(poses, 2)


def test_chunks_of_several_tiles():
    """Above 16,384 poses a chunk holds more than one LDS tile: 16,500 poses
    are 9 chunks of 2 tiles, the last a tile of 116 columns.  Checked on a
    sample of rows against the host rule (the full matrix would be 2 GB)."""
    from slamhip import lcd
    poses = lap_poses(16500, seed=12)
    start, n_rows = lcd.path_starts(poses, 2)
    j, d = lcd.nearest_after(poses, start, n_rows)
    rows = np.unique(np.r_[0, 1, 255, 256, 257, n_rows - 2, n_rows - 1,
                           np.random.default_rng(0).integers(0, n_rows, 600)])
    for i in rows:
        dx, dy = poses[i, 0] - poses[start[i]:, 0], poses[i, 1] - poses[start[i]:, 1]
        row = np.sqrt(dx * dx + dy * dy)
        assert j[i] == start[i] + np.argmin(row), i
        assert d[i] == row.min(), i


def test_exact_ties_first_index_wins():
    """A 12 x 12 serpentine lattice at 0.5 m: many poses at exactly equal
    distances; the earliest wins."""
    from slamhip import lcd
    pts = []
    for yy in range(12):
        xs = range(12) if yy % 2 == 0 else range(11, -1, -1)
        pts += [(0.5 * xx, 0.5 * yy, 0.0) for xx in xs]
    poses = np.array(pts)
    want = _host(poses)
    assert len(want) == 130
    assert lcd.proximity_candidates_device(poses) == want
    _check_rows(poses, 2)


def test_square_roots_that_collapse():
    """Pose 2 is further from pose 0 than pose 4 in s (1 + 2^-52 against 1)
    but both distances round to 1.0, and pose 2 comes first; a search that
    compares squares answers (0, 4)."""
    from slamhip import lcd
    poses = np.array([(0, 0, 0), (50, 0, 0), (1, 2.0 ** -26, 0), (50, 50, 0), (1, 0, 0)], dtype=np.float64)
    assert _host(poses, 2, 1.5) == [(2, 4), (0, 2)]
    assert lcd.proximity_candidates_device(poses, 2, 1.5) == [(2, 4), (0, 2)]
    start, n_rows = lcd.path_starts(poses, 2)
    j, d = lcd.nearest_after(poses, start, n_rows)
    assert j[0] == 2 and d[0] == 1.0


def test_edge_inputs_repeat_and_stream():
    import torch
    from slamhip import lcd
    for n in (0, 1, 2):
        assert lcd.proximity_candidates_device(np.zeros((n, 3))) == []
    assert lcd.proximity_candidates_device(np.array([[0.0, 0, 0], [0.5, 0, 0]]), 0.1, 1) == [(0, 1)]
    bad = lap_poses(300)
    for v in (np.nan, np.inf):
        bad[77, 0] = v
        with pytest.raises(ValueError, match="finite"):
            lcd.proximity_candidates_device(bad)
    poses = lap_poses(2500, seed=5)
    start, n_rows = lcd.path_starts(poses, 2)
    j0, d0 = lcd.nearest_after(poses, start, n_rows)
    j1, d1 = lcd.nearest_after(poses, start, n_rows)
    assert np.array_equal(j0, j1) and np.array_equal(d0.view(np.uint64), d1.view(np.uint64))
    j2, d2 = lcd.nearest_after(poses, start, n_rows, stream=torch.cuda.Stream())
    assert np.array_equal(j0, j2) and np.array_equal(d0.view(np.uint64), d2.view(np.uint64))
    # fewer rows than the path rule gives, and starts in any order, are the caller's choice
    rng = np.random.default_rng(1)
    some = rng.integers(0, 2500, size=1000).astype(np.int32)
    j3, d3 = lcd.nearest_after(poses, some, 1000)
    for i in (0, 1, 255, 256, 999):
        dx, dy = poses[i, 0] - poses[some[i]:, 0], poses[i, 1] - poses[some[i]:, 1]
        row = np.sqrt(dx * dx + dy * dy)
        assert j3[i] == some[i] + np.argmin(row) and d3[i] == row.min()


class _Graph:
    def __init__(self, poses):
        self.poses = poses
        self.added = []

    def add_constraint(self, i, j, tf):
        self.added.append((i, j, np.array(tf)))


@pytest.fixture(scope="module")
def wiring():
    """make_loop_sequence(700, seed=5, n_beams=361) and the constraints the
    default detect_proximity (host candidates) adds to it."""
    import src.loop_closure_detection as host
    from slamhip import synthetic
    seq = synthetic.make_loop_sequence(700, seed=5, n_beams=361)
    g = _Graph(seq.odometry.copy())
    host.detect_proximity(g, seq.scans, min_dist_along_path=2, max_dist=1, err_thresh=110)
    assert len(g.added) > 3
    return seq, g.added


def test_detect_proximity_device_candidates(wiring):
    import src.loop_closure_detection as host
    seq, want = wiring
    g = _Graph(seq.odometry.copy())
    host.detect_proximity(g, seq.scans, min_dist_along_path=2, max_dist=1, err_thresh=110, candidates="device")
    assert [(i, j) for i, j, _ in g.added] == [(i, j) for i, j, _ in want]
    for (_, _, a), (_, _, b) in zip(g.added, want):
        assert np.array_equal(a, b)


def test_pipeline_stage_on_resident_scans(wiring):
    from slamhip import icp, pipeline
    seq, want = wiring
    g = _Graph(seq.odometry.copy())
    ss = icp.ScanSet(seq.scans)
    cand, accepted = pipeline.proximity_loop_closures(g, seq.scans, scanset=ss)
    assert cand == _host(seq.odometry) and accepted.shape == (len(cand),) and accepted.dtype == bool
    assert [(i, j) for i, j, _ in g.added] == [(i, j) for i, j, _ in want] == \
        [c for c, ok in zip(cand, accepted) if ok]
    assert accepted.sum() > 3
    for (_, _, a), (_, _, b) in zip(g.added, want):
        assert np.abs(a - b).max() <= 1e-9
    with pytest.raises(ValueError, match="init"):
        pipeline.proximity_loop_closures(g, seq.scans, scanset=ss, init="bogus")


def test_cli_proximity(tmp_path):
    """The whole driver at the default 1081 beams, 1,200 scans (2.3 laps)."""
    import main_batched as mb
    rep = mb.run(mb.parse(["synthetic:loop:1200:3", "--loop-closure-detection", "proximity",
                           "--results-dir", str(tmp_path), "--skip-occupancy-grid"]))
    det = rep["loop_closure_detection"]
    assert det["candidates"] > 0 and det["accepted"] > 0 and det["s"] >= 0
    assert "optimization_s" in rep and (tmp_path / "optim.g2o").exists()
    edges = [line.split()[1:3] for line in open(tmp_path / "loop_closure_pose_graph.g2o")
             if line.startswith("EDGE_SE2")]
    loops = [(int(a), int(b)) for a, b in edges if abs(int(a) - int(b)) > 1]
    assert len(loops) == det["accepted"]
