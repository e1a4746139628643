"""CPU-side checks of the proximity loop-closure search (slamhip.lcd,
csrc/lcd_kernels.hip): the O(N) path rule against the reference's scalar loop,
the C-ABI's argument validation and work-buffer size (no GPU needed), and the
new keyword and command-line flags."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "scripts"))


def _ref_starts(poses, min_dist_along_path):
    # the row loop of /root/reference/src/loop_closure_detection.py:12-19
    dx, dy = poses[:-1, 0] - poses[1:, 0], poses[:-1, 1] - poses[1:, 1]
    walked = np.append([0], np.cumsum(np.sqrt(dx * dx + dy * dy)))
    starts = []
    for i in range(len(poses)):
        s = np.searchsorted(walked, walked[i] + min_dist_along_path, side="right")
        if s >= len(poses):
            break
        starts.append(int(s))
    return starts


@pytest.mark.parametrize("mdp", [2, 5, 1])
def test_path_starts_loop_sequence(mdp):
    from slamhip import lcd, synthetic
    poses = synthetic.make_loop_sequence(700, seed=3, n_beams=11).odometry
    start, n_rows = lcd.path_starts(poses, mdp)
    want = _ref_starts(poses, mdp)
    assert start.dtype == np.int32 and start.shape == (700,)
    assert 0 < n_rows == len(want) < 700
    assert start[:n_rows].tolist() == want
    assert (start[n_rows:] == 700).all()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_path_starts_tiny(n):
    from slamhip import lcd
    poses = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 1.0, 0.0]])[:n]
    for mdp in (2, 1, 0.5):
        start, n_rows = lcd.path_starts(poses, mdp)
        want = _ref_starts(poses, mdp)
        assert n_rows == len(want) and start[:n_rows].tolist() == want and len(start) == n
    assert lcd.path_starts(np.zeros((0, 3)), 2)[1] == 0


def test_path_geometry_matches_cdist():
    """The walked lengths the host rule reads off cdist's diagonal are
    np.sqrt(dx * dx + dy * dy) bit for bit, so both rules see the same starts."""
    import src.loop_closure_detection as host
    from slamhip import synthetic
    poses = synthetic.make_loop_sequence(700, seed=3, n_beams=11).odometry
    _, walked = host._path_geometry(poses)
    dx, dy = poses[:-1, 0] - poses[1:, 0], poses[:-1, 1] - poses[1:, 1]
    assert np.array_equal(walked, np.append([0], np.cumsum(np.sqrt(dx * dx + dy * dy))))


def test_non_finite_and_tiny_inputs_stay_on_the_host():
    from slamhip import lcd
    bad = np.zeros((4, 3))
    for v in (np.nan, np.inf, -np.inf):
        bad[2, 1] = v
        with pytest.raises(ValueError, match="finite"):
            lcd.proximity_candidates_device(bad)
        with pytest.raises(ValueError, match="finite"):
            lcd.path_starts(bad, 2)
        with pytest.raises(ValueError, match="finite"):
            lcd.nearest_after(bad, np.zeros(4, np.int32), 1)
    for n in (0, 1):
        assert lcd.proximity_candidates_device(np.zeros((n, 3))) == []   # returns before anything touches the device
    j, d = lcd.nearest_after(np.zeros((3, 3)), np.zeros(0, np.int32), 0)
    assert j.shape == d.shape == (0,)
    with pytest.raises(ValueError, match="range"):
        lcd.nearest_after(np.zeros((3, 3)), np.array([0, 3], np.int32), 2)
    with pytest.raises(ValueError, match="n_rows"):
        lcd.nearest_after(np.zeros((3, 3)), np.zeros(4, np.int32), 4)


def _call(lib, ptrs, N=10, n_rows=5):
    p = [1 if f else None for f in ptrs]   # never dereferenced: validation fails first
    return lib.slam_lcd_nearest_f64(p[0], N, p[1], n_rows, p[2], p[3], p[4], None)


def test_abi_validation():
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 103
    assert _call(lib, [0] * 5) == -1 and b"null" in lib.slam_last_error()
    for missing in range(5):
        ptrs = [1] * 5
        ptrs[missing] = 0
        assert _call(lib, ptrs) == -1 and b"null" in lib.slam_last_error(), missing
    for kw, word in ((dict(N=0), b"N"), (dict(N=-3), b"N"), (dict(n_rows=-1), b"n_rows"), (dict(n_rows=11), b"n_rows")):
        assert _call(lib, [1] * 5, **kw) == -1
        assert word in lib.slam_last_error(), lib.slam_last_error()
    # no rows: success without a launch (nothing is dereferenced, no device needed)
    assert _call(lib, [1] * 5, n_rows=0) == 0 and lib.slam_last_error() == b""


def test_work_size_is_linear():
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_lcd_work_size(0) == -1 and lib.slam_last_error() != b""
    assert lib.slam_lcd_work_size(-5) == -1
    w50, w100 = lib.slam_lcd_work_size(50000), lib.slam_lcd_work_size(100000)
    assert 0 < w50 < 64 << 20
    assert w100 <= 2.5 * w50
    # at least one (d, j) partial per pose, at most 16 of them, for any N
    for n in (1, 257, 1024, 1025, 6001, 16385, 1 << 20, (1 << 31) - 1):
        assert 12 * n <= lib.slam_lcd_work_size(n) <= 16 * 12 * n + 256, n


def test_unknown_candidate_search_raises():
    import src.loop_closure_detection as host
    with pytest.raises(ValueError, match="candidate"):
        host.detect_proximity(None, [], candidates="bogus")


def test_cli_flags():
    import main_batched as mb
    a = mb.parse(["synthetic:loop:100"])
    assert a.loop_closure_detection == "none"
    assert (a.proximity_min_dist_along_path, a.proximity_max_dist, a.proximity_icp_error) == (2, 1, 110)
    a = mb.parse(["synthetic:loop:100", "--loop-closure-detection", "proximity", "--proximity-min-dist-along-path",
                  "5", "--proximity-max-dist", "0.3", "--proximity-icp-error", "30", "--loop-closure-init", "csm"])
    assert a.loop_closure_detection == "proximity" and a.loop_closure_init == "csm"
    assert (a.proximity_min_dist_along_path, a.proximity_max_dist, a.proximity_icp_error) == (5, 0.3, 30)
    with pytest.raises(SystemExit):
        mb.parse(["synthetic:loop:100", "--loop-closure-detection", "images"])
