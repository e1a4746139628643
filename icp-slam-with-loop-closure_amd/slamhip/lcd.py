"""Proximity loop-closure candidates on the GPU (kernels in
csrc/lcd_kernels.hip): the candidate search of the reference's
``detect_proximity`` (``src/loop_closure_detection.py:12-24``) without the
N x N distance matrix.

The reference pairs every pose i with the nearest pose j among those at least
``min_dist_along_path`` further along the path and keeps the pair when they lie
within ``max_dist``.  It, and the drop-in's host path
(``src.loop_closure_detection.proximity_candidates``), take both from a
``scipy.spatial.distance.cdist`` matrix: 20 GB at 50,000 poses.  Here the path
rule is an O(N) host pass (``path_starts``) and the nearest pose a HIP kernel
over O(N) memory (``nearest_after``).  The answers are the host rule's bit for
bit: ``d = np.sqrt(dx * dx + dy * dy)``, the smallest j among equal d
(include/slamhip.h states the rule; tests/test_lcd_gpu.py compares the lists).
"""
import numpy as np

from . import _abi
from . import device as dv


def _xy_theta(poses):
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2:
        raise ValueError(f"poses must be (N, 3) rows of (x, y, theta), got shape {p.shape}")
    if not np.all(np.isfinite(p[:, :2])):
        raise ValueError("non-finite poses")
    return p


def path_starts(poses, min_dist_along_path):
    """``(start int32[N], n_rows)``: ``start[i]`` is the first pose at least
    ``min_dist_along_path`` further along the path than pose i (reference :13,
    :17: ``np.searchsorted(walked, walked[i] + min_dist_along_path,
    side="right")``), N where there is none; ``n_rows`` counts the leading
    rows with ``start < N`` (the reference's loop breaks at the first other)."""
    p = _xy_theta(poses)
    N = len(p)
    if N == 0:
        return np.zeros(0, np.int32), 0
    dx, dy = p[:-1, 0] - p[1:, 0], p[:-1, 1] - p[1:, 1]
    walked = np.append([0], np.cumsum(np.sqrt(dx * dx + dy * dy)))
    start = np.searchsorted(walked, walked + min_dist_along_path, side="right")
    past = start >= N
    n_rows = int(np.argmax(past)) if past.any() else N
    return start.astype(np.int32), n_rows


def nearest_after(poses, start, n_rows, device=None, stream=None):
    """``(j int64[n_rows], d float64[n_rows])``: for every row i < n_rows the
    smallest j in [start[i], N) at the least distance from pose i, and that
    distance (slam_lcd_nearest_f64)."""
    p = _xy_theta(poses)
    N, n_rows = len(p), int(n_rows)
    start = np.asarray(start)
    if not 0 <= n_rows <= N or start.ndim != 1 or len(start) < n_rows:
        raise ValueError(f"n_rows = {n_rows} needs 0 <= n_rows <= N = {N} and that many starts")
    start = start[:n_rows]
    if n_rows and (start.min() < 0 or start.max() >= N):
        raise ValueError("start out of range [0, N)")
    if n_rows == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    if N >= 1 << 31:
        raise ValueError("more than 2^31 - 1 poses")
    xyt = np.zeros((N, 3))
    xyt[:, :min(3, p.shape[1])] = p[:, :3]
    L = _abi.lib()
    n_work = int(L.slam_lcd_work_size(N))
    if n_work < 0:
        _abi.check(n_work, "slam_lcd_work_size")
    dev = device if device is not None else dv.default_device()
    d_poses = dv.to_dev(xyt, np.float64, dev)
    d_start = dv.to_dev(start, np.int32, dev)
    work = dv.empty((n_work,), np.uint8, dev)
    out_j = dv.empty((n_rows,), np.int32, dev)
    out_d = dv.empty((n_rows,), np.float64, dev)
    _abi.check(L.slam_lcd_nearest_f64(dv.ptr(d_poses), N, dv.ptr(d_start), n_rows, dv.ptr(out_j), dv.ptr(out_d),
                                      dv.ptr(work), dv.stream_handle(stream)), "slam_lcd_nearest_f64")
    if stream is not None:
        stream.synchronize()
    return out_j.cpu().numpy().astype(np.int64), out_d.cpu().numpy()


def proximity_candidates_device(poses, min_dist_along_path=2, max_dist=1, device=None):
    """The (i, j) pairs of ``src.loop_closure_detection.proximity_candidates``
    (reference :12-24, in the order the greedy pass visits them), searched on
    the GPU."""
    p = _xy_theta(poses)
    if len(p) < 2:
        return []
    start, n_rows = path_starts(p, min_dist_along_path)
    if n_rows == 0:
        return []
    j, d = nearest_after(p, start, n_rows, device)
    rows = np.nonzero(d <= max_dist)[0]
    out = [(int(i), int(j[i])) for i in rows]
    out.reverse()
    return out
