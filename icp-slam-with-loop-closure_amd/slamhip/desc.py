"""Batched matching of ORB descriptors on the GPU (kernel in
csrc/desc_kernels.hip): everything the reference's image loop-closure detector
(``src/loop_closure_detection.py:81-131``) does between the descriptors and the
list of image pairs handed to ICP.

The reference matches every image pair (i, j >= start[i]) with OpenCV on a
joblib pool (``matchify``, :61-79) and sums the ``n_matches`` best match
distances into ``dist_mat[i, j]``.  Here the descriptors are packed once into a
resident ``DescriptorSet`` and all pairs are matched in one launch, one
workgroup per pair.  include/slamhip.h states the rule (``hamming``: the
cross-checked brute-force matcher of ``approximate_match=False``; ``l2``: the
exact search the default FLANN kd-tree approximates); tests/desc_ref.py
restates it in NumPy and tests/test_desc_gpu.py compares bit for bit.  ORB
keypoint extraction stays OpenCV's; nothing here imports it.
"""
import numpy as np

from . import _abi
from . import device as dv

METRICS = {"hamming": 0, "l2": 1}
MAX_MATCHES = 256


class DescriptorSet:
    """The descriptors of M images, packed and resident on the device.

    ``descriptors``: one (n, 32) uint8 array per image; ``None`` or an empty
    array for an image without keypoints."""

    def __init__(self, descriptors, device=None):
        rows = []
        for m, d in enumerate(descriptors):
            if d is None:
                d = np.zeros((0, 32), np.uint8)
            d = np.asarray(d)
            if d.size == 0:
                d = np.zeros((0, 32), np.uint8)
            if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 32:
                raise ValueError(f"image {m}: descriptors must be (n, 32) uint8, got {d.dtype} {d.shape}")
            rows.append(d)
        if not rows:
            raise ValueError("no images")
        self.counts = np.array([len(d) for d in rows], dtype=np.int64)
        self.off = np.zeros(len(rows) + 1, dtype=np.int64)
        self.off[1:] = np.cumsum(self.counts)
        packed = np.concatenate(rows, axis=0) if self.off[-1] else np.zeros((0, 32), np.uint8)
        self.host = packed
        self.device = device if device is not None else dv.default_device()
        # at least one row: an empty allocation has no pointer to pass
        self.d_desc = dv.to_dev(packed if len(packed) else np.zeros((1, 32), np.uint8), np.uint8, self.device)
        self.d_off = dv.to_dev(self.off, np.int64, self.device)

    def __len__(self):
        return len(self.counts)

    def image(self, m):
        return self.host[self.off[m]:self.off[m + 1]]


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"unknown descriptor metric {metric!r} ({' | '.join(METRICS)})")
    return METRICS[metric]


def match_pairs(ds, qi, ti, n_matches, metric="hamming", return_matches=False, stream=None):
    """Match image ``qi[b]`` (query) against ``ti[b]`` (train) for every b in
    one launch: ``(score float64[B], count int64[B])`` and, with
    ``return_matches``, ``matches int64[B][n_matches][3]`` rows (a, b, d)
    (slam_desc_match_batch).  An image index outside the set raises
    ``SlamHipError`` with status -1 (the kernel's own check), a set with an
    image of more than 4,096 descriptors with status -3."""
    code = _metric(metric)
    n_matches = int(n_matches)
    if not 1 <= n_matches <= MAX_MATCHES:
        raise ValueError(f"n_matches = {n_matches} outside 1..{MAX_MATCHES}")
    qi, ti = np.asarray(qi, dtype=np.int64).ravel(), np.asarray(ti, dtype=np.int64).ravel()
    if len(qi) != len(ti):
        raise ValueError(f"{len(qi)} query images for {len(ti)} train images")
    B = len(qi)
    if B >= 1 << 31:
        raise ValueError("more than 2^31 - 1 pairs")
    if B == 0:
        out = (np.zeros(0), np.zeros(0, np.int64))
        return out + (np.zeros((0, n_matches, 3), np.int64),) if return_matches else out
    lim = np.iinfo(np.int32)
    L = _abi.lib()
    n_work = int(L.slam_desc_work_size(B, int(ds.counts.max()), n_matches))
    if n_work < 0:
        _abi.check(n_work, "slam_desc_work_size")
    dev = ds.device
    d_qi = dv.to_dev(np.clip(qi, lim.min, lim.max), np.int32, dev)   # an index beyond int32 stays out of range
    d_ti = dv.to_dev(np.clip(ti, lim.min, lim.max), np.int32, dev)
    work = dv.empty((n_work,), np.uint8, dev)
    out_s = dv.empty((B,), np.float64, dev)
    out_c = dv.empty((B,), np.int32, dev)
    out_m = dv.empty((B, n_matches, 3), np.int32, dev) if return_matches else None
    h = dv.stream_handle(stream)
    _abi.check(L.slam_desc_match_batch(dv.ptr(ds.d_desc), dv.ptr(ds.d_off), len(ds), dv.ptr(d_qi), dv.ptr(d_ti), B,
                                       code, n_matches, dv.ptr(out_s), dv.ptr(out_c), dv.ptr(out_m), dv.ptr(work), h),
               "slam_desc_match_batch")
    _abi.check(L.slam_desc_status(h), "slam_desc_match_batch")
    out = (out_s.cpu().numpy(), out_c.cpu().numpy().astype(np.int64))
    return out + (out_m.cpu().numpy().astype(np.int64),) if return_matches else out


def similarity_matrix(ds, start, n_matches, metric="hamming"):
    """The reference's ``dist_mat`` (:103-110): (M, M) float64, entry (i, j)
    the match score of images i and j for ``start[i] <= j < M`` — all of them
    matched in one launch — and ``inf`` elsewhere."""
    _metric(metric)
    M = len(ds)
    start = np.asarray(start, dtype=np.int64).ravel()
    if len(start) != M:
        raise ValueError(f"{len(start)} starts for {M} images")
    if M and start.min() < 0:
        raise ValueError("negative start")
    lo = np.minimum(start, M)
    qi = np.repeat(np.arange(M), M - lo)
    ti = np.concatenate([np.arange(s, M) for s in lo]) if M else np.zeros(0, np.int64)
    out = np.full((M, M), np.inf)
    if len(qi):
        out[qi, ti] = match_pairs(ds, qi, ti, n_matches, metric)[0]
    return out


def select_matches(dist_mat, image_err_thresh):
    """The reference's column rule (:126-131): for every image j the row
    ``i = argmin(dist_mat[:, j])``, kept when ``dist_mat[i, j] <
    image_err_thresh``.  A list of (i, j), in column order."""
    dist_mat = np.asarray(dist_mat, dtype=np.float64)
    if dist_mat.ndim != 2:
        raise ValueError(f"dist_mat must be a matrix, got shape {dist_mat.shape}")
    good = []
    if dist_mat.shape[0] == 0:
        return good
    for j in range(dist_mat.shape[1]):
        i = int(np.argmin(dist_mat[:, j]))
        if dist_mat[i, j] < image_err_thresh:
            good.append((i, j))
    return good


def image_starts(poses, min_dist_along_path=5, image_rate=1):
    """``start_idx`` of the reference (:84-91): for image m (scan m *
    image_rate) the first image at least ``min_dist_along_path`` further along
    the path, as ``floor(start[::image_rate] / image_rate)`` of the per-scan
    ``np.searchsorted(..., side="right")`` — quirk included: only a scan start
    equal to the number of scans is scaled by ``image_rate`` first, so a start
    between two images rounds DOWN to the earlier one."""
    from .lcd import path_starts
    image_rate = int(image_rate)
    if image_rate < 1:
        raise ValueError(f"image_rate = {image_rate} < 1")
    start = path_starts(poses, min_dist_along_path)[0].astype(np.int64)
    start[start == len(start)] = start[start == len(start)] * image_rate
    return np.floor(start[::image_rate] / image_rate).astype(int)
