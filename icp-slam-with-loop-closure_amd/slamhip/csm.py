"""Batched correlative scan matching on the GPU (kernels in
csrc/csm_kernels.hip): an initial guess for loop-closure ICP that does not
need the two scans to share a heading.

The reference starts every loop-closure ICP from the identity
(``scripts/main.py:298-307``, ``src/loop_closure_detection.py:33-35`` and
``:136-142``), which works only while both scans were taken with nearly the
same heading.  ``csm_batch`` searches, for B pairs in one launch, every
rotation of ``n_theta`` bins and every shift of an ``ny`` x ``nx`` window of
``res``-wide cells around a search centre for the pose of the query scan that
puts most of its points on (2) or next to (1) cells occupied by the reference
scan (Olson 2009, brute force, single resolution).  The scores are integer
sums, so the result is the same for any launch shape; ties go to the smallest
flat index ``(k * ny + j) * nx + i``.  include/slamhip.h states the exact
definition; tests/csm_ref.py restates it in NumPy.  A call takes a transient
workspace of (G + 2 ny) x (G + 2 nx + 4) bytes per pair (0.39 MiB at the
defaults).

The result follows ``icp(pc1=query, pc2=reference)``: ``tf @ query ~ reference``,
so ``tf`` is the ``init_transform`` of that ICP call.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv
from . import icp as _icp


@dataclass(frozen=True)
class CsmParams:
    res: float = 0.05                   # cell width (m)
    G: int = 512                        # cells per side of the look-up table (even); origin -(G // 2) * res
    n_theta: int = 240                  # angle bins: th0 + (k - n_theta // 2) * d_theta
    d_theta: float = 2 * np.pi / 240    # angle bin spacing (rad)
    nx: int = 61                        # shift window in cells: tx0 + (i - nx // 2) * res
    ny: int = 61


@dataclass
class CsmResult:
    tf: np.ndarray            # (B, 3, 3) best transform, query -> reference frame
    score: np.ndarray         # (B,) int32 best score (at most 2 * n_query)
    n_query: np.ndarray       # (B,) query points
    index: np.ndarray         # (B, 3) int32 (k, j, i) of the best score
    scores: np.ndarray = None  # (B, n_theta, ny, nx) int32 when requested


def rotations(centre, params):
    """(B, n_theta, 2) cos / sin of every pair's angle bins: ``np.cos`` /
    ``np.sin`` of the Python float, one scalar call per distinct angle (as
    ``slamhip.grid.pose4``: no SIMD-path rounding differences)."""
    half = params.n_theta // 2
    d = float(params.d_theta)
    out = np.empty((len(centre), params.n_theta, 2))
    rows = {}
    for b, th0 in enumerate(centre[:, 0]):
        th0 = float(th0)
        if th0 not in rows:
            rows[th0] = [(np.cos(th0 + (k - half) * d), np.sin(th0 + (k - half) * d))
                         for k in range(params.n_theta)]
        out[b] = rows[th0]
    return out


def _check_params(p):
    if not (np.isfinite(p.res) and p.res > 0):
        raise ValueError(f"csm: res must be positive, got {p.res}")
    if p.G <= 0 or p.G % 2:
        raise ValueError(f"csm: G must be positive and even, got {p.G}")
    if p.n_theta <= 0 or p.nx <= 0 or p.ny <= 0:
        raise ValueError(f"csm: n_theta, nx, ny must be positive, got {p.n_theta}, {p.nx}, {p.ny}")
    if not np.isfinite(p.d_theta):
        raise ValueError("csm: d_theta must be finite")


def check_offsets(off, n_points, n_scans=None):
    """Raises ValueError unless ``off`` are the offsets of ``n_scans`` packed
    scans (any number when None) within ``n_points`` points: one-dimensional
    integers, ``n_scans + 1`` of them, the first at least 0, non-decreasing,
    the last at most ``n_points``.  The kernels read ``scan_off`` unchecked."""
    off = np.asarray(off)
    if off.ndim != 1 or len(off) < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("csm: scan offsets must be a non-empty 1-D integer array")
    if n_scans is not None and len(off) != n_scans + 1:
        raise ValueError(f"csm: {len(off)} scan offsets for {n_scans} scans")
    if off[0] < 0:
        raise ValueError(f"csm: first scan offset {int(off[0])} < 0")
    if np.any(off[1:] < off[:-1]):
        s = int(np.argmax(off[1:] < off[:-1]))
        raise ValueError(f"csm: scan offsets decrease at scan {s} ({int(off[s])} > {int(off[s + 1])})")
    if off[-1] > n_points:
        raise ValueError(f"csm: last scan offset {int(off[-1])} exceeds the {int(n_points)} points")


def csm_batch(scans, src, dst, centre=None, params=CsmParams(), return_scores=False, device=None, stream=None):
    """Correlative scan match of B pairs (query ``src[b]`` against reference
    ``dst[b]``) over a list of scans or a ``slamhip.icp.ScanSet`` (one made by
    ``slamhip.plicp.packed_scans`` too: its offsets are checked here, on the
    host, and empty scans score 0 everywhere); ``centre`` (B, 3) holds the
    search centres (theta0, tx0, ty0), zeros by default.  Returns a CsmResult."""
    _check_params(params)
    ss = scans if isinstance(scans, _icp.ScanSet) else _icp.ScanSet(scans, device)
    check_offsets(ss.off, len(ss.host_pts), len(ss))
    if not np.all(np.isfinite(ss.host_pts)):
        raise ValueError("non-finite scan points")
    src = np.asarray(src, dtype=np.int32)
    dst = np.asarray(dst, dtype=np.int32)
    if src.shape != dst.shape or src.ndim != 1:
        raise ValueError("src/dst must be equal-length 1-D index arrays")
    B, S = len(src), len(ss)
    if B and (src.min() < 0 or dst.min() < 0 or src.max() >= S or dst.max() >= S):
        raise ValueError("scan index out of range")
    centre = np.zeros((B, 3)) if centre is None else np.asarray(centre, dtype=np.float64).reshape(B, 3)
    if not np.all(np.isfinite(centre)):
        raise ValueError("non-finite search centre")
    p = params
    shape = (B, p.n_theta, p.ny, p.nx)
    if B == 0:
        return CsmResult(np.zeros((0, 3, 3)), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3), np.int32),
                         np.zeros(shape, np.int32) if return_scores else None)
    rot = rotations(centre, p)
    L = _abi.lib()
    n_work = int(L.slam_csm_work_size(B, p.G, p.n_theta, p.ny, p.nx))
    if n_work < 0:
        _abi.check(n_work, "slam_csm_work_size")
    dev = ss.device
    d_src = dv.to_dev(src, np.int32, dev)
    d_dst = dv.to_dev(dst, np.int32, dev)
    d_centre = dv.to_dev(centre, np.float64, dev)
    d_rot = dv.to_dev(rot, np.float64, dev)
    work = dv.empty((n_work,), np.uint8, dev)
    best = dv.empty((B, 4), np.int32, dev)
    scores = dv.empty(shape, np.int32, dev) if return_scores else None
    _abi.check(L.slam_csm_batch(
        dv.ptr(ss.pts), dv.ptr(ss.scan_off), dv.ptr(d_src), dv.ptr(d_dst), dv.ptr(d_centre), dv.ptr(d_rot), B,
        float(p.res), int(p.G), int(p.n_theta), int(p.nx), int(p.ny), dv.ptr(best), dv.ptr(scores), dv.ptr(work),
        dv.stream_handle(stream)), "slam_csm_batch")
    if stream is not None:
        stream.synchronize()
    h = best.cpu().numpy()
    return CsmResult(assemble(centre, rot, h[:, 1:], p), h[:, 0].copy(), ss.lens[src].copy(), h[:, 1:].copy(),
                     scores.cpu().numpy() if return_scores else None)


def assemble(centre, rot, index, params):
    """(B, 3, 3) transforms of the bins ``index`` (B, 3) = (k, j, i)."""
    B = len(index)
    tf = np.zeros((B, 3, 3))
    for b, (k, j, i) in enumerate(index):
        c, s = rot[b, k]
        tf[b] = [[c, -s, centre[b, 1] + (int(i) - params.nx // 2) * params.res],
                 [s, c, centre[b, 2] + (int(j) - params.ny // 2) * params.res],
                 [0.0, 0.0, 1.0]]
    return tf
