"""Point-to-line refinement of ICP edges on the GPU (kernels in
csrc/plicp_kernels.hip).

The reference's ICP is point-to-point: it pulls every point towards the nearest
*sample* of the other scan, so its result is biased along the walls by up to
half the beam spacing, and the bias accumulates in the odometry chain.  Here a
finished ICP result is refined with a gated point-to-line metric (the
Gauss-Newton form of Censi's PLICP): every destination point gets the normal of
the surface it lies on (``scan_normals``), a source point within ``max_dist`` of
its nearest destination point contributes its distance to that point's tangent
line (both coordinates where the match has no normal), and the 3x3 normal
equations are solved for a step (x, y, theta) until the step is small.

The reference has no counterpart.  include/slamhip.h states the rule,
tests/plicp_ref.py restates it in NumPy and tests/test_plicp_gpu.py compares.
Everything here is opt-in: no existing call changes what it returns.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv
from .icp import ScanSet, _se2_rows

CONVERGED, MAX_ITERS, DEGENERATE, TOO_FEW = 0, 1, 2, 3
STATUS_NAMES = ("CONVERGED", "MAX_ITERS", "DEGENERATE", "TOO_FEW")
MAX_QUERY_POINTS = 8192


@dataclass(frozen=True)
class PlicpParams:
    max_dist: float = 0.5        # m: the correspondence gate
    min_inliers: int = 10        # fewer inliers than this: TOO_FEW
    max_iters: int = 50
    eps_t: float = 5e-4          # m: a step below (eps_t, eps_t, eps_r) ends the refinement.  At 1e-6 two of twenty
    eps_r: float = 5e-4          # rad: pairs cycled at about 2.5e-4 m, far below the 10 mm range noise
    pivot_tol: float = 1e-9      # a pivot d_k <= pivot_tol H_kk: DEGENERATE
    normal_k: int = 8            # neighbours per side that support a normal
    normal_rho: float = 0.15     # m: the support radius
    corner_tol: float = 0.03     # m: a point this far off its support's chord is a corner and has no normal

    def __post_init__(self):
        tol = (self.max_dist, self.eps_t, self.eps_r, self.pivot_tol, self.normal_rho, self.corner_tol)
        if not all(np.isfinite(float(v)) and float(v) >= 0 for v in tol):
            raise ValueError(f"tolerances {tol}: finite and >= 0 expected")
        if int(self.max_iters) < 1 or int(self.normal_k) < 1 or int(self.min_inliers) < 0:
            raise ValueError(f"max_iters = {self.max_iters} >= 1, normal_k = {self.normal_k} >= 1 and "
                             f"min_inliers = {self.min_inliers} >= 0 expected")

    @property
    def normals_key(self):
        return (int(self.normal_k), float(self.normal_rho), float(self.corner_tol))


@dataclass
class PlicpResult:
    tf: np.ndarray         # (B, 3, 3) refined transforms (the input where status is DEGENERATE or TOO_FEW)
    err: np.ndarray        # (B,) mean squared residual per inlier of the last linearisation
    obs: np.ndarray        # (B,) observability of the translation, 0 (corridor) .. 1 (room), same linearisation
    inliers: np.ndarray    # (B,) int64: inliers of the same linearisation
    iters: np.ndarray      # (B,) int64: steps taken
    status: np.ndarray     # (B,) int64: CONVERGED, MAX_ITERS, DEGENERATE or TOO_FEW
    match: list = None     # B int32 arrays: the matched destination index per source point, -1 for an outlier


def _stream(stream):
    """The handle of ``stream`` (None: the current one), made to wait for the
    work already queued on the current stream: uploads and earlier launches."""
    if stream is not None:
        stream.wait_stream(dv.torch().cuda.current_stream())
    return dv.stream_handle(stream)


def packed_scans(pts, off, device=None):
    """A ``ScanSet`` of scans that are already packed: ``pts`` (P, 2) and ``off``
    (S + 1,) offsets, uploaded as they are (empty scans are allowed, and the
    offsets are checked on the device, scan by scan, not here)."""
    ss = ScanSet.__new__(ScanSet)
    host = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    ss.off = np.asarray(off, dtype=np.int64).copy()
    ss.lens = np.diff(ss.off)
    ss.host_pts = host
    ss.pts = dv.to_dev(host if len(host) else np.zeros((1, 2)), np.float64, device)
    ss.scan_off = dv.to_dev(ss.off, np.int64, ss.pts.device)
    ss.device = ss.pts.device
    return ss


def status(stream=None):
    """Synchronises and raises if a launch since the last call met a scan with
    bad offsets or a pair outside its bounds (slam_plicp_status)."""
    _abi.check(_abi.lib().slam_plicp_status(dv.stream_handle(stream)), "slam_plicp_status")


def scan_normals(scanset, params=None, stream=None, check=True):
    """The (P, 2) float64 device array of unit normals of the resident scans of
    ``scanset`` ((0, 0): none), by slam_plicp_normals_f64: no second upload.
    Cached on the scanset per (normal_k, normal_rho, corner_tol).  ``check``
    false leaves the status to the caller (``status``)."""
    params = params if params is not None else PlicpParams()
    cache = scanset.__dict__.setdefault("_plicp_normals", {})
    key = params.normals_key
    if key in cache:
        return cache[key]
    P = len(scanset.host_pts)
    out = dv.empty((max(P, 1), 2), np.float64, scanset.device)
    if P:
        rho = float(params.normal_rho)
        h = _stream(stream)
        lib = _abi.lib()
        _abi.check(lib.slam_plicp_normals_f64(dv.ptr(scanset.pts), dv.ptr(scanset.scan_off), len(scanset), P,
                                              int(params.normal_k), rho * rho, float(params.corner_tol), dv.ptr(out),
                                              h), "slam_plicp_normals_f64")
        if check:
            _abi.check(lib.slam_plicp_status(h), "slam_plicp_normals_f64")
    cache[key] = out[:P]
    return cache[key]


def refine_batch(scanset, src, dst, init, params=None, normals=None, return_match=False, stream=None, check=True):
    """Refines B transforms ``init`` of icp(pc1 = src[b], pc2 = dst[b]) over the
    resident scans in ONE launch (slam_plicp_batch_f64).  ``normals``: the array
    of ``scan_normals`` (None: taken from the scanset's cache or computed).
    ``check`` false skips the host's index check and leaves the device's flags
    to the caller (``status``): a flagged pair has status -1.  Returns a
    ``PlicpResult``."""
    params = params if params is not None else PlicpParams()
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    if src.shape != dst.shape or src.ndim != 1:
        raise ValueError("src/dst must be equal-length 1-D index arrays")
    S, B = len(scanset), len(src)
    if check and B and (src.min() < 0 or dst.min() < 0 or src.max() >= S or dst.max() >= S):
        raise ValueError("scan index out of range")
    rows = _se2_rows(init, B)
    if B == 0:
        z = np.zeros(0, np.int64)
        return PlicpResult(np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0), z, z.copy(), z.copy(),
                           [] if return_match else None)
    inside = (src >= 0) & (src < S)
    max_n1 = int(max(scanset.lens[src[inside]].max(initial=0), 0))
    if max_n1 > MAX_QUERY_POINTS:
        raise ValueError(f"pc1 of {max_n1} points exceeds the kernel capacity {MAX_QUERY_POINTS}")
    dev = scanset.device
    if normals is None:
        normals = scan_normals(scanset, params, stream)
    P = len(scanset.host_pts)
    if tuple(normals.shape) != (P, 2):
        raise ValueError(f"normals of shape {tuple(normals.shape)} for {P} points")
    d_src = dv.to_dev(src, np.int32, dev)
    d_dst = dv.to_dev(dst, np.int32, dev)
    d_init = dv.to_dev(rows, np.float64, dev)
    out_tf = dv.empty((B, 9), np.float64, dev)
    out_err, out_obs = dv.empty((B,), np.float64, dev), dv.empty((B,), np.float64, dev)
    out_inl, out_it, out_st = (dv.empty((B,), np.int32, dev) for _ in range(3))
    out_match = dv.empty((B, max(max_n1, 1)), np.int32, dev) if return_match else None
    md = float(params.max_dist)
    h = _stream(stream)
    lib = _abi.lib()
    _abi.check(lib.slam_plicp_batch_f64(
        dv.ptr(scanset.pts), dv.ptr(scanset.scan_off), S, P, dv.ptr(normals), dv.ptr(d_src), dv.ptr(d_dst),
        dv.ptr(d_init), B, md * md, int(params.min_inliers), int(params.max_iters), float(params.eps_t),
        float(params.eps_r), float(params.pivot_tol), max_n1, dv.ptr(out_tf), dv.ptr(out_err), dv.ptr(out_obs),
        dv.ptr(out_inl), dv.ptr(out_it), dv.ptr(out_st), dv.ptr(out_match), max(max_n1, 1) if return_match else 0, h),
        "slam_plicp_batch_f64")
    if check:
        _abi.check(lib.slam_plicp_status(h), "slam_plicp_batch_f64")
    match = None
    if return_match:
        mm = out_match.cpu().numpy()
        match = [mm[b, :max(int(scanset.lens[src[b]]), 0) if inside[b] else 0].copy() for b in range(B)]
    return PlicpResult(out_tf.cpu().numpy().reshape(B, 3, 3), out_err.cpu().numpy(), out_obs.cpu().numpy(),
                       out_inl.cpu().numpy().astype(np.int64), out_it.cpu().numpy().astype(np.int64),
                       out_st.cpu().numpy().astype(np.int64), match)


def apply_refinement(tf, n_src, result, min_overlap=0.5, min_observability=0.0):
    """Which refinements to take.  ``tf``: the (B, 3, 3) transforms that were
    refined, ``n_src``: the (B,) source scan sizes, ``result``: the
    ``PlicpResult``.  A pair takes its refined transform where its status is
    CONVERGED or MAX_ITERS, ``inliers >= min_overlap * n_src`` and ``obs >=
    min_observability``; otherwise it keeps its input row bit for bit.  Returns
    (transforms (B, 3, 3), taken (B,) bool).  Host arithmetic only."""
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 3, 3)
    n_src = np.asarray(n_src, dtype=np.float64).reshape(-1)
    if not (len(tf) == len(n_src) == len(result.tf)):
        raise ValueError(f"{len(tf)} transforms, {len(n_src)} sizes and {len(result.tf)} results: one per pair expected")
    with np.errstate(invalid="ignore"):
        take = ((result.status == CONVERGED) | (result.status == MAX_ITERS)) & \
            (result.inliers >= float(min_overlap) * n_src) & (result.obs >= float(min_observability))
    out = tf.copy()
    out[take] = result.tf[take]
    return out, take
