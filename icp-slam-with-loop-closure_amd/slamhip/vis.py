"""Verification of pose-graph edges by scan visibility on the GPU (kernels in
csrc/vis_kernels.hip).

An edge icp(pc1 = src, pc2 = dst) -> T is accepted elsewhere on its ICP error
alone.  Here it is judged geometrically and on its own, without a pose chain:
every point of one scan is mapped through T into the other scan's frame and its
range is compared with the range that scan measured at the same bearing (a
table of the nearest return per sector, ``scan_tables``).  A point on the
measured surface *agrees*; a point well in front of it lies where the other
scan saw free space and *conflicts*; anything else (occluded, outside the field
of view, no return at that bearing: the scans keep no record of beams without
one) is unknown.  Both directions are counted, and ``VisParams.passes`` turns
the six counts into a verdict.

The reference has no counterpart.  include/slamhip.h states the rule,
tests/vis_ref.py restates it in NumPy and tests/test_vis_gpu.py compares.
Everything here is opt-in: no existing call changes what it returns.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv
from .icp import _se2_rows
from .plicp import _stream

MIN_SECTORS, MAX_SECTORS = 3, 1024


@dataclass(frozen=True)
class VisParams:
    sectors: int = 360           # bearings of a scan's range table
    window: int = 1              # sectors to each side of a point's own that are looked at
    margin: float = 0.15         # m: a range within this of the table's agrees, one shorter by more conflicts
    min_agree: float = 0.25      # a direction passes with agree >= min_agree n ...
    max_conflict: float = 0.02   # ... and conflict <= max_conflict (agree + conflict)

    def __post_init__(self):
        S, W = self.sectors, self.window
        if int(S) != S or not MIN_SECTORS <= S <= MAX_SECTORS:
            raise ValueError(f"sectors = {S}: an integer in {MIN_SECTORS}..{MAX_SECTORS} expected")
        if int(W) != W or W < 0 or 2 * W + 1 > S:
            raise ValueError(f"window = {W}: an integer with 0 <= window and 2 window + 1 <= sectors = {S} expected")
        if not (np.isfinite(float(self.margin)) and float(self.margin) >= 0):
            raise ValueError(f"margin = {self.margin}: finite and >= 0 expected")
        for name in ("min_agree", "max_conflict"):
            v = float(getattr(self, name))
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} = {v}: a share in [0, 1] expected")

    @property
    def tables_key(self):
        return (int(self.sectors),)

    def passes(self, counts):
        """The verdict on (B, 6) counts (agree0, conflict0, n0, agree1,
        conflict1, n1): both directions need ``agree_d >= min_agree n_d`` and
        ``conflict_d <= max_conflict (agree_d + conflict_d)``.  An edge with an
        empty scan fails, and so does one the device flagged (counts -1).
        Host arithmetic only."""
        c = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
        a, k, n = c[:, 0::3], c[:, 1::3], c[:, 2::3]
        ok = (n > 0) & (a >= float(self.min_agree) * n) & (k <= float(self.max_conflict) * (a + k))
        return ok.all(axis=1)


@dataclass
class VisResult:
    counts: np.ndarray     # (B, 6) int64: agree0, conflict0, n0, agree1, conflict1, n1 (-1: flagged on the device)
    agree: np.ndarray      # (B, 2) agree_d / n_d (0 for an empty scan)
    conflict: np.ndarray   # (B, 2) conflict_d / (agree_d + conflict_d) (0 where no point is either)
    ok: np.ndarray         # (B,) bool: VisParams.passes


def sector_dirs(sectors):
    """float64[S][2] sector centres (cos, sin)((k + 0.5) 2 pi / S): one scalar
    np.cos / np.sin call per entry, as the signatures' table (``slamhip.sig``)."""
    S = int(sectors)
    return np.array([[np.cos((k + 0.5) * 2 * np.pi / S), np.sin((k + 0.5) * 2 * np.pi / S)] for k in range(S)])


def shares(counts):
    """(agree (B, 2), conflict (B, 2)) shares of (B, 6) counts."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 6).astype(np.float64)
    a, k, n = c[:, 0::3], c[:, 1::3], c[:, 2::3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, a / n, 0.0), np.where(a + k > 0, k / (a + k), 0.0)


def candidate_key(counts, order):
    """Orders the candidate transforms of an edge when none passes: the
    smallest ``(conflict0 + conflict1, -(agree0 + agree1), order)`` is taken."""
    c = np.asarray(counts, dtype=np.int64).reshape(6)
    return (int(c[1] + c[4]), -int(c[0] + c[3]), int(order))


def status(stream=None):
    """Synchronises and raises if a launch since the last call met a scan with
    bad offsets or an edge outside its bounds (slam_vis_status)."""
    _abi.check(_abi.lib().slam_vis_status(dv.stream_handle(stream)), "slam_vis_status")


def _dirs_dev(scanset, S):
    cache = scanset.__dict__.setdefault("_vis_dirs", {})
    if S not in cache:
        cache[S] = dv.to_dev(sector_dirs(S), np.float64, scanset.device)
    return cache[S]


def scan_tables(scanset, params=None, stream=None, check=True):
    """The (n_scans, S) float64 device array of range tables of the resident
    scans of ``scanset`` (the squared range of the nearest return per sector,
    +inf for none), by slam_vis_tables_f64: no second upload.  Cached on the
    scanset per ``(sectors,)``.  ``check`` false leaves the status to the caller
    (``status``)."""
    params = params if params is not None else VisParams()
    cache = scanset.__dict__.setdefault("_vis_tables", {})
    key = params.tables_key
    if key in cache:
        return cache[key]
    n, S = len(scanset), int(params.sectors)
    out = dv.empty((n, S), np.float64, scanset.device)
    if n:
        h = _stream(stream)
        lib = _abi.lib()
        _abi.check(lib.slam_vis_tables_f64(dv.ptr(scanset.pts), dv.ptr(scanset.scan_off), n, len(scanset.host_pts),
                                           dv.ptr(_dirs_dev(scanset, S)), S, dv.ptr(out), h), "slam_vis_tables_f64")
        if check:
            _abi.check(lib.slam_vis_status(h), "slam_vis_tables_f64")
    cache[key] = out
    return out


def check_batch(scanset, src, dst, tf, params=None, tables=None, stream=None, check=True):
    """Counts, for B edges icp(pc1 = src[b], pc2 = dst[b]) -> ``tf[b]`` over
    the resident scans, the agreeing and conflicting points of both directions
    in ONE launch (slam_vis_check_f64).  ``tables``: the array of
    ``scan_tables`` (None: taken from the scanset's cache or computed).
    ``check`` false skips the host's index check and leaves the device's flags
    to the caller (``status``): a flagged edge has counts -1 and fails.
    Returns a ``VisResult``."""
    params = params if params is not None else VisParams()
    if not isinstance(params, VisParams):
        raise TypeError(f"params must be a slamhip.vis.VisParams, got {type(params).__name__}")
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    if src.shape != dst.shape or src.ndim != 1:
        raise ValueError("src/dst must be equal-length 1-D index arrays")
    n, B, S = len(scanset), len(src), int(params.sectors)
    if check and B and (src.min() < 0 or dst.min() < 0 or src.max() >= n or dst.max() >= n):
        raise ValueError("scan index out of range")
    rows = _se2_rows(tf, B)
    if B == 0:
        z = np.zeros((0, 2))
        return VisResult(np.zeros((0, 6), np.int64), z, z.copy(), np.zeros(0, dtype=bool))
    if tables is None:
        tables = scan_tables(scanset, params, stream, check)
    if tuple(tables.shape) != (n, S):
        raise ValueError(f"tables of shape {tuple(tables.shape)} for {n} scans and {S} sectors")
    dev = scanset.device
    d_src = dv.to_dev(src, np.int32, dev)
    d_dst = dv.to_dev(dst, np.int32, dev)
    d_tf = dv.to_dev(rows, np.float64, dev)
    out = dv.empty((B, 6), np.int32, dev)
    h = _stream(stream)
    lib = _abi.lib()
    _abi.check(lib.slam_vis_check_f64(dv.ptr(scanset.pts), dv.ptr(scanset.scan_off), n, len(scanset.host_pts),
                                      dv.ptr(_dirs_dev(scanset, S)), S, dv.ptr(tables), dv.ptr(d_src), dv.ptr(d_dst),
                                      dv.ptr(d_tf), B, float(params.margin), int(params.window), dv.ptr(out), h),
               "slam_vis_check_f64")
    if check:
        _abi.check(lib.slam_vis_status(h), "slam_vis_check_f64")
    elif stream is not None:
        stream.synchronize()
    counts = out.cpu().numpy().astype(np.int64)
    agree, conflict = shares(counts)
    return VisResult(counts, agree, conflict, params.passes(counts))
