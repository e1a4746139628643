"""Lidar-only place recognition on the GPU (kernels in csrc/sig_kernels.hip):
loop-closure candidates from the scans themselves.

The proximity search (``slamhip.lcd``) looks at the estimated poses, so it
never proposes a loop that drift has opened by more than ``max_dist``; the
image detector (``slamhip.desc``) needs a camera.  Here every scan gets a
rotation-invariant polar occupancy signature (S sectors x 32 rings of bits),
and every row is compared with every later scan at every rotation:
``d(i, j, k) = sum_s popcount(sig_i[s] ^ sig_j[(s + k) % S])``, minimised over
k.  The poses only exclude the recent path (``lcd.path_starts``); nearness is
never asked of them.  The best shift ``k_ij`` also gives the relative heading
for the loop-closure ICP's initial guess.

The reference has no counterpart.  include/slamhip.h states the rule,
tests/sig_ref.py restates it in NumPy and tests/test_sig_gpu.py compares bit
for bit.  Limit: the detector is for revisits in the direction of travel, at
any rotation of the scan frame.  A 270-degree scan taken at a truly different
heading sees other walls, and neither the signature nor point-to-point ICP
matches it.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv

RINGS = 32
MAX_TOP_K = 16


@dataclass(frozen=True)
class SigParams:
    sectors: int = 64      # S: 8..128, a multiple of 8
    r_min: float = 0.0     # inner edge of ring 0 (m)
    dr: float = 0.4        # ring width (m)

    def __post_init__(self):
        if not (8 <= int(self.sectors) <= 128 and int(self.sectors) % 8 == 0):
            raise ValueError(f"sectors = {self.sectors}: a multiple of 8 in 8..128")
        if not (self.r_min >= 0 and self.dr > 0):
            raise ValueError(f"r_min = {self.r_min} >= 0 and dr = {self.dr} > 0 expected")

    def tables(self):
        """``(dirs float64[S][2], edges2 float64[33])`` as include/slamhip.h
        wants them: one scalar np.cos / np.sin call per entry."""
        S = int(self.sectors)
        dirs = np.array([[np.cos((s + 0.5) * 2 * np.pi / S), np.sin((s + 0.5) * 2 * np.pi / S)] for s in range(S)])
        edges2 = np.array([(self.r_min + k * self.dr) ** 2 for k in range(RINGS + 1)])
        return dirs, edges2


class SignatureSet:
    """The signatures of N scans, resident on the device: ``d_sig`` (N, S)
    uint32 bits (held as int32), ``d_ring`` (N, 32) uint8, ``d_n`` (N,) int32."""

    def __init__(self, params, n, device):
        self.params = params
        self.device = device
        S = int(params.sectors)
        self.d_sig = dv.empty((max(n, 1), S), np.int32, device)
        self.d_ring = dv.empty((max(n, 1), RINGS), np.uint8, device)
        self.d_n = dv.empty((max(n, 1),), np.int32, device)
        self.n = n

    def __len__(self):
        return self.n

    @classmethod
    def from_host(cls, sig, params=None, device=None):
        """A resident set of given masks ((N, S) uint32), ring counts taken
        from them."""
        sig = np.ascontiguousarray(sig, dtype=np.uint32)
        if sig.ndim != 2:
            raise ValueError(f"signatures must be (N, S) uint32, got shape {sig.shape}")
        params = params if params is not None else SigParams(sectors=sig.shape[1])
        if sig.shape[1] != params.sectors:
            raise ValueError(f"{sig.shape[1]} masks per scan for {params.sectors} sectors")
        self = cls(params, len(sig), device if device is not None else dv.default_device())
        if len(sig):
            bits = (sig[:, :, None] >> np.arange(RINGS, dtype=np.uint32)[None, None, :]) & np.uint32(1)
            ring = bits.sum(1)
            self.d_sig.copy_(dv.to_dev(sig.view(np.int32), np.int32, self.device))
            self.d_ring.copy_(dv.to_dev(ring, np.uint8, self.device))
            self.d_n.copy_(dv.to_dev(ring.sum(1), np.int32, self.device))
        return self

    def host(self):
        """``(sig uint32[N][S], ring uint8[N][32], n int32[N])``."""
        n = self.n
        return (self.d_sig[:n].cpu().numpy().view(np.uint32), self.d_ring[:n].cpu().numpy(),
                self.d_n[:n].cpu().numpy())


def build_signatures(scanset, params=None, stream=None, tables=None):
    """The resident ``SignatureSet`` of a resident ``slamhip.icp.ScanSet``
    (slam_sig_build): one launch, no host copies of the scans.  ``tables``
    (diagnostics): ``(dirs (S, 2), edges2 (33,))`` instead of
    ``params.tables()``."""
    params = params if params is not None else SigParams()
    N = len(scanset)
    if N >= 1 << 31:
        raise ValueError("more than 2^31 - 1 scans")
    out = SignatureSet(params, N, scanset.device)
    if N == 0:
        return out
    dirs, edges2 = tables if tables is not None else params.tables()
    dirs, edges2 = np.asarray(dirs, dtype=np.float64), np.asarray(edges2, dtype=np.float64)
    if dirs.shape != (params.sectors, 2) or edges2.shape != (RINGS + 1,) or not np.all(np.diff(edges2) >= 0):
        raise ValueError(f"tables must be dirs ({params.sectors}, 2) and nondecreasing edges2 ({RINGS + 1},)")
    d_dirs = dv.to_dev(dirs, np.float64, scanset.device)
    d_edges = dv.to_dev(edges2, np.float64, scanset.device)
    L = _abi.lib()
    h = _stream(stream)
    _abi.check(L.slam_sig_build(dv.ptr(scanset.pts), dv.ptr(scanset.scan_off), N, int(scanset.off[-1]),
                                dv.ptr(d_dirs), dv.ptr(d_edges), int(params.sectors), dv.ptr(out.d_sig),
                                dv.ptr(out.d_ring), dv.ptr(out.d_n), h), "slam_sig_build")
    _abi.check(L.slam_sig_status(h), "slam_sig_build")
    return out


def _stream(stream):
    """The handle of ``stream`` (None: the current one), made to wait for the
    work already queued on the current stream: uploads and earlier launches."""
    if stream is not None:
        stream.wait_stream(dv.torch().cuda.current_stream())
    return dv.stream_handle(stream)


def match_signatures(sigset, start, n_rows, max_frac=(1, 4), top_k=1, stream=None):
    """``(j, d, k int64[n_rows][top_k], count int64[n_rows])``: for every row
    i < n_rows the ``top_k`` best candidates among the scans j in [start[i],
    N) with ``d_ij * den <= num * (n_i + n_j)`` (``max_frac = (num, den)``),
    ordered by (d_ij, j); unused slots are -1; ``count`` is the number of
    candidates, which may exceed ``top_k`` (slam_sig_match).  ``start[i] ==
    N`` leaves a row empty."""
    N, n_rows, K = len(sigset), int(n_rows), int(top_k)
    num, den = (int(v) for v in max_frac)
    if not 1 <= K <= MAX_TOP_K:
        raise ValueError(f"top_k = {K} outside 1..{MAX_TOP_K}")
    if not (0 <= num <= den and 1 <= den < 1 << 31):
        raise ValueError(f"max_frac = {num} / {den}: 0 <= num <= den and 1 <= den < 2^31 expected")
    start = np.asarray(start)
    if not 0 <= n_rows <= N or start.ndim != 1 or len(start) < n_rows:
        raise ValueError(f"n_rows = {n_rows} needs 0 <= n_rows <= N = {N} and that many starts")
    empty = np.full((n_rows, K), -1, np.int64)
    if n_rows == 0:
        return empty, empty.copy(), empty.copy(), np.zeros(0, np.int64)
    lim = np.iinfo(np.int32)
    L = _abi.lib()
    S = int(sigset.params.sectors)
    n_work = int(L.slam_sig_work_size(N, S, K))
    if n_work < 0:
        _abi.check(n_work, "slam_sig_work_size")
    dev = sigset.device
    d_start = dv.to_dev(np.clip(start[:n_rows], lim.min, lim.max), np.int32, dev)   # beyond int32 stays out of range
    work = dv.empty((n_work,), np.uint8, dev)
    out = [dv.empty((n_rows, K), np.int32, dev) for _ in range(3)]
    out_c = dv.empty((n_rows,), np.int32, dev)
    h = _stream(stream)
    _abi.check(L.slam_sig_match(dv.ptr(sigset.d_sig), dv.ptr(sigset.d_ring), dv.ptr(sigset.d_n), N, S,
                                dv.ptr(d_start), n_rows, num, den, K, dv.ptr(out[0]), dv.ptr(out[1]), dv.ptr(out[2]),
                                dv.ptr(out_c), dv.ptr(work), h), "slam_sig_match")
    _abi.check(L.slam_sig_status(h), "slam_sig_match")
    j, d, k = (o.cpu().numpy().astype(np.int64) for o in out)
    return j, d, k, out_c.cpu().numpy().astype(np.int64)


def signature_candidates_device(scanset, poses, min_dist_along_path=5, params=None, max_frac=(1, 4), sigset=None):
    """The (i, j, k) of every scan's best signature candidate, in the order the
    greedy pass visits them (the last row first, like
    ``lcd.proximity_candidates_device``).  The poses only exclude the recent
    path: j is at least ``min_dist_along_path`` further along it than i
    (``lcd.path_starts``).  ``sigset``: signatures already built from
    ``scanset``."""
    from .lcd import path_starts
    N = len(scanset)
    if len(poses) != N:
        raise ValueError(f"{len(poses)} poses for {N} scans")
    if N < 2:
        return []
    start, n_rows = path_starts(poses, min_dist_along_path)
    if n_rows == 0:
        return []
    sg = sigset if sigset is not None else build_signatures(scanset, params)
    j, _, k, _ = match_signatures(sg, start, n_rows, max_frac, 1)
    out = [(int(i), int(j[i, 0]), int(k[i, 0])) for i in np.nonzero(j[:, 0] >= 0)[0]]
    out.reverse()
    return out


def shift_inits(k, sectors):
    """(B, 3, 3) initial transforms of icp(pc1 = scan j, pc2 = scan i) from
    the best shifts k_ij: the pure rotation by -2 pi k / S (scan j's masks match
    scan i's moved up k sectors: its frame is turned by that much)."""
    from . import se2
    return np.stack([se2.pose_to_mat((0.0, 0.0, -2 * np.pi * int(kk) / int(sectors))) for kk in k]) \
        if len(k) else np.zeros((0, 3, 3))
