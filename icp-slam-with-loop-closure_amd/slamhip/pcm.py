"""Loop-closure verification on the GPU (kernels in csrc/pcm_kernels.hip):
pairwise consistent measurement set selection.

The detectors propose loop closures and accept one when its ICP error is under
a threshold.  A wrong closure with a low error (an aliased place) bends the
whole map in both optimisers.  Here the closures check each other: two are
consistent when the cycle they form with the chain of poses closes to within
the chain's drift, ``trans_tol^2 + trans_drift^2 n`` in squared translation and
``rot_tol^2 + rot_drift^2 n`` in the squared chord of the rotation, n the
number of chain steps the cycle spans; a min-degree peel then keeps a large set
that is pairwise consistent.  The peel returns *a* maximal consistent set, not
the maximum one, and when the chain's drift exceeds the tolerances true
closures are rejected too.

The reference has no counterpart.  include/slamhip.h states the rule,
tests/pcm_ref.py restates it in NumPy and tests/test_pcm_gpu.py compares bit
for bit; tests/pcm_cases.py holds hand-placed inputs for every peel slot, tile
edge and the capacity, checked on the CPU by tests/test_pcm_cases.py and run on
the GPU by tests/test_pcm_paths_gpu.py.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv

MAX_CLOSURES = 65536


@dataclass(frozen=True)
class PcmParams:
    # The defaults keep 99.8 % of the true pairs on the C5 stand-in's stage-1 chain, which drifts by 21 m: wide
    # enough to be a weak check there (DESIGN.md section 3.9 has the figures).  Set them to the chain at hand.
    trans_tol: float = 0.05      # m: the floor of the cycle's translation
    rot_tol: float = 0.01        # chord of the cycle's rotation (about rad)
    trans_drift: float = 0.5     # m per square root of a chain step
    rot_drift: float = 0.05      # chord per square root of a chain step
    min_size: int = 2            # fewer consistent closures than this: none is kept

    def __post_init__(self):
        tol = (self.trans_tol, self.rot_tol, self.trans_drift, self.rot_drift)
        if not all(float(v) >= 0 for v in tol) or int(self.min_size) < 0:
            raise ValueError(f"tolerances {tol} >= 0 and min_size = {self.min_size} >= 0 expected")


@dataclass
class PcmResult:
    keep: np.ndarray        # (L,) bool: the closures of the consistent set
    degree: np.ndarray      # (L,) int64: closures each one is consistent with
    order: np.ndarray       # (L,) int64: the step that removed it, -1 if none did
    steps: int              # removals
    adjacency: np.ndarray = None   # (L, ceil(L / 32)) uint32 bit rows (return_adjacency=True)


def pose_elements(poses):
    """float64[N][4] (cos, sin, x, y) of (N, 3) poses: one scalar np.cos /
    np.sin call per pose, as ``se2.pose_to_mat``."""
    return np.array([[np.cos(p[2]), np.sin(p[2]), p[0], p[1]] for p in np.asarray(poses, dtype=np.float64)]
                    ).reshape(-1, 4)


def _stream(stream):
    """The handle of ``stream`` (None: the current one), made to wait for the
    work already queued on the current stream: uploads and earlier launches."""
    if stream is not None:
        stream.wait_stream(dv.torch().cuda.current_stream())
    return dv.stream_handle(stream)


def consistency(poses, a, b, Z, params=None, return_adjacency=False, stream=None):
    """The consistent set of L closures ``X_b = X_a Z`` ("relative" convention)
    over the chain ``poses``, (N, 3) rows (x, y, theta) or (N, 4) elements
    (cos, sin, x, y) as ``pose_elements`` makes them: ``Z`` is (L, 3, 3) SE(2)
    matrices.  slam_pcm_adjacency_f64, then slam_pcm_select."""
    params = params if params is not None else PcmParams()
    poses = np.asarray(poses, dtype=np.float64)
    a, b = np.asarray(a), np.asarray(b)
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 3, 3)
    L = len(a)
    if poses.ndim != 2 or poses.shape[1] not in (3, 4) or len(poses) == 0 or len(poses) >= 1 << 31:
        raise ValueError(f"poses must be (N, 3) or (N, 4) with 1 <= N < 2^31, got shape {poses.shape}")
    if a.ndim != 1 or b.shape != a.shape or len(Z) != L:
        raise ValueError(f"{L} a, {b.shape} b and {len(Z)} transforms: one of each per closure expected")
    if L > MAX_CLOSURES:
        raise ValueError(f"{L} closures, above {MAX_CLOSURES}")
    if L == 0:
        empty = np.zeros(0, np.int64)
        return PcmResult(np.zeros(0, bool), empty, empty.copy(), 0,
                         np.zeros((0, 0), np.uint32) if return_adjacency else None)
    lim = np.iinfo(np.int32)
    dev = dv.default_device()
    W = (L + 31) // 32
    lib = _abi.lib()
    n_work = int(lib.slam_pcm_work_size(L))
    if n_work < 0:
        _abi.check(n_work, "slam_pcm_work_size")
    d_X = dv.to_dev(pose_elements(poses) if poses.shape[1] == 3 else poses, np.float64, dev)
    d_a = dv.to_dev(np.clip(a, lim.min, lim.max), np.int32, dev)   # beyond int32 stays out of range
    d_b = dv.to_dev(np.clip(b, lim.min, lim.max), np.int32, dev)
    d_Z = dv.to_dev(np.stack([Z[:, 0, 0], Z[:, 1, 0], Z[:, 0, 2], Z[:, 1, 2]], axis=-1), np.float64, dev)
    d_adj = dv.empty((L, W), np.int32, dev)
    d_deg, d_order, d_steps = (dv.empty((n,), np.int32, dev) for n in (L, L, 1))
    d_keep = dv.empty((L,), np.uint8, dev)
    work = dv.empty((n_work,), np.uint8, dev)
    h = _stream(stream)
    _abi.check(lib.slam_pcm_adjacency_f64(dv.ptr(d_X), len(poses), dv.ptr(d_a), dv.ptr(d_b), dv.ptr(d_Z), L,
                                          float(params.trans_tol), float(params.trans_drift), float(params.rot_tol),
                                          float(params.rot_drift), dv.ptr(d_adj), dv.ptr(d_deg), dv.ptr(work), h),
               "slam_pcm_adjacency_f64")
    _abi.check(lib.slam_pcm_select(dv.ptr(d_adj), dv.ptr(d_deg), L, int(params.min_size), dv.ptr(d_order),
                                   dv.ptr(d_keep), dv.ptr(d_steps), h), "slam_pcm_select")
    _abi.check(lib.slam_pcm_status(h), "slam_pcm_adjacency_f64")
    return PcmResult(d_keep.cpu().numpy().astype(bool), d_deg.cpu().numpy().astype(np.int64),
                     d_order.cpu().numpy().astype(np.int64), int(d_steps.cpu().numpy()[0]),
                     d_adj.cpu().numpy().view(np.uint32) if return_adjacency else None)
