"""Localisation of scans in a finished occupancy grid on the GPU (kernels in
csrc/loc_kernels.hip).

The pipeline ends at ``produce_occupancy_grid``; this module answers where a
scan lies in the map it made: tracking from a rough guess (``localize``),
relocalisation with no guess (``relocalize``) and a check that the scans of a
run agree with the final map (``score_poses``).  A ``LikelihoodField`` holds,
resident on the device, the squared cell distance of every cell to the nearest
occupied cell, capped at ``d_cap`` cells (integers only, exact).  ``search``
sums that field under a scan's points for every angle bin and whole-cell shift
of a window and returns the cheapest bin, ties to the smallest flat index
``(k * ny + j) * nx + i``; ``refine`` runs Gauss-Newton on the bilinear field in
metres from a start pose.  include/slamhip.h states the exact definitions;
tests/loc_ref.py restates them in NumPy.  The reference has no counterpart, and
everything here is opt-in: no existing call changes what it returns.

Poses are (x, y, theta) rows in the map frame, as everywhere in the project;
``search`` takes its centres as (theta0, x0, y0), as ``slamhip.csm`` does.
"""
from dataclasses import dataclass

import numpy as np

from . import _abi
from . import device as dv
from .csm import rotations
from .icp import ScanSet

CONVERGED, MAX_ITERS, SINGULAR, TOO_FEW = 0, 1, 2, 3
STATUS_NAMES = ("CONVERGED", "MAX_ITERS", "SINGULAR", "TOO_FEW")
MAX_D_CAP = 255


@dataclass(frozen=True)
class LocParams:
    n_theta: int = 41            # angle bins: theta0 + (k - n_theta // 2) * d_theta
    d_theta: float = 0.0125      # angle bin spacing (rad)
    nx: int = 21                 # shift window: x0 + (i - nx // 2) * step cells
    ny: int = 21
    step: int = 1                # cells per shift
    max_iters: int = 30          # refinement
    eps_t: float = 1e-4          # m: a step below (eps_t, eps_r) ends the refinement
    eps_r: float = 1e-4          # rad
    min_inlier_frac: float = 0.5  # fewer points than this share on the field: TOO_FEW
    pivot_tol: float = 1e-9      # a pivot d_k <= pivot_tol H_kk: SINGULAR

    def __post_init__(self):
        if min(int(self.n_theta), int(self.nx), int(self.ny), int(self.step)) < 1:
            raise ValueError(f"loc: n_theta = {self.n_theta}, nx = {self.nx}, ny = {self.ny}, step = {self.step} "
                             "must be positive")
        if int(self.n_theta) * int(self.ny) * int(self.nx) >= 2 ** 31:
            raise ValueError("loc: the cost volume n_theta * ny * nx does not fit 31 bits")
        if not np.isfinite(float(self.d_theta)):
            raise ValueError("loc: d_theta must be finite")
        tol = (self.eps_t, self.eps_r, self.pivot_tol, self.min_inlier_frac)
        if not all(np.isfinite(float(v)) and float(v) >= 0 for v in tol) or float(self.min_inlier_frac) > 1:
            raise ValueError(f"loc: tolerances {tol}: finite and >= 0 expected, min_inlier_frac at most 1")
        if int(self.max_iters) < 1:
            raise ValueError(f"loc: max_iters = {self.max_iters} >= 1 expected")


@dataclass
class LocSearchResult:
    index: np.ndarray          # (B, 3) int32 (k, j, i) of the cheapest bin
    cost: np.ndarray           # (B,) int32 its cost (at most n * d_cap^2)
    poses: np.ndarray          # (B, 3) (x, y, theta) of that bin
    n_points: np.ndarray       # (B,) points of the query's scan
    costs: np.ndarray = None   # (B, n_theta, ny, nx) int32 when requested


@dataclass
class LocRefineResult:
    poses: np.ndarray          # (B, 3) (x, y, theta); the pose of the last linearisation where status is SINGULAR / TOO_FEW
    iters: np.ndarray          # (B,) int64 steps taken
    inliers: np.ndarray        # (B,) int64 points on the field in the last linearisation
    status: np.ndarray         # (B,) int64 CONVERGED, MAX_ITERS, SINGULAR or TOO_FEW
    rms: np.ndarray            # (B,) rms residual (m) of the last linearisation


@dataclass
class LocResult:
    poses: np.ndarray          # (B, 3) the refined poses
    search: LocSearchResult
    refine: LocRefineResult


def check_map(grid, origin, cell_width, d_cap, occ_min):
    """The map's arrays as the kernels take them; ValueError for a bad one."""
    grid = np.asarray(grid)
    if grid.dtype != np.int8 or grid.ndim != 2 or grid.size == 0:
        raise ValueError("loc: the occupancy grid must be a non-empty 2-D np.int8 array")
    if grid.shape[0] > 65535:
        raise ValueError(f"loc: a grid of {grid.shape[0]} rows, above 65,535")
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (2,) or not np.all(np.isfinite(origin)):
        raise ValueError("loc: origin must be two finite numbers (min_x, min_y)")
    cw = float(cell_width)
    if not (np.isfinite(cw) and cw > 0):
        raise ValueError(f"loc: cell_width must be positive, got {cell_width}")
    if int(d_cap) != d_cap or not 1 <= int(d_cap) <= MAX_D_CAP:
        raise ValueError(f"loc: d_cap = {d_cap} outside 1..{MAX_D_CAP}")
    if int(occ_min) != occ_min or not -128 <= int(occ_min) <= 127:
        raise ValueError(f"loc: occ_min = {occ_min} outside int8")
    return np.ascontiguousarray(grid), origin, cw, int(d_cap), int(occ_min)


class LikelihoodField:
    """The capped squared-distance field of an occupancy grid, resident on the
    device.  ``grid`` (H, W) int8 and ``origin`` (min_x, min_y) as
    ``produce_occupancy_grid`` returns them; a cell is occupied iff
    ``grid > occ_min``; ``d_cap`` in cells."""

    def __init__(self, grid, origin, cell_width, d_cap=20, occ_min=0, device=None, stream=None):
        grid, self.origin, self.cell_width, self.d_cap, self.occ_min = check_map(grid, origin, cell_width, d_cap,
                                                                                 occ_min)
        self.H, self.W = grid.shape
        L = _abi.lib()
        t = dv.require_gpu()
        d_grid = dv.to_dev(grid, np.int8, device)
        self.device = d_grid.device
        n_work = int(L.slam_loc_field_work_size(self.H, self.W))
        if n_work < 0:
            _abi.check(n_work, "slam_loc_field_work_size")
        work = dv.empty((n_work,), np.uint8, self.device)
        self.dev = t.empty((self.H, self.W), dtype=t.int16, device=self.device)   # uint16 bits
        _abi.check(L.slam_loc_field(dv.ptr(d_grid), self.H, self.W, self.occ_min, self.d_cap, dv.ptr(self.dev),
                                    dv.ptr(work), dv.stream_handle(stream)), "slam_loc_field")
        if stream is not None:
            stream.synchronize()
        self._host = None

    @property
    def field(self):
        """The (H, W) uint16 host copy."""
        if self._host is None:
            self._host = self.dev.cpu().numpy().view(np.uint16)
        return self._host


def _queries(field, scans, idx):
    ss = scans if isinstance(scans, ScanSet) else ScanSet(scans, field.device)
    if not np.all(np.isfinite(ss.host_pts)):
        raise ValueError("non-finite scan points")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(ss)):
        raise ValueError("scan index out of range")
    max_n = int(ss.lens[idx].max(initial=0))
    if max_n * field.d_cap ** 2 >= 2 ** 31:
        raise ValueError(f"loc: a scan of {max_n} points at d_cap = {field.d_cap}: its cost does not fit 31 bits")
    return ss, idx, max_n


def _map_args(f):
    return (dv.ptr(f.dev), f.H, f.W, float(f.origin[0]), float(f.origin[1]), f.cell_width, f.d_cap)


def assemble(centre, index, params, cell_width):
    """(B, 3) poses (x, y, theta) of the bins ``index`` (B, 3) = (k, j, i)."""
    p = params
    out = np.zeros((len(index), 3))
    for b, (k, j, i) in enumerate(index):
        out[b] = (centre[b, 1] + (int(i) - p.nx // 2) * p.step * cell_width,
                  centre[b, 2] + (int(j) - p.ny // 2) * p.step * cell_width,
                  float(centre[b, 0]) + (int(k) - p.n_theta // 2) * float(p.d_theta))
    return out


def search(field, scans, idx, centre, params=LocParams(), return_costs=False, stream=None):
    """Window search of B queries (scan ``idx[b]`` of a list of scans or a
    ``ScanSet``, centre ``centre[b]`` = (theta0, x0, y0)) against ``field`` in
    one launch.  Returns a ``LocSearchResult``."""
    ss, idx, max_n = _queries(field, scans, idx)
    B = len(idx)
    centre = np.asarray(centre, dtype=np.float64).reshape(B, 3)
    if not np.all(np.isfinite(centre)):
        raise ValueError("non-finite search centre")
    p = params
    shape = (B, p.n_theta, p.ny, p.nx)
    if (field.H + 2 * p.ny * p.step) * (field.W + 2 * p.nx * p.step) >= 2 ** 31:
        raise ValueError("loc: the window's bordered table does not fit 31 bits")
    if B * p.n_theta >= 2 ** 31:
        raise ValueError("loc: queries x angles exceed the launch grid")
    if B == 0:
        return LocSearchResult(np.zeros((0, 3), np.int32), np.zeros(0, np.int32), np.zeros((0, 3)),
                               np.zeros(0, np.int64), np.zeros(shape, np.int32) if return_costs else None)
    rot = rotations(centre, p)
    L = _abi.lib()
    n_work = int(L.slam_loc_search_work_size(B, field.H, field.W, p.n_theta, p.ny, p.nx, p.step))
    if n_work < 0:
        _abi.check(n_work, "slam_loc_search_work_size")
    dev = field.device
    d_idx = dv.to_dev(idx, np.int32, dev)
    d_centre = dv.to_dev(centre, np.float64, dev)
    d_rot = dv.to_dev(rot, np.float64, dev)
    work = dv.empty((n_work,), np.uint8, dev)
    best = dv.empty((B, 4), np.int32, dev)
    costs = dv.empty(shape, np.int32, dev) if return_costs else None
    h = dv.stream_handle(stream)
    _abi.check(L.slam_loc_search(*_map_args(field), dv.ptr(ss.pts), dv.ptr(ss.scan_off), len(ss), len(ss.host_pts),
                                 dv.ptr(d_idx), dv.ptr(d_centre), dv.ptr(d_rot), B, max_n, int(p.n_theta), int(p.nx),
                                 int(p.ny), int(p.step), dv.ptr(best), dv.ptr(costs), dv.ptr(work), h),
               "slam_loc_search")
    _abi.check(L.slam_loc_status(h), "slam_loc_search")
    hb = best.cpu().numpy()
    return LocSearchResult(hb[:, 1:].copy(), hb[:, 0].copy(), assemble(centre, hb[:, 1:], p, field.cell_width),
                           ss.lens[idx].copy(), costs.cpu().numpy() if return_costs else None)


def refine(field, scans, idx, poses, params=LocParams(), stream=None):
    """Gauss-Newton on the field in metres from ``poses`` (B, 3) = (x, y, theta),
    one workgroup per query, one launch.  Returns a ``LocRefineResult``."""
    ss, idx, max_n = _queries(field, scans, idx)
    B = len(idx)
    poses = np.asarray(poses, dtype=np.float64).reshape(B, 3)
    if not np.all(np.isfinite(poses)):
        raise ValueError("non-finite start pose")
    if B == 0:
        z = np.zeros(0, np.int64)
        return LocRefineResult(np.zeros((0, 3)), z, z.copy(), z.copy(), np.zeros(0))
    p = params
    dev = field.device
    d_idx = dv.to_dev(idx, np.int32, dev)
    d_init = dv.to_dev(poses[:, [2, 0, 1]], np.float64, dev)
    out_pose, out_rms = dv.empty((B, 3), np.float64, dev), dv.empty((B,), np.float64, dev)
    out_inl, out_it, out_st = (dv.empty((B,), np.int32, dev) for _ in range(3))
    L = _abi.lib()
    h = dv.stream_handle(stream)
    _abi.check(L.slam_loc_refine_f64(*_map_args(field), dv.ptr(ss.pts), dv.ptr(ss.scan_off), len(ss), len(ss.host_pts),
                                     dv.ptr(d_idx), dv.ptr(d_init), B, max_n, int(p.max_iters), float(p.eps_t),
                                     float(p.eps_r), float(p.min_inlier_frac), float(p.pivot_tol), dv.ptr(out_pose),
                                     dv.ptr(out_rms), dv.ptr(out_inl), dv.ptr(out_it), dv.ptr(out_st), h),
               "slam_loc_refine_f64")
    _abi.check(L.slam_loc_status(h), "slam_loc_refine_f64")
    return LocRefineResult(out_pose.cpu().numpy()[:, [1, 2, 0]], out_it.cpu().numpy().astype(np.int64),
                           out_inl.cpu().numpy().astype(np.int64), out_st.cpu().numpy().astype(np.int64),
                           out_rms.cpu().numpy())


def localize(field, scans, idx, guess, params=LocParams()):
    """Tracking: the window search around ``guess`` (B, 3) = (x, y, theta), then
    the refinement from the cheapest bin.  Returns a ``LocResult``."""
    ss = scans if isinstance(scans, ScanSet) else ScanSet(scans, field.device)
    guess = np.asarray(guess, dtype=np.float64).reshape(-1, 3)
    s = search(field, ss, idx, guess[:, [2, 0, 1]], params)
    r = refine(field, ss, idx, s.poses, params)
    return LocResult(r.poses, s, r)


def reloc_params(params):
    """``params`` with the angle bins spread over the full circle: the number of
    bins closest to 2 pi / d_theta, evenly spaced."""
    n = max(1, int(round(2 * np.pi / abs(float(params.d_theta))))) if params.d_theta else 1
    return LocParams(**{**params.__dict__, "n_theta": n, "d_theta": 2 * np.pi / n})


def reloc_centres(H, W, origin, cell_width, params):
    """(T, 3) centres (theta0 = 0, x0, y0) of the windows that tile an (H, W)
    map: tile (ty, tx) covers the cells tx nx step + i step, ty ny step +
    j step, its centre the middle of cell (ty ny + ny // 2) step, (tx nx +
    nx // 2) step.  Row-major in (ty, tx)."""
    p = params
    tx = np.arange(-(-W // (p.nx * p.step)))
    ty = np.arange(-(-H // (p.ny * p.step)))
    x0 = origin[0] + ((tx * p.nx + p.nx // 2) * p.step + 0.5) * cell_width
    y0 = origin[1] + ((ty * p.ny + p.ny // 2) * p.step + 0.5) * cell_width
    out = np.zeros((len(ty) * len(tx), 3))
    out[:, 1] = np.tile(x0, len(ty))
    out[:, 2] = np.repeat(y0, len(tx))
    return out


def relocalize(field, scans, idx, params=LocParams(nx=21, ny=21, step=2, d_theta=np.deg2rad(3.0))):
    """No guess: windows of ``params`` tile the whole map at ``step`` cells, the
    angle bins cover the full circle, and the cheapest bin over all tiles (ties
    to the first tile, then the smallest flat index) is refined.  One search
    launch per scan.  Returns a ``LocResult`` whose ``search.index`` rows are
    (k, j, i) inside the winning tile, listed in ``tile``."""
    ss = scans if isinstance(scans, ScanSet) else ScanSet(scans, field.device)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    p = reloc_params(params)
    centres = reloc_centres(field.H, field.W, field.origin, field.cell_width, p)
    index, cost, poses, tile = [], [], [], []
    for s in idx:
        r = search(field, ss, np.full(len(centres), s), centres, p)
        t = int(np.argmin(r.cost))    # the first minimum
        index.append(r.index[t])
        cost.append(r.cost[t])
        poses.append(r.poses[t])
        tile.append(t)
    B = len(idx)
    sr = LocSearchResult(np.asarray(index, np.int32).reshape(B, 3), np.asarray(cost, np.int32),
                         np.asarray(poses, np.float64).reshape(B, 3), ss.lens[idx].copy())
    sr.tile = np.asarray(tile, np.int64)
    rr = refine(field, ss, idx, sr.poses, p)
    return LocResult(rr.poses, sr, rr)


def score_poses(field, scans, poses, idx=None):
    """The map-consistency report: per scan the field summed under its points at
    ``poses`` (S, 3) = (x, y, theta) and that sum per point (squared cells; 0
    where every point sits on an occupied cell).  Returns (cost (S,) int32, mean
    (S,) float64)."""
    ss = scans if isinstance(scans, ScanSet) else ScanSet(scans, field.device)
    idx = np.arange(len(ss)) if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1)
    poses = np.asarray(poses, dtype=np.float64).reshape(len(idx), 3)
    r = search(field, ss, idx, poses[:, [2, 0, 1]], LocParams(n_theta=1, nx=1, ny=1, step=1))
    return r.cost, r.cost / np.maximum(r.n_points, 1)


def save_map(fname, grid, origin, cell_width):
    """One ``.npz`` holding the int8 grid, its origin (min_x, min_y) and its cell
    width."""
    grid, origin, cw, _, _ = check_map(grid, origin, cell_width, 1, 0)
    with open(fname, "wb") as f:
        np.savez_compressed(f, grid=grid, origin=origin, cell_width=np.float64(cw))


def load_map(fname):
    """(grid, origin, cell_width) of ``save_map``'s file."""
    with np.load(fname, allow_pickle=False) as z:
        grid, origin, cw = z["grid"], z["origin"], float(z["cell_width"])
    grid, origin, cw, _, _ = check_map(grid, origin, cw, 1, 0)
    return grid, origin, cw
