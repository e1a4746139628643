"""Robust Gauss-Newton: loss kernels by per-edge reweighting on the GPU.

``GaussNewton`` minimises sum_e w[e] |e_e|^2 with the fixed information
w = 2 / 5 (odometry / loop edges), so one wrong loop closure bends the whole
map.  ``RobustGaussNewton`` minimises sum_e rho(s_e), s_e = info_e |e_e|^2,
by iteratively reweighted least squares: before every iteration one launch of
``slam_gn_robust_weights_f64`` (csrc/robust_kernels.hip) rewrites the solver's
weight array as w[e] = info_e rho'(s_e) at the current poses, and the
UNCHANGED Gauss-Newton iteration follows on the same stream.  Losses: huber,
cauchy, gm (Geman-McClure), dcs (dynamic covariance scaling) and gnc-gm
(Geman-McClure with graduated non-convexity: its scale starts wide enough to
be convex over the residuals present and is lowered by 1.4 per iteration).

The loss ``scale`` c is in units of sqrt(information) x metres (radians for
the heading): the informations 2 I / 5 I are not covariances, so c is not a
chi-square quantile.  With information 5, c = 0.3 puts the turning point of
gm / dcs at a residual of about 0.13 m.
"""
import contextlib

import numpy as np

from . import _abi
from . import device as dv
from .gn import LOOP_INFO, ODOM_INFO, GaussNewton

LOSSES = tuple(_abi.LOSSES)
GNC_STEP = 1.4   # gnc-gm: mu <- max(1, mu / GNC_STEP) after every iteration


def robust_mask(ea, eb, robust_edges="loops"):
    """The edges a loss applies to: "loops" (|b - a| != 1, the rule that tells
    loop from odometry information), "all", or a boolean mask of E entries."""
    ea = np.asarray(ea, dtype=np.int64)
    eb = np.asarray(eb, dtype=np.int64)
    if isinstance(robust_edges, str):
        if robust_edges == "loops":
            return np.abs(eb - ea) != 1
        if robust_edges == "all":
            return np.ones(len(ea), dtype=bool)
        raise ValueError(f"robust_edges {robust_edges!r} (loops | all | a boolean mask)")
    m = np.asarray(robust_edges)
    if m.dtype != np.bool_ or m.shape != ea.shape:
        raise ValueError(f"robust_edges: a boolean mask of {len(ea)} entries (got {m.dtype}, shape {m.shape})")
    return m.copy()


class RobustGaussNewton(GaussNewton):
    def __init__(self, poses, ea, eb, tf, loss, scale, information=None, robust_edges="loops",
                 odom_information=ODOM_INFO, loop_information=LOOP_INFO, fixed=0, device=None, plan=None):
        if loss not in _abi.LOSSES:
            raise ValueError(f"unknown loss {loss!r} ({' | '.join(LOSSES)})")
        scale = float(scale)
        if not np.isfinite(scale) or scale <= 0:
            raise ValueError(f"loss scale {scale!r} is not finite and positive")
        ea = np.asarray(ea, dtype=np.int32)
        eb = np.asarray(eb, dtype=np.int32)
        N = len(poses)
        if len(ea) and (min(ea.min(), eb.min()) < 0 or max(ea.max(), eb.max()) >= N):
            raise ValueError("edge endpoints outside the poses")
        super().__init__(poses, ea, eb, tf, odom_information, loop_information, fixed, device, plan)
        self.loss, self.scale = loss, scale
        mask = robust_mask(ea, eb, robust_edges)
        dev = self.poses.device
        if information is None:
            self.info = self.w.clone()   # the 2 / 5 rule as GaussNewton applied it
        else:
            info = np.asarray(information, dtype=np.float64)
            if info.shape != (self.E,) or not np.all(np.isfinite(info)) or np.any(info < 0):
                raise ValueError(f"information: {self.E} finite non-negative scalars")
            self.info = dv.to_dev(info, np.float64, dev)
        self.mask = mask
        self._mask = dv.to_dev(mask.astype(np.uint8), np.uint8, dev)
        self.n_part = (self.E + _abi.GN_ROBUST_BLOCK - 1) // _abi.GN_ROBUST_BLOCK
        # s, ratio and the weights-only launches' partials in one buffer: one copy reads them all back
        E1, P1 = max(self.E, 1), max(self.n_part, 1)
        self._out = dv.torch().zeros(2 * E1 + 2 * P1, dtype=dv.torch().float64, device=dev)
        self._s, self._r = self._out[:E1], self._out[E1:2 * E1]
        self._final = self._out[2 * E1:].view(2, 1, P1)
        # iterations -> (cost, max s) partials, one row per iteration.  Kept for the solver's life: a
        # captured graph holds their addresses, and the base class may capture again at any time
        self._parts = {}
        self._row = None
        self._k = 0
        self.mu = 1.0         # gnc-gm: the scale factor of the next iteration (1 for every other loss)
        self._mu_start = 1.0  # ... and where the steps in flight began: _run starts over from it
        self.cost = self.ratios = self.edge_chi2 = self.final_cost = None

    def _partials(self, rows):
        t = dv.torch()
        return t.zeros((2, max(rows, 1), max(self.n_part, 1)), dtype=t.float64, device=self.poses.device)

    def _weights(self, part, row, mu, stream=None):
        """The reweighting launch at the current poses: w, s and the ratios, and row `row` of the partials."""
        _abi.check(_abi.lib().slam_gn_robust_weights_f64(
            dv.ptr(self.poses), dv.ptr(self.ea), dv.ptr(self.eb), dv.ptr(self.tf), dv.ptr(self.info),
            dv.ptr(self._mask), self.E, _abi.LOSSES[self.loss], self.scale, mu, dv.ptr(self.w), dv.ptr(self._s),
            dv.ptr(self._r), dv.ptr(part[0, row]), dv.ptr(part[1, row]), dv.stream_handle(stream)),
            "slam_gn_robust_weights_f64")

    def reweight(self, stream=None):
        """One weights-only launch at the current poses (asynchronous): leaves w = info x ratio in
        the solver; what run() does once more after its last step."""
        self._weights(self._final, 0, self.mu, stream)

    def _mu0(self, stream=None):
        """gnc-gm's first mu, max(1, 2 max s / c^2) over the masked edges at
        the current poses (one read-back): every masked residual starts on
        the convex side of the Geman-McClure loss of scale mu c^2."""
        if self.E == 0:
            return 1.0
        self._weights(self._final, 0, 1.0, stream)
        smax = float(self._final[1, 0].cpu().numpy().max())
        return max(1.0, 2.0 * smax / (self.scale * self.scale))

    def iterate(self, chi2_out, stream=None):
        """The reweighting launch, then one unchanged GN iteration (chi2_out: sum of ratio x s)."""
        self._weights(self._row, self._k, self.mu, stream)
        self._k += 1
        if self.loss == "gnc-gm":
            self.mu = max(1.0, self.mu / GNC_STEP)
        super().iterate(chi2_out, stream)

    def _run(self, iterations, stream, graph):
        # also the entry of the base class's re-run after a fused back-substitution
        # timeout: the partial rows and gnc-gm's mu start over with the restored poses
        self._k = 0
        self.mu = self._mu_start
        self._row = self._parts.get(iterations)
        if self._row is None:
            self._row = self._parts[iterations] = self._partials(iterations)
        return super()._run(iterations, stream, graph)

    def _steps(self, iterations, stream, graph):
        """`iterations` steps: (robust cost, GN chi2) before each."""
        if self.loss == "gnc-gm":
            graph = False   # mu is a launch argument: no graph with a baked mu
        self._mu_start = self.mu
        chi2 = self._run(iterations, stream, False if stream is not None else graph)
        cost = self._row[0, :iterations].cpu().numpy().sum(axis=1)
        return cost, chi2

    def run(self, iterations=10, tol=None, stream=None, graph=None):
        """Run `iterations` steps; returns the ROBUST cost (sum of rho over
        the masked edges plus s over the others) before every step.  The GN
        kernels' own chi2, sum of ratio x s, stays in ``.chi2``.  ``tol`` stops
        once the robust cost changes by less than tol (relative).  Afterwards
        ``.ratios`` and ``.edge_chi2`` hold every edge's ratio and s at the
        final poses and ``.final_cost`` the robust cost there."""
        t = dv.torch()
        ctx = t.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            if self.loss == "gnc-gm":
                self.mu = self._mu0(stream)
            if tol is not None and iterations > 1:
                cost, chi2 = [], []
                for _ in range(iterations):
                    c, x = self._steps(1, stream, graph)
                    cost.append(float(c[0]))
                    chi2.append(float(x[0]))
                    if len(cost) > 1 and abs(cost[-2] - cost[-1]) <= tol * max(abs(cost[-2]), 1e-300):
                        break
                cost, chi2 = np.asarray(cost), np.asarray(chi2)
            else:
                cost, chi2 = self._steps(iterations, stream, graph)
            self.cost, self.chi2 = cost, chi2
            # the ratios at the final poses (also leaves w = info x those ratios)
            self.reweight(stream)
            out = self._out.cpu().numpy()
            E1 = len(self._s)
            self.edge_chi2, self.ratios = out[:self.E].copy(), out[E1:E1 + self.E].copy()
            self.final_cost = float(out[2 * E1:2 * E1 + self.n_part].sum())
        return cost

    def outliers(self, threshold=0.5):
        """Indices of the masked edges whose ratio at the final poses is below `threshold`."""
        if self.ratios is None:
            raise RuntimeError("outliers(): run() first")
        return np.flatnonzero(self.mask & (self.ratios < threshold))


def optimize(poses, ea, eb, tf, loss, scale, iterations=10, **kw):
    s = RobustGaussNewton(poses, ea, eb, tf, loss, scale, **kw)
    cost = s.run(iterations)
    return s.host_poses(), cost, s
