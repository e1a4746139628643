"""Robust Gauss-Newton, CPU side: the loss table of tests/robust_ref.py (the
restatement the GPU kernel is compared with in tests/test_robust_gpu.py), what
the reweighted solve achieves on a graph with wrong closures, and the new
entry point's ABI and argument checks (no GPU needed)."""
import os
import re

import numpy as np
import pytest

import robust_ref as rr
from conftest import REPO

C = 0.3
MU = 3.7   # gnc-gm's scale factor in the table checks


@pytest.mark.parametrize("loss", rr.LOSSES)
def test_ratio_is_the_derivative_of_the_cost(loss):
    """r(s) = rho'(s) by a central difference with h = 1e-5 (s + c2).  Its
    truncation error is h^2 |rho'''| / 6 <= 1e-10 r (rho''' is of the order of
    r / (s + c2)^2 for every loss) and its rounding error eps rho / h <= 2.3e-11
    (rho <= s + c2): the bound 1e-9 + 1e-7 r covers both.  The grid steps
    around the kinks of Huber and DCS at s = c2 by more than h."""
    c2 = C * C * (MU if loss == "gnc-gm" else 1.0)
    s = np.r_[np.logspace(-3, 2, 400), c2 * (1 - 1e-3), c2 * (1 + 1e-3)]
    s = np.sort(s[np.abs(s - c2) > 4e-5 * c2])
    h = 1e-5 * (s + c2)
    fd = (rr.costs(loss, s + h, C, MU) - rr.costs(loss, s - h, C, MU)) / (2 * h)
    r = rr.ratios(loss, s, C, MU)
    err = np.abs(fd - r)
    print(f"{loss}: max |fd - r| {err.max():.2e}, max relative {np.max(err / r):.2e}")
    assert np.all(err <= 1e-9 + 1e-7 * r), (loss, float(err.max()))
    assert np.all(np.diff(r) <= 0) and np.all((r > 0) & (r <= 1))
    assert rr.ratios(loss, 0.0, C, MU) == 1.0 and rr.costs(loss, 0.0, C, MU) == 0.0


def test_dcs_switch_form_is_flat_past_the_kink():
    """Why the DCS cost is the integral of its ratio: sg^2 s + c2 (1 - sg)^2
    with sg = 2 c2 / (c2 + s) is the constant c2 for s > c2, so its derivative
    is 0 there, not the ratio sg^2."""
    s = np.logspace(np.log10(C * C) + 0.01, 3, 200)
    assert np.abs(rr.dcs_switch_cost(s, C) - C * C).max() <= 8 * np.finfo(float).eps * C * C
    assert rr.ratios("dcs", s, C).max() > 0.9


@pytest.mark.parametrize("loss", ["huber", "dcs"])
def test_continuity_at_the_kink(loss):
    """Ratio and cost are continuous at s = c2: one ulp either side of the
    kink they differ by a few ulps."""
    c2 = C * C
    lo, hi = np.nextafter(c2, 0.0), np.nextafter(c2, 1.0)
    eps = np.finfo(float).eps
    for f in (rr.ratios, rr.costs):
        a, b, m = float(f(loss, lo, C)), float(f(loss, hi, C)), float(f(loss, c2, C))
        assert abs(a - b) <= 8 * eps * max(abs(a), abs(b)), (loss, f.__name__, a, b)
        assert min(a, b) - 8 * eps <= m <= max(a, b) + 8 * eps
    assert float(rr.ratios(loss, lo, C)) == 1.0


def test_gnc_at_mu_one_is_geman_mcclure():
    s = np.logspace(-6, 12, 500)
    assert np.array_equal(rr.ratios("gnc-gm", s, C, 1.0), rr.ratios("gm", s, C))
    assert np.array_equal(rr.costs("gnc-gm", s, C, 1.0), rr.costs("gm", s, C))
    # a larger mu is the same loss at the scale sqrt(mu) c
    assert np.allclose(rr.ratios("gnc-gm", s, C, MU), rr.ratios("gm", s, C * np.sqrt(MU)), rtol=1e-14, atol=0)


def test_mask_rule():
    from slamhip import robust
    ea, eb = np.array([0, 1, 2, 0, 3]), np.array([1, 2, 3, 3, 3])
    assert robust.robust_mask(ea, eb).tolist() == [False, False, False, True, True]
    assert np.array_equal(robust.robust_mask(ea, eb), rr.loop_mask(ea, eb))
    assert robust.robust_mask(ea, eb, "all").all()
    m = np.array([True, False, False, True, False])
    assert np.array_equal(robust.robust_mask(ea, eb, m), m)
    for bad in ("some", np.ones(4, dtype=bool), np.ones(5)):
        with pytest.raises(ValueError):
            robust.robust_mask(ea, eb, bad)


@pytest.mark.parametrize("loss", ["gm", "dcs"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_recovers_the_clean_solution(seed, loss):
    """160-node lap graph, 60 exact closures, 10 wrong ones, c = 0.3, 20
    iterations: (a) the max position error to the truth is within 1.10 x that
    of plain GN on the graph WITHOUT the wrong edges; (b) every wrong edge's
    ratio is below 0.01 and every right loop edge's above 0.98; (c) plain GN
    with the wrong edges is more than 1 m off (it does not pass (a))."""
    out = rr.irls_outlier(seed, loss)
    rr.check_abc(out.poses, out.ratios, seed)
    assert rr.plain_error(seed) > 1.10 * rr.clean_error(seed)
    # the robust cost the iteration reports falls and ends near 3 c2 (dcs) / c2 (gm) per wrong edge
    assert out.cost[-1] < out.cost[0] and out.final_cost <= out.cost[-1] * (1 + 1e-9)


# ---------------------------------------------------------------- the entry point (no GPU)

def _aligned(nbytes):
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, a + (-a) % 64


def test_symbol_in_header_library_and_ctypes_table():
    from slamhip import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "slamhip.h")).read(), flags=re.S)
    assert re.search(r"\bslam_gn_robust_weights_f64\s*\(", txt)
    assert len(_abi.SIGNATURES["slam_gn_robust_weights_f64"][1]) == 16
    lib = _abi.lib()
    assert hasattr(lib, "slam_gn_robust_weights_f64") and lib.slam_abi_version() >= 110
    for name, code in _abi.LOSSES.items():
        assert re.search(r"#define SLAM_LOSS_%s %d\b" % (name.upper().replace("-", "_"), code), txt), name
    assert re.search(r"#define SLAM_GN_ROBUST_BLOCK %d\b" % _abi.GN_ROBUST_BLOCK, txt)
    assert tuple(_abi.LOSSES) == rr.LOSSES
    src = open(os.path.join(REPO, "icp-slam-with-loop-closure_amd", "csrc", "Makefile")).read()
    assert "robust_kernels.hip" in src


def test_argument_checks_before_any_launch():
    """Null arrays, E < 0, an unknown loss, a scale that is not finite and
    positive and mu < 1 are refused with a message; E = 0 succeeds: all before
    anything touches a device."""
    from slamhip import _abi
    lib = _abi.lib()
    EINVAL = -1
    keep, p = _aligned(256)      # never dereferenced: every call below returns before a launch

    def call(poses=p, info=p, mask=p, E=0, loss=2, c=0.3, mu=1.0, w=p, parts=p):
        return lib.slam_gn_robust_weights_f64(poses, p, p, p, info, mask, E, loss, c, mu, w, p, p, parts, p, None)

    assert call() == 0 and lib.slam_last_error() == b""
    for kw in ({"poses": None}, {"info": None}, {"mask": None}, {"w": None}, {"parts": None}, {"poses": None, "E": 3}):
        assert call(**kw) == EINVAL and b"null" in lib.slam_last_error(), kw
    assert call(E=-1) == EINVAL and b"E=-1" in lib.slam_last_error()
    for loss in (-1, 5, 99):
        assert call(loss=loss) == EINVAL and b"loss" in lib.slam_last_error(), loss
    for loss in range(5):
        assert call(loss=loss) == 0, loss
    for c in (0.0, -0.3, float("nan"), float("inf")):
        assert call(c=c) == EINVAL and b"scale" in lib.slam_last_error(), c
    for mu in (0.999, 0.0, -2.0, float("nan"), float("inf")):
        assert call(mu=mu, loss=4) == EINVAL and b"mu" in lib.slam_last_error(), mu
    assert call(mu=1.0, loss=4) == 0 and call(mu=1e9, loss=4) == 0
    del keep


def test_python_argument_checks():
    """Rejected before any device memory is touched."""
    from slamhip import robust
    import src.pose_graph_optimization as pgo
    g = rr.outlier_graph(0)
    for kw in ({"loss": "l2", "scale": 0.3}, {"loss": "gm", "scale": 0.0}, {"loss": "gm", "scale": float("nan")}):
        with pytest.raises(ValueError):
            robust.RobustGaussNewton(g[0], g[1], g[2], g[3], **kw)
    with pytest.raises(ValueError):
        robust.RobustGaussNewton(g[0], g[1], g[2] + 1000, g[3], "gm", 0.3)
    with pytest.raises(ValueError):
        pgo.optimize_pose_graph(None, loss="l2")
    with pytest.raises(ValueError):
        pgo.optimize_pose_graph(None, return_weights=True)
