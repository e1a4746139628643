"""Robust Gauss-Newton on the GPU: the reweighting kernel against the NumPy
restatement (tests/robust_ref.py) on hand-placed edges, its tie to the GN
kernels' own chi2, and the reweighted solve (eager, graph replay, every solver
path, the fused back-substitution fallback, the drop-in and the pipeline)
against ``robust_ref.irls``."""
import warnings

import numpy as np
import pytest

import gn_oracle as go
import gn_step
import robust_ref as rr

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
C = 0.3
MU = 3.7
SPECIALS = ("fixed", "self", "zero", "pi_below", "pi_above", "huge", "unmasked")


def _rel(pa, pb):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    d = pb[:2] - pa[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], pb[2] - pa[2]])


def _special(kind, poses, rng):
    """(a, b, tf, info, mask) of one hand-placed edge; nodes 1-6 of `poses` are placed for them."""
    z = rng.uniform([-2, -2, -3], [2, 2, 3])
    if kind == "fixed":        # an edge on the fixed node
        return 0, 9, rr.pose_mat(*z), 5.0, True
    if kind == "self":         # a self-loop: e = (-Rz^T tz, wrap(-thz))
        return 8, 8, rr.pose_mat(*z), 5.0, True
    if kind == "zero":         # nodes 1 and 2 coincide, identity measurement: e = 0 exactly, s = 0
        return 1, 2, np.eye(3), 5.0, True
    if kind == "pi_below":     # thj - thi - thz = pi - 5e-13: stays below pi
        return 3, 4, rr.pose_mat(0.4, -0.2, 0.2), 5.0, True
    if kind == "pi_above":     # pi + 5e-13: wraps to -pi + 5e-13
        return 3, 5, rr.pose_mat(0.4, -0.2, 0.2), 5.0, True
    if kind == "huge":         # node 6 is 4.5e5 m away: s ~ 1e12
        return 7, 6, rr.pose_mat(*z), 5.0, True
    if kind == "unmasked":     # a large s off the mask: the ratio is exactly 1
        return 7, 6, rr.pose_mat(*z), 2.0, False
    raise ValueError(kind)


def _poses(rng, N=40):
    p = np.c_[rng.uniform(-5, 5, (N, 2)), rng.uniform(-np.pi, np.pi, N)]
    p[2] = p[1]
    p[3, 2] = 0.3
    p[4, 2] = 0.5 + np.pi - 5e-13
    p[5, 2] = 0.5 + np.pi + 5e-13
    p[6, :2] = [3.2e5, -3.2e5]
    return p


def _case(E, kinds, seed=5):
    """E edges over 40 poses: the hand-placed ones spread over the array
    (the first and the last slot among them), the rest random pairs, half of
    them nearly consistent (s below c2, Huber's and DCS's flat side)."""
    rng = np.random.default_rng(seed)
    poses = _poses(rng)
    N = len(poses)
    ea = rng.integers(7, N, E)
    eb = rng.integers(7, N, E)
    info = np.where(rng.random(E) < 0.5, 2.0, 5.0)
    mask = rng.random(E) < 0.7
    tf = np.empty((E, 3, 3))
    for e in range(E):
        z = _rel(poses[ea[e]], poses[eb[e]]) + rng.normal(0, 0.03, 3) if e % 2 else rng.uniform([-2, -2, -3], [2, 2, 3])
        tf[e] = rr.pose_mat(*z)
    slots = np.unique(np.linspace(0, E - 1, len(kinds)).astype(int)) if E >= len(kinds) else np.arange(min(E, len(kinds)))
    placed = {}
    for k, e in zip(kinds, slots):
        ea[e], eb[e], tf[e], info[e], mask[e] = _special(k, poses, rng)
        placed[k] = int(e)
    return poses, ea.astype(np.int32), eb.astype(np.int32), tf, info, mask, placed


def _launch(poses, ea, eb, tf, info, mask, loss, c, mu):
    """slam_gn_robust_weights_f64 on host arrays: (w, s, ratio, cost partials, max partials)."""
    from slamhip import _abi
    from slamhip import device as dv
    import torch
    E = len(ea)
    n_part = (E + _abi.GN_ROBUST_BLOCK - 1) // _abi.GN_ROBUST_BLOCK
    d = [dv.to_dev(poses, np.float64), dv.to_dev(ea, np.int32), dv.to_dev(eb, np.int32),
         dv.to_dev(tf.reshape(-1, 9), np.float64), dv.to_dev(info, np.float64), dv.to_dev(mask.astype(np.uint8), np.uint8)]
    out = [torch.full((n,), np.nan, dtype=torch.float64, device=d[0].device) for n in (E, E, E, n_part, n_part)]
    _abi.check(_abi.lib().slam_gn_robust_weights_f64(*[dv.ptr(x) for x in d], E, _abi.LOSSES[loss], c, mu,
                                                     *[dv.ptr(x) for x in out], dv.stream_handle()), "robust weights")
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _s_bound(poses, ea, eb, tf, info):
    """|s_gpu - s_ref| <= info (2 |e| d + d^2) with d = 16 eps (|dx| + |dy| + |z|_1 + pi):
    the device's sincos / atan2 and the rounding of the residual's sums."""
    z = go.edge_measurements(tf)
    d = 16 * EPS * (np.abs(poses[eb, 0] - poses[ea, 0]) + np.abs(poses[eb, 1] - poses[ea, 1]) + np.abs(z).sum(1) + np.pi)
    e = np.linalg.norm(rr.residuals(poses, ea, eb, tf), axis=1)
    return info * (2 * e * d + d * d)


def _check_kernel(poses, ea, eb, tf, info, mask, loss, placed=()):
    mu = MU if loss == "gnc-gm" else 1.0
    w, s, r, costp, smaxp = _launch(poses, ea, eb, tf, info, mask, loss, C, mu)
    E = len(ea)
    s_ref = rr.edge_s(poses, ea.astype(np.int64), eb.astype(np.int64), tf, info)
    ds = _s_bound(poses, ea, eb, tf, info)
    assert np.all(np.abs(s - s_ref) <= ds), np.max(np.abs(s - s_ref) / np.maximum(ds, 1e-300))
    # the bound on s pushed through the (non-increasing) ratio and the (non-decreasing) cost,
    # plus 8 eps for the few roundings of the formulas themselves
    lo, hi = np.maximum(s_ref - ds, 0.0), s_ref + ds
    r_ref = np.where(mask, rr.ratios(loss, s_ref, C, mu), 1.0)
    dr = np.where(mask, rr.ratios(loss, lo, C, mu) - rr.ratios(loss, hi, C, mu), 0.0) + 8 * EPS * r_ref
    assert np.all(np.abs(r - r_ref) <= dr), np.max(np.abs(r - r_ref) / dr)
    assert np.all(r[~mask] == 1.0) and np.all((r > 0) & (r <= 1))
    assert np.array_equal(w, info * r)
    rho_ref = np.where(mask, rr.costs(loss, s_ref, C, mu), s_ref)
    drho = np.where(mask, rr.costs(loss, hi, C, mu) - rr.costs(loss, lo, C, mu), 2 * ds) + 8 * EPS * rho_ref
    assert len(costp) == len(smaxp) == (E + 255) // 256
    assert abs(costp.sum() - rho_ref.sum()) <= drho.sum() + (E + 8) * EPS * rho_ref.sum()
    smax_ref = s_ref[mask].max() if mask.any() else 0.0
    assert abs(smaxp.max() - smax_ref) <= (ds[mask].max() if mask.any() else 0.0)
    # per workgroup too: partial g covers edges 256 g .. 256 g + 255
    for g in range(len(costp)):
        sl = slice(256 * g, min(256 * (g + 1), E))
        assert abs(costp[g] - rho_ref[sl].sum()) <= drho[sl].sum() + 264 * EPS * rho_ref[sl].sum(), g
        m = mask[sl]
        assert smaxp[g] == (s[sl][m].max() if m.any() else 0.0), g
    for k, e in dict(placed).items():
        if k == "zero":
            assert s[e] == 0.0 and r[e] == 1.0 and w[e] == info[e]
        if k in ("pi_below", "pi_above"):     # |e_th| is pi to 5e-13 on either side, never 5e-13 or 2 pi
            e_t = rr.residuals(poses, ea[e:e + 1], eb[e:e + 1], tf[e:e + 1])[0]
            assert abs(s[e] / info[e] - (e_t[0] ** 2 + e_t[1] ** 2 + np.pi ** 2)) <= 1e-11 and abs(abs(e_t[2]) - np.pi) < 1e-12
            assert (e_t[2] > 0) == (k == "pi_below")
        if k == "huge":
            assert 0.9e12 < s[e] < 1.2e12 and 0 < r[e] < (1e-5 if loss in ("huber", "cauchy") else 1e-20)
        if k == "unmasked":
            assert r[e] == 1.0 and w[e] == info[e] and s[e] > 1e11


@pytest.mark.parametrize("loss", rr.LOSSES)
@pytest.mark.parametrize("E", [1, 255, 256, 257, 1000])
def test_kernel_matches_the_restatement(E, loss):
    """Every loss at E = 1, one edge short of a workgroup, exactly one, one
    more, and four workgroups with a partial last one.  Each case holds an edge
    on the fixed node, a self-loop, e = 0 exactly, a heading residual 5e-13
    either side of pi, s ~ 1e12 and an unmasked edge with a large s; at E = 1
    each of them is the single edge of a launch of its own."""
    if E == 1:
        for k in SPECIALS:
            poses, ea, eb, tf, info, mask, placed = _case(1, (k,))
            assert placed == {k: 0}
            _check_kernel(poses, ea, eb, tf, info, mask, loss, placed)
        return
    poses, ea, eb, tf, info, mask, placed = _case(E, SPECIALS)
    assert sorted(placed) == sorted(SPECIALS) and placed["fixed"] == 0 and placed["unmasked"] == E - 1
    s_ref = rr.edge_s(poses, ea.astype(np.int64), eb.astype(np.int64), tf, info)
    assert (s_ref[mask] <= C * C).sum() > E // 20 and (s_ref[mask] > C * C).sum() > E // 5   # both sides of the kinks
    _check_kernel(poses, ea, eb, tf, info, mask, loss, placed)


def _solver(g, loss, **kw):
    from slamhip import robust
    return robust.RobustGaussNewton(np.array(g[0]), g[1], g[2], g[3], loss, C, **kw)


def test_ratio_times_s_is_the_gn_kernels_chi2():
    """At one pose set the sum of ratio x s equals the chi2 the unchanged GN
    iteration reports when it runs with that w: the residual restated in
    robust_kernels.hip is linearize_edge's.  Bound: the s bound weighted by
    the ratios plus the rounding of a sum of E terms."""
    import torch
    from slamhip import gn
    g = rr.outlier_graph(0)
    s = _solver(g, "gm")
    s.reweight()
    r, se = s._r.cpu().numpy().copy(), s._s.cpu().numpy().copy()
    assert np.array_equal(s.w.cpu().numpy(), s.info.cpu().numpy() * r)
    chi = torch.zeros(1, dtype=torch.float64, device=s.poses.device)
    gn.GaussNewton.iterate(s, chi)
    chi2 = float(chi.cpu().numpy()[0])
    ds = _s_bound(np.array(g[0]), g[1], g[2], g[3], go.information(g[1], g[2]))
    bound = float((r * ds).sum()) + (len(r) + 8) * EPS * float((r * se).sum())
    print(f"sum r s {float((r * se).sum())!r}, chi2 {chi2!r}, bound {bound:.3e}")
    assert abs(float((r * se).sum()) - chi2) <= bound
    assert r.min() < 0.01 and chi2 < 0.5 * float(se.sum())   # the weights mattered


@pytest.mark.parametrize("loss", ["gm", "dcs"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solve_matches_irls_and_recovers_the_clean_solution(seed, loss):
    """outlier_graph(seed), c = 0.3, 20 iterations: poses within 1e-8 of
    robust_ref.irls (the tolerance of tests/test_gn.py against the oracle),
    conditions (a)-(c) on the GPU result, and the same bits eager, replayed
    from the HIP graph, and on a second instance."""
    import torch
    g = rr.outlier_graph(seed)
    ref = rr.irls_outlier(seed, loss)
    a = _solver(g, loss)
    cost_a = a.run(20, graph=False)
    pa = a.host_poses().copy()
    print(f"|dP| {np.abs(pa[:, :2] - ref.poses[:, :2]).max():.2e}, |dth| {np.abs(go.wrap(pa[:, 2] - ref.poses[:, 2])).max():.2e}")
    assert np.abs(pa[:, :2] - ref.poses[:, :2]).max() <= 1e-8
    assert np.abs(go.wrap(pa[:, 2] - ref.poses[:, 2])).max() <= 1e-8
    assert np.allclose(cost_a, ref.cost, rtol=1e-8, atol=0)
    assert np.allclose(a.chi2, ref.chi2, rtol=1e-8, atol=0)
    assert np.allclose(a.ratios, ref.ratios, rtol=1e-6, atol=1e-12) and abs(a.final_cost - ref.final_cost) <= 1e-8 * ref.final_cost
    rr.check_abc(pa, a.ratios, seed)
    assert np.array_equal(a.outliers(0.5), np.flatnonzero(g[5]))
    b = _solver(g, loss)
    cost_b = b.run(20, graph=False)
    assert np.array_equal(cost_a, cost_b) and np.array_equal(pa, b.host_poses())
    b.poses.copy_(torch.as_tensor(np.array(g[0]), dtype=torch.float64).reshape(b.poses.shape))
    cost_g = b.run(20, graph=True)
    assert (20, False) in b._graphs or (20, True) in b._graphs
    assert np.array_equal(cost_a, cost_g) and np.array_equal(pa, b.host_poses())
    assert np.array_equal(a.ratios, b.ratios) and np.array_equal(a.chi2, b.chi2)
    b.poses.copy_(torch.as_tensor(np.array(g[0]), dtype=torch.float64).reshape(b.poses.shape))
    assert np.array_equal(cost_a, b.run(20)) and np.array_equal(pa, b.host_poses())   # the cached graph again


@pytest.mark.parametrize("loss", ["huber", "cauchy", "gnc-gm"])
def test_every_loss_matches_irls(loss):
    """Parity of the remaining losses with the restatement (40 iterations for
    gnc-gm, whose mu starts at max(1, 2 max s / c2) and falls by 1.4 per
    iteration); Huber and Cauchy do not recover the clean solution here and
    are not asked to."""
    it = 40 if loss == "gnc-gm" else 20
    g = rr.outlier_graph(0)
    ref = rr.irls_outlier(0, loss, iterations=it)
    a = _solver(g, loss)
    cost = a.run(it)
    p = a.host_poses()
    print(f"{loss}: |dP| {np.abs(p[:, :2] - ref.poses[:, :2]).max():.2e}, mu {a.mu!r} (ref {ref.mu!r})")
    assert np.abs(p[:, :2] - ref.poses[:, :2]).max() <= 1e-8
    assert np.abs(go.wrap(p[:, 2] - ref.poses[:, 2])).max() <= 1e-8
    assert np.allclose(cost, ref.cost, rtol=1e-8, atol=0)
    if loss == "gnc-gm":
        assert a.mu == ref.mu == 1.0 and not a._graphs
        cost2 = a.run(3)            # a second run restarts mu from the residuals then present
        assert len(cost2) == 3 and not a._graphs
    with_tol = _solver(g, loss)
    hist = with_tol.run(it, tol=1e-6)
    assert 2 <= len(hist) <= it and np.array_equal(hist, cost[:len(hist)]) and len(with_tol.chi2) == len(hist)


def _with_wrong_edges(case, n=3):
    """The gn_step case's graph plus n wrong edges of span <= dmax (the band and
    the block structure stay the case's)."""
    guess, ea, eb, tf = gn_step.case_graph(case)
    rng = np.random.default_rng(77)
    xa, xb, xt = [], [], []
    while len(xa) < n:
        a = int(rng.integers(1, case.N - case.dmax))
        b = a + int(rng.integers(2, case.dmax + 1))
        if a in case.border or b in case.border:
            continue
        xa.append(a)
        xb.append(b)
        xt.append(rr.pose_mat(*rng.uniform([-2, -2, -3], [2, 2, 3])))
    wrong = np.r_[np.zeros(len(ea), dtype=bool), np.ones(n, dtype=bool)]
    return np.array(guess), np.r_[ea, xa], np.r_[eb, xb], np.concatenate([tf, np.stack(xt)]), wrong


@pytest.mark.parametrize("name", ["N70_d4", "N70_d4_b2"])
def test_solver_paths(name):
    """The gm solve through the plain band entry point (block cyclic
    reduction) and through the bordered Schur entry point: tests/gn_step.py's
    cases with 3 wrong edges added, planned in natural order as there."""
    from slamhip import gn, robust
    case = gn_step.BY_NAME[name]
    guess, ea, eb, tf, wrong = _with_wrong_edges(case)
    plan = gn.GnPlan(case.N, ea, eb, order=np.arange(case.N), border=list(case.border))
    assert plan.W == case.W and gn_step.block_shape(plan)[0] == case.wb
    if case.border:
        assert plan.nv_band < plan.nv and plan.pslot is not None
    else:
        assert plan.nv_band == plan.nv
    ref = rr.irls(guess, ea, eb, tf, "gm", C, 20)
    s = robust.RobustGaussNewton(guess, ea, eb, tf, "gm", C, plan=plan)
    cost = s.run(20)
    p = s.host_poses()
    print(f"{name}: |dP| {np.abs(p[:, :2] - ref.poses[:, :2]).max():.2e}, wrong-edge ratios {s.ratios[wrong]}")
    assert np.abs(p[:, :2] - ref.poses[:, :2]).max() <= 1e-8
    assert np.abs(go.wrap(p[:, 2] - ref.poses[:, 2])).max() <= 1e-8
    assert np.allclose(cost, ref.cost, rtol=1e-8, atol=0)
    assert np.allclose(s.ratios, ref.ratios, rtol=1e-6, atol=1e-12)
    assert np.all(p[0] == guess[0])


@pytest.mark.parametrize("loss,graph", [("gm", False), ("gm", True), ("gnc-gm", False)])
def test_fused_back_substitution_fallback(loss, graph):
    """With the fused back-substitution's wait forced down to one tick (as
    tests/test_gn.py does) every fused step times out and GaussNewton restores
    the poses and re-runs with a launch per level: the robust run gives the
    same bits (all three pose components, costs, ratios) as one that never
    fell back (w is recomputed from the restored poses, gnc-gm's mu starts
    over).  With `graph` the timeout strikes a replayed graph: the base class
    drops its graphs and captures the overridden iterate again, with the
    partial rows starting over."""
    from slamhip import _abi, gn, robust, synthetic
    lib = _abi.lib()
    guess, ea, eb, tf, _ = synthetic.lap_graph_c4()
    try:
        assert lib.slam_gn_set_fused_back(1) == 0
        a = robust.RobustGaussNewton(guess, ea, eb, tf, loss, C)
        assert a.plan.pslot is not None and a.plan.nv_band < a.plan.nv
        cost_a = np.concatenate([a.run(1, graph=False), a.run(5, graph=False)])
        assert lib.slam_gn_get_fused_back() == 1
        n_fb = gn.FUSED_BACK_FALLBACKS
        c = robust.RobustGaussNewton(guess, ea, eb, tf, loss, C)
        first = c.run(1, graph=False) if graph else None   # the eager step before the wait is cut
        assert lib.slam_gn_set_fused_wait(1) == 0
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            if graph:
                cost_c = np.concatenate([first, c.run(5, graph=True)])
                assert list(c._graphs) == [(5, False)]   # captured again without the fused kernel
            else:
                cost_c = np.concatenate([c.run(1, graph=False), c.run(5, graph=False)])
        assert any("timed out" in str(x.message) for x in w)
        assert lib.slam_gn_get_fused_back() == 0 and gn.FUSED_BACK_FALLBACKS == n_fb + 1
        assert np.array_equal(cost_a, cost_c)
        assert np.array_equal(a.host_poses(), c.host_poses())
        assert np.array_equal(a.ratios, c.ratios) and a.mu == c.mu
        assert a.ratios[a.mask].min() < 1.0
    finally:
        lib.slam_gn_set_fused_wait(0)
        lib.slam_gn_set_fused_back(1)


def _pose_graph(seed):
    """outlier_graph(seed) as a PoseGraph: constructor odometry edges from the
    dead-reckoned guess, every closure (right and wrong) through add_constraint."""
    import src.pose_graph as pgm
    guess, ea, eb, tf, truth, wrong = rr.outlier_graph(seed)
    pg = pgm.PoseGraph(np.array(guess))
    loops = np.flatnonzero(rr.loop_mask(ea, eb))
    assert len({(int(ea[e]), int(eb[e])) for e in loops}) == len(loops)
    for e in loops:
        pg.add_constraint(int(ea[e]), int(eb[e]), np.array(tf[e]), convention="relative")
    return pg


def _ratios_in_graph_order(wts, seed):
    _, ea, eb, _, _, _ = rr.outlier_graph(seed)
    at = {(int(a), int(b)): r for a, b, r in zip(wts["ea"], wts["eb"], wts["ratio"])}
    return np.array([at[(int(a), int(b))] for a, b in zip(ea, eb)])


def test_drop_in_and_pipeline():
    """optimize_pose_graph(loss="gm", loss_scale=0.3, return_weights=True) on a
    160-node PoseGraph with wrong closures meets (a)-(c); loss=None is the
    plain call bit for bit; pipeline.optimize(gn_drop_below=0.5) removes
    exactly the wrong closures."""
    import src.pose_graph_optimization as pgo
    from slamhip import pipeline
    seed = 0
    _, ea, eb, _, truth, wrong = rr.outlier_graph(seed)
    pg = _pose_graph(seed)
    obj = pg.poses
    hist, wts = pgo.optimize_pose_graph(pg, iterations=20, loss="gm", loss_scale=C, return_weights=True,
                                        return_history=True)
    assert pg.poses is obj and len(hist) == 20 and hist[-1] < hist[0]
    assert len(wts["ratio"]) == len(ea) and wts["robust"].sum() == rr.loop_mask(ea, eb).sum()
    rr.check_abc(pg.poses, _ratios_in_graph_order(wts, seed), seed)
    assert pgo.optimize_pose_graph(_pose_graph(seed), iterations=3, loss="dcs", loss_scale=C) is None

    p1, p2 = _pose_graph(seed), _pose_graph(seed)
    h1 = pgo.optimize_pose_graph(p1, iterations=5, return_history=True)
    h2 = pgo.optimize_pose_graph(p2, iterations=5, return_history=True, loss=None, loss_scale=C, robust_edges="all")
    assert np.array_equal(p1.poses, p2.poses) and np.array_equal(h1, h2)

    pg = _pose_graph(seed)
    n_edges = pg.graph.number_of_edges()
    rep = {}
    pipeline.optimize(pg, None, method="gn", gn_iterations=20, gn_loss="gm", gn_loss_scale=C, gn_drop_below=0.5,
                      report=rep)
    want = sorted((int(a), int(b)) for a, b in zip(ea[wrong], eb[wrong]))
    assert sorted(rep["gn_dropped"]) == want
    assert pg.graph.number_of_edges() == n_edges - len(want) and not any(pg.graph.has_edge(a, b) for a, b in want)
    assert rr.max_position_error(pg.poses, truth) <= 1.10 * rr.clean_error(seed)
    with pytest.raises(ValueError):
        pipeline.optimize(_pose_graph(seed), None, method="sgd", gn_loss="gm")
