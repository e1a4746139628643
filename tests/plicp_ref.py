"""NumPy restatement of the point-to-line refinement (include/slamhip.h, the
section of csrc/plicp_kernels.hip): fp64, every product and sum rounded on its
own, as NumPy elementwise code does.  Not a test module; the yardstick of
tests/test_plicp.py and tests/test_plicp_gpu.py.

Every comparison (supports, corner test, matches, gate, pivots, stop) is made
on the same bits as on the device.  The ten sums of a linearisation are the
only place where the order of the operations is the implementation's own: here
``np.sum`` over the rows (optionally shuffled by ``rng``), on the device a
fixed tree; both are plain fp64 sums.
"""
import numpy as np

CONVERGED, MAX_ITERS, DEGENERATE, TOO_FEW = 0, 1, 2, 3
DEFAULTS = dict(max_dist=0.5, min_inliers=10, max_iters=50, eps_t=5e-4, eps_r=5e-4, pivot_tol=1e-9)
NORMAL_DEFAULTS = dict(K=8, rho=0.15, ctol=0.03)


def scan_normals(Q, K=8, rho=0.15, ctol=0.03):
    """(n, 2) normals, (0, 0) for none, and the (n,) bool ``has`` of one scan."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 2)
    n = len(Q)
    rho2 = np.float64(rho) * np.float64(rho)
    N = np.zeros((n, 2))
    has = np.zeros(n, dtype=bool)

    def d2(a, b):
        dx, dy = Q[a, 0] - Q[b, 0], Q[a, 1] - Q[b, 1]
        return (dx * dx) + (dy * dy)

    for j in range(n):
        l = j
        while l > 0 and j - l < K and d2(l - 1, j) <= rho2:
            l -= 1
        r = j
        while r < n - 1 and r - j < K and d2(r + 1, j) <= rho2:
            r += 1
        if r - l < 2:
            continue
        tx, ty = Q[r, 0] - Q[l, 0], Q[r, 1] - Q[l, 1]
        L2 = (tx * tx) + (ty * ty)
        if not (L2 > 0 and np.isfinite(L2)):
            continue
        L = np.sqrt(L2)
        nx, ny = -ty / L, tx / L
        off = (nx * (Q[j, 0] - Q[l, 0])) + (ny * (Q[j, 1] - Q[l, 1]))
        if abs(off) > ctol:
            continue
        N[j] = (nx, ny)
        has[j] = True
    return N, has


def normals_packed(pts, off, **kw):
    """The (P, 2) normals of packed scans; a scan with bad offsets gets none.
    Returns (normals, flagged)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    P = len(pts)
    out = np.zeros((P, 2))
    flagged = False
    for s in range(len(off) - 1):
        p0, p1 = int(off[s]), int(off[s + 1])
        if p0 < 0 or p1 < p0 or p1 > P:
            flagged = True
            continue
        out[p0:p1] = scan_normals(pts[p0:p1], **kw)[0]
    return out, flagged


def nearest(x, y, Q, chunk=256):
    """(j*, d2 min) per query: the smallest index of the minimum (np.argmin)."""
    n = len(x)
    j = np.zeros(n, dtype=np.int64)
    dm = np.full(n, np.inf)
    if len(Q) == 0:
        return j, dm
    for a in range(0, n, chunk):
        dx = x[a:a + chunk, None] - Q[None, :, 0]
        dy = y[a:a + chunk, None] - Q[None, :, 1]
        d = (dx * dx) + (dy * dy)
        jj = d.argmin(axis=1)
        j[a:a + chunk] = jj
        dm[a:a + chunk] = d[np.arange(len(jj)), jj]
    return j, dm


def linearise(P, Q, N, T, max_dist2, rng=None):
    """One linearisation at T: a dict with match (-1: outlier), m, the rows'
    sums H (3, 3), g (3,), e, and the smallest relative distance of an inlier
    test from the gate (``gate_margin``)."""
    x = ((T[0, 0] * P[:, 0]) + (T[0, 1] * P[:, 1])) + T[0, 2]
    y = ((T[1, 0] * P[:, 0]) + (T[1, 1] * P[:, 1])) + T[1, 2]
    j, dm = nearest(x, y, Q)
    inl = dm <= max_dist2
    m = int(inl.sum())
    match = np.where(inl, j, -1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(dm / max_dist2 - 1.0) if max_dist2 > 0 else np.full(len(dm), np.inf)
    ji = j[inl]
    xi, yi = x[inl], y[inl]
    if len(Q):
        ex, ey = xi - Q[ji, 0], yi - Q[ji, 1]
        nx, ny = N[ji, 0], N[ji, 1]
    else:
        ex = ey = nx = ny = np.zeros(0)
    has = (nx != 0) | (ny != 0)
    one, zero = np.ones(int((~has).sum())), np.zeros(int((~has).sum()))
    A = np.concatenate([
        np.stack([nx[has], ny[has], (ny[has] * xi[has]) - (nx[has] * yi[has])], axis=1).reshape(-1, 3),
        np.stack([one, zero, -yi[~has]], axis=1).reshape(-1, 3),
        np.stack([zero, one, xi[~has]], axis=1).reshape(-1, 3)])
    r = np.concatenate([(nx[has] * ex[has]) + (ny[has] * ey[has]), ex[~has], ey[~has]])
    if rng is not None:
        p = rng.permutation(len(r))
        A, r = A[p], r[p]
    H = np.array([[(A[:, a] * A[:, b]).sum() for b in range(3)] for a in range(3)])
    g = np.array([(A[:, a] * r).sum() for a in range(3)])
    e = (r * r).sum()
    return dict(match=match, m=m, H=H, g=g, e=e, gate_margin=rel, dmin=dm)


def solve(H, g, pivot_tol):
    """(delta (dx, dy, dth) or None when degenerate, the pivot ratios d_k / H_kk
    that were computed)."""
    ratios = []

    def bad(d, hkk):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios.append(d / hkk)
        return not np.isfinite(d) or d <= pivot_tol * hkk

    with np.errstate(all="ignore"):
        d0 = H[0, 0]
        if bad(d0, H[0, 0]):
            return None, ratios
        l10, l20 = H[0, 1] / d0, H[0, 2] / d0
        d1 = H[1, 1] - (l10 * H[0, 1])
        if bad(d1, H[1, 1]):
            return None, ratios
        u = H[1, 2] - (l20 * H[0, 1])
        l21 = u / d1
        d2 = (H[2, 2] - (l20 * H[0, 2])) - (l21 * u)
        if bad(d2, H[2, 2]):
            return None, ratios
        z0 = -g[0]
        z1 = -g[1] - (l10 * z0)
        z2 = (-g[2] - (l20 * z0)) - (l21 * z1)
        dth = z2 / d2
        dy = (z1 / d1) - (l21 * dth)
        dx = ((z0 / d0) - (l10 * dy)) - (l20 * dth)
    return (dx, dy, dth), ratios


def observability(H):
    with np.errstate(all="ignore"):
        h = (H[0, 0] + H[1, 1]) / 2.0
        q2 = (h * h) - ((H[0, 0] * H[1, 1]) - (H[0, 1] * H[0, 1]))
        q = np.sqrt(q2 if q2 > 0 else 0.0)
        return np.float64(h - q) / np.float64(h + q)


def refine(P, Q, N, T0, max_dist=0.5, min_inliers=10, max_iters=50, eps_t=5e-4, eps_r=5e-4, pivot_tol=1e-9, rng=None,
           trace=None):
    """The refinement of one pair: a dict with tf, err, obs, inliers, iters,
    status, match.  ``trace`` (a list) receives per linearisation a dict with
    the steps' ratios to eps, the pivot ratios and the gate margins, for the
    fixture conditions of tests/test_plicp.py."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 2)
    T = np.array(T0, dtype=np.float64).reshape(3, 3).copy()
    T[2] = (0.0, 0.0, 1.0)
    max_dist2 = np.float64(max_dist) * np.float64(max_dist)
    it = 0
    while True:
        lin = linearise(P, Q, N, T, max_dist2, rng)
        m, H, g = lin["m"], lin["H"], lin["g"]
        with np.errstate(all="ignore"):
            err = np.float64(lin["e"]) / np.float64(m)
        obs = observability(H)
        rec = dict(gate_margin=lin["gate_margin"], dmin=lin["dmin"], pivots=[], step=None)
        if trace is not None:
            trace.append(rec)
        if m < min_inliers:
            status = TOO_FEW
            break
        delta, rec["pivots"] = solve(H, g, pivot_tol)
        if delta is None:
            status = DEGENERATE
            break
        dx, dy, dth = delta
        c, s = np.cos(dth), np.sin(dth)
        Tn = T.copy()
        Tn[0, 0] = (c * T[0, 0]) - (s * T[1, 0])
        Tn[0, 1] = (c * T[0, 1]) - (s * T[1, 1])
        Tn[0, 2] = ((c * T[0, 2]) - (s * T[1, 2])) + dx
        Tn[1, 0] = (s * T[0, 0]) + (c * T[1, 0])
        Tn[1, 1] = (s * T[0, 1]) + (c * T[1, 1])
        Tn[1, 2] = ((s * T[0, 2]) + (c * T[1, 2])) + dy
        T = Tn
        it += 1
        rec["step"] = (abs(dx) / eps_t if eps_t > 0 else np.inf, abs(dy) / eps_t if eps_t > 0 else np.inf,
                       abs(dth) / eps_r if eps_r > 0 else np.inf)
        if abs(dx) < eps_t and abs(dy) < eps_t and abs(dth) < eps_r:
            status = CONVERGED
            break
        if it == max_iters:
            status = MAX_ITERS
            break
    return dict(tf=T, err=err, obs=obs, inliers=m, iters=it, status=status, match=lin["match"])


def refine_packed(pts, off, src, dst, init, normals=None, rng=None, traces=None, **kw):
    """B pairs over packed scans, as slam_plicp_batch_f64: a list of dicts."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    nk = {k: kw.pop(k) for k in ("K", "rho", "ctol") if k in kw}
    if normals is None:
        normals = normals_packed(pts, off, **nk)[0]
    out = []
    for b, (s, d) in enumerate(zip(src, dst)):
        tr = [] if traces is not None else None
        out.append(refine(pts[off[s]:off[s + 1]], pts[off[d]:off[d + 1]], normals[off[d]:off[d + 1]],
                          np.asarray(init, dtype=np.float64).reshape(-1, 3, 3)[b], rng=rng, trace=tr, **kw))
        if traces is not None:
            traces.append(tr)
    return out


def apply_refinement(tf, n_src, res, min_overlap=0.5, min_observability=0.0):
    out = np.array(tf, dtype=np.float64).reshape(-1, 3, 3).copy()
    take = np.zeros(len(out), dtype=bool)
    for b, r in enumerate(res):
        if r["status"] in (CONVERGED, MAX_ITERS) and r["inliers"] >= min_overlap * n_src[b] and \
                r["obs"] >= min_observability:
            out[b] = r["tf"]
            take[b] = True
    return out, take
