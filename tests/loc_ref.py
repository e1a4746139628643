"""NumPy restatement of the localisation in a finished occupancy grid
(include/slamhip.h, the section of csrc/loc_kernels.hip): the field, the window
search and the sub-cell refinement.  Not a test module; the yardstick of
tests/test_loc.py and tests/test_loc_gpu.py.

The field and the search are integers: they are compared bit for bit.  The
refinement is fp64 with every product and sum rounded on its own, as NumPy
elementwise code does; its eleven sums are ``np.sum`` here and a fixed tree on
the device, and cos / sin of the pose's angle are NumPy's here: the two places
where the last bits may differ.
"""
import numpy as np

CONVERGED, MAX_ITERS, SINGULAR, TOO_FEW = 0, 1, 2, 3
REFINE_DEFAULTS = dict(max_iters=30, eps_t=1e-4, eps_r=1e-4, min_inlier_frac=0.5, pivot_tol=1e-9)


def field(grid, d_cap, occ_min=0):
    """(H, W) uint16: min(d_cap^2, squared cell distance to the nearest cell with
    grid > occ_min).  Two passes: the capped vertical distance per column, then
    the minimum of g^2 + dx^2 over |dx| <= d_cap per row."""
    occ = np.asarray(grid).astype(np.int64) > occ_min
    H, W = occ.shape
    g = np.full((H, W), d_cap, dtype=np.int64)
    d = np.full(W, d_cap, dtype=np.int64)
    for r in range(H):
        d = np.where(occ[r], 0, np.minimum(d + 1, d_cap))
        g[r] = d
    d = np.full(W, d_cap, dtype=np.int64)
    for r in range(H - 1, -1, -1):
        d = np.where(occ[r], 0, np.minimum(d + 1, d_cap))
        g[r] = np.minimum(g[r], d)
    g2 = np.full((H, W + 2 * d_cap), d_cap * d_cap, dtype=np.int64)
    g2[:, d_cap:d_cap + W] = g * g
    F = np.full((H, W), d_cap * d_cap, dtype=np.int64)
    for dx in range(-d_cap, d_cap + 1):
        F = np.minimum(F, g2[:, d_cap + dx:d_cap + dx + W] + dx * dx)
    return F.astype(np.uint16)


def field_brute(grid, d_cap, occ_min=0):
    """The definition itself, O(cells x occupied cells): small grids only."""
    occ = np.asarray(grid).astype(np.int64) > occ_min
    H, W = occ.shape
    rr, cc = np.nonzero(occ)
    F = np.full((H, W), d_cap * d_cap, dtype=np.int64)
    if len(rr):
        r, c = np.mgrid[0:H, 0:W]
        d2 = (r[..., None] - rr) ** 2 + (c[..., None] - cc) ** 2
        F = np.minimum(F, d2.min(axis=2))
    return F.astype(np.uint16)


def rotations(theta0, n_theta, d_theta):
    """(n_theta, 2) cos / sin of the angle bins, one scalar call per angle."""
    half = n_theta // 2
    th0, d = float(theta0), float(d_theta)
    return np.array([(np.cos(th0 + (k - half) * d), np.sin(th0 + (k - half) * d)) for k in range(n_theta)])


def cells(pts, c, s, x0, y0, origin, cw):
    """Integer cells (cx, cy) of a scan at one rotation and centre; clipped in
    fp64 far outside any grid before the conversion, like the device.  A cell
    that is not finite (a coordinate that overflowed to inf, or inf - inf = NaN)
    is outside the map: NaN goes to the low end, as the device's fmax does."""
    px, py = pts[:, 0], pts[:, 1]
    big = 2.0 ** 40
    with np.errstate(over="ignore", invalid="ignore"):
        gx = (c * px - s * py) + x0
        gy = (s * px + c * py) + y0
        cx = np.floor((gx - origin[0]) / cw)
        cy = np.floor((gy - origin[1]) / cw)
        cx = np.where(np.isnan(cx), -big, np.clip(cx, -big, big))
        cy = np.where(np.isnan(cy), -big, np.clip(cy, -big, big))
    return cx.astype(np.int64), cy.astype(np.int64)


def search(F, origin, cw, d_cap, pts, centre, n_theta, d_theta, nx, ny, step):
    """(costs (n_theta, ny, nx) int32, (cost, k, j, i) of the minimum with the
    smallest flat index) of one query; ``centre`` = (theta0, x0, y0)."""
    F = np.asarray(F).astype(np.int64)
    H, W = F.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    cap2 = d_cap * d_cap
    rot = rotations(centre[0], n_theta, d_theta)
    sj = (np.arange(ny) - ny // 2) * step
    si = (np.arange(nx) - nx // 2) * step
    costs = np.zeros((n_theta, ny, nx), dtype=np.int64)
    for k in range(n_theta):
        cx, cy = cells(pts, rot[k, 0], rot[k, 1], float(centre[1]), float(centre[2]), origin, cw)
        rows = cy[:, None, None] + sj[None, :, None]
        cols = cx[:, None, None] + si[None, None, :]
        inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
        v = np.where(inside, F[np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)], cap2)
        costs[k] = v.sum(axis=0)
    assert costs.max(initial=0) < 2 ** 31
    flat = int(np.argmin(costs.reshape(-1)))   # the first minimum: the smallest flat index
    k, rem = divmod(flat, ny * nx)
    j, i = divmod(rem, nx)
    return costs.astype(np.int32), (int(costs[k, j, i]), k, j, i)


def assemble(centre, kji, n_theta, d_theta, nx, ny, step, cw):
    """(x, y, theta) of bin (k, j, i) around ``centre`` = (theta0, x0, y0)."""
    k, j, i = kji
    return np.array([centre[1] + (int(i) - nx // 2) * step * cw, centre[2] + (int(j) - ny // 2) * step * cw,
                     float(centre[0]) + (int(k) - n_theta // 2) * float(d_theta)])


def reloc_shape(H, W, origin, cw, nx, ny, step, d_theta):
    """(n_theta, d_theta, centres (T, 3) = (0, x0, y0), row-major in (ty, tx)) of
    the windows that tile the whole map with the angle bins over the full circle."""
    n_theta = max(1, int(round(2 * np.pi / abs(float(d_theta)))))
    out = []
    for ty in range(-(-H // (ny * step))):
        for tx in range(-(-W // (nx * step))):
            out.append((0.0, origin[0] + ((tx * nx + nx // 2) * step + 0.5) * cw,
                        origin[1] + ((ty * ny + ny // 2) * step + 0.5) * cw))
    return n_theta, 2 * np.pi / n_theta, np.array(out)


def relocalize(F, origin, cw, d_cap, pts, nx, ny, step, d_theta):
    """(cost, tile, (k, j, i), pose (x, y, theta)) of the cheapest bin over all
    tiles, ties to the first tile and then the smallest flat index."""
    H, W = np.asarray(F).shape
    n_theta, d, centres = reloc_shape(H, W, origin, cw, nx, ny, step, d_theta)
    best = None
    for t, c in enumerate(centres):
        _, (cost, k, j, i) = search(F, origin, cw, d_cap, pts, c, n_theta, d, nx, ny, step)
        if best is None or cost < best[0]:
            best = (cost, t, (k, j, i))
    return best + (assemble(centres[best[1]], best[2], n_theta, d, nx, ny, step, cw),)


def linearise(F, origin, cw, d_cap, pts, pose, rng=None):
    """One linearisation at ``pose`` = (x, y, theta): m, H (3, 3), g (3,), e."""
    F = np.asarray(F)
    Hc, W = F.shape
    x, y, th = (np.float64(v) for v in pose)
    c, s = np.cos(th), np.sin(th)
    px, py = pts[:, 0], pts[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):   # a point that overflows is not on the field
        gx = ((c * px) - (s * py)) + x
        gy = ((s * px) + (c * py)) + y
        u = ((gx - origin[0]) / cw) - 0.5
        v = ((gy - origin[1]) / cw) - 0.5
        fu, fv = np.floor(u), np.floor(v)
        ok = (fu >= 0) & (fu <= W - 2) & (fv >= 0) & (fv <= Hc - 2)
    i0 = np.where(ok, fu, 0).astype(np.int64)
    j0 = np.where(ok, fv, 0).astype(np.int64)
    if W < 2 or Hc < 2:
        ok[:] = False
        i0[:] = j0[:] = 0
        f00 = f10 = f01 = f11 = np.zeros(len(pts), dtype=np.int64)
    else:
        f00, f10 = F[j0, i0].astype(np.int64), F[j0, i0 + 1].astype(np.int64)
        f01, f11 = F[j0 + 1, i0].astype(np.int64), F[j0 + 1, i0 + 1].astype(np.int64)
    cap2 = d_cap * d_cap
    inl = ok & ~((f00 == cap2) & (f10 == cap2) & (f01 == cap2) & (f11 == cap2))
    a, b = u[inl] - fu[inl], v[inl] - fv[inl]
    a1, b1 = 1.0 - a, 1.0 - b
    D00, D10 = np.sqrt(f00[inl].astype(np.float64)) * cw, np.sqrt(f10[inl].astype(np.float64)) * cw
    D01, D11 = np.sqrt(f01[inl].astype(np.float64)) * cw, np.sqrt(f11[inl].astype(np.float64)) * cw
    r = (b1 * ((a1 * D00) + (a * D10))) + (b * ((a1 * D01) + (a * D11)))
    jx = ((b1 * (D10 - D00)) + (b * (D11 - D01))) / cw
    jy = ((a1 * (D01 - D00)) + (a * (D11 - D10))) / cw
    qx, qy = px[inl], py[inl]
    jt = (jx * ((-s * qx) - (c * qy))) + (jy * ((c * qx) - (s * qy)))
    A = np.stack([jx, jy, jt], axis=1).reshape(-1, 3)
    if rng is not None:
        p = rng.permutation(len(r))
        A, r = A[p], r[p]
    Hm = np.array([[(A[:, p] * A[:, q]).sum() for q in range(3)] for p in range(3)])
    g = np.array([(A[:, p] * r).sum() for p in range(3)])
    return int(inl.sum()), Hm, g, (r * r).sum()


def solve(H, g, pivot_tol):
    """(dx, dy, dth) = -H^-1 g by LDL^T, or None at a bad pivot (PLICP's rule)."""
    def bad(d, hkk):
        return not np.isfinite(d) or d <= pivot_tol * hkk

    with np.errstate(all="ignore"):
        d0 = H[0, 0]
        if bad(d0, H[0, 0]):
            return None
        l10, l20 = H[0, 1] / d0, H[0, 2] / d0
        d1 = H[1, 1] - (l10 * H[0, 1])
        if bad(d1, H[1, 1]):
            return None
        u = H[1, 2] - (l20 * H[0, 1])
        l21 = u / d1
        d2 = (H[2, 2] - (l20 * H[0, 2])) - (l21 * u)
        if bad(d2, H[2, 2]):
            return None
        z0 = -g[0]
        z1 = -g[1] - (l10 * z0)
        z2 = (-g[2] - (l20 * z0)) - (l21 * z1)
        dth = z2 / d2
        dy = (z1 / d1) - (l21 * dth)
        dx = ((z0 / d0) - (l10 * dy)) - (l20 * dth)
    return dx, dy, dth


def refine(F, origin, cw, d_cap, pts, pose, max_iters=30, eps_t=1e-4, eps_r=1e-4, min_inlier_frac=0.5,
           pivot_tol=1e-9, rng=None):
    """Gauss-Newton on the field in metres from ``pose`` = (x, y, theta): a dict
    with pose, iters, inliers, status, rms."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    x, y, th = (np.float64(v) for v in pose)
    it = 0
    while True:
        m, H, g, e = linearise(F, origin, cw, d_cap, pts, (x, y, th), rng)
        with np.errstate(all="ignore"):
            rms = np.sqrt(np.float64(e) / np.float64(m))
        if m == 0 or np.float64(m) < np.float64(min_inlier_frac) * np.float64(len(pts)):
            status = TOO_FEW
            break
        delta = solve(H, g, pivot_tol)
        if delta is None:
            status = SINGULAR
            break
        dx, dy, dth = delta
        x, y, th = x + dx, y + dy, th + dth
        it += 1
        if np.sqrt((dx * dx) + (dy * dy)) < eps_t and abs(dth) < eps_r:
            status = CONVERGED
            break
        if it == max_iters:
            status = MAX_ITERS
            break
    return dict(pose=np.array([x, y, th]), iters=it, inliers=m, status=status, rms=rms)


# ---- the end-to-end experiment shared by tests/test_loc.py and tests/test_loc_gpu.py ----

E2E = dict(n_scans=600, seed=5, n_beams=361, cell_width=0.05, d_cap=20, every=15, shift=0.4, turn=0.2, guess_seed=11,
           n_theta=41, d_theta=0.0125, nx=21, ny=21, step=1)
# Largest error of THIS restatement on the experiment's inputs (measured on the CPU with the map of
# oracle/occupancy_oracle.py), and the test bound of twice that.
E2E_MEASURED = (0.06996, 0.007692)   # m (scan 331), rad (scan 391); tests/test_loc.py re-measures them
E2E_BOUND = (2 * E2E_MEASURED[0], 2 * E2E_MEASURED[1])
# Held-out scans whose cheapest bin over the whole map (step 2 cells, 3 degree bins) is the true pose,
# chosen with this restatement on the CPU; all eight tried (31, 91, 151, 211, 271, 391, 451, 511) were.
RELOC_SCANS = (31, 151, 271, 511)
RELOC = dict(nx=21, ny=21, step=2, d_theta=np.deg2rad(3.0))


def e2e_inputs():
    """(seq, map scan indices, held-out scan indices, guesses (x, y, theta)) of the
    experiment: the map from the even scans of the first lap at their true poses,
    every 15th remaining scan of that lap moved by a seeded uniform +-0.4 m per
    axis and +-0.2 rad."""
    from slamhip import synthetic
    seq = synthetic.make_loop_sequence(E2E["n_scans"], seed=E2E["seed"], n_beams=E2E["n_beams"])
    lap = np.arange(seq.per_lap)
    map_idx = lap[lap % 2 == 0]
    held = lap[lap % 2 == 1][::E2E["every"]]
    rng = np.random.default_rng(E2E["guess_seed"])
    guess = seq.truth[held].copy()
    guess[:, :2] += rng.uniform(-E2E["shift"], E2E["shift"], size=(len(held), 2))
    guess[:, 2] += rng.uniform(-E2E["turn"], E2E["turn"], size=len(held))
    return seq, map_idx, held, guess


def pose_error(pose, truth):
    """(position error (m), heading error (rad)) rows."""
    pose, truth = np.atleast_2d(pose), np.atleast_2d(truth)
    d = pose[:, 2] - truth[:, 2]
    return np.hypot(pose[:, 0] - truth[:, 0], pose[:, 1] - truth[:, 1]), np.abs(np.arctan2(np.sin(d), np.cos(d)))


def localize(F, origin, cw, d_cap, pts, guess, **refine_kw):
    """Search around ``guess`` (x, y, theta) with the experiment's window, then
    refine: ((cost, k, j, i), the refinement's dict)."""
    w = {k: E2E[k] for k in ("n_theta", "d_theta", "nx", "ny", "step")}
    centre = (guess[2], guess[0], guess[1])
    _, best = search(F, origin, cw, d_cap, pts, centre, **w)
    start = assemble(centre, best[1:], w["n_theta"], w["d_theta"], w["nx"], w["ny"], w["step"], cw)
    return best, refine(F, origin, cw, d_cap, pts, start, **refine_kw)


# ---- the hand-made refinement case shared by tests/test_loc.py and tests/test_loc_gpu.py ----

def refine_case():
    """A 60 x 80 map of 0.1 m cells (a walled box with a block inside; free and
    unknown cells of both signs) and a 111-point scan taken at ``truth`` whose
    points lie on the centres of occupied cells: (grid, origin, cw, d_cap, pts,
    truth (x, y, theta))."""
    g = np.zeros((60, 80), np.int8)
    g[10, 10:71] = 5
    g[50, 10:71] = 5
    g[10:51, 10] = 5
    g[10:51, 70] = 5
    g[25:31, 40:47] = 9
    g[26:30, 41:46] = -3
    origin, cw = np.array([-1.0, -0.5]), 0.1
    rr, cc = np.nonzero(g > 0)
    wx, wy = origin[0] + (cc + 0.5) * cw, origin[1] + (rr + 0.5) * cw
    truth = np.array([2.2, 1.9, 0.3])
    c, s = np.cos(truth[2]), np.sin(truth[2])
    dx, dy = wx - truth[0], wy - truth[1]
    pts = np.stack([c * dx + s * dy, -s * dx + c * dy], axis=1)[::2]
    return g, origin, cw, 8, pts, truth
