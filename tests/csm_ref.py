"""NumPy restatement of the correlative scan matcher's definition
(include/slamhip.h, "correlative scan matcher"): the yardstick of
tests/test_csm.py and tests/test_csm_gpu.py, written from the definition and
not from the kernel (plain G x G table, explicit bounds tests, no border)."""
import numpy as np


def origin(G, res):
    return -(G // 2) * res


def lookup_table(ref, G, res):
    """L (G, G) uint8, row = y: 2 on cells holding a point of ``ref`` (n, 2),
    1 on their 8 neighbours that hold none, 0 elsewhere."""
    o = origin(G, res)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 2)
    cx = np.floor((ref[:, 0] - o) / res)
    cy = np.floor((ref[:, 1] - o) / res)
    L = np.zeros((G, G), dtype=np.uint8)
    for value, shifts in ((1, [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), (2, [(0, 0)])):
        for dy, dx in shifts:
            x, y = cx + dx, cy + dy                        # floats: no overflow for far points
            ok = (x >= 0) & (x < G) & (y >= 0) & (y < G)   # each cell clipped on its own
            L[y[ok].astype(np.int64), x[ok].astype(np.int64)] = value
    return L


def angle_table(th0, n_theta, d_theta):
    """(n_theta, 2): np.cos / np.sin of th0 + (k - n_theta // 2) * d_theta, one scalar call each."""
    th0, d_theta = float(th0), float(d_theta)
    return np.array([(np.cos(th0 + (k - n_theta // 2) * d_theta), np.sin(th0 + (k - n_theta // 2) * d_theta))
                     for k in range(n_theta)]).reshape(n_theta, 2)


def score_volume(query, ref, centre=(0.0, 0.0, 0.0), res=0.05, G=512, n_theta=240, d_theta=2 * np.pi / 240,
                 nx=61, ny=61):
    """S (n_theta, ny, nx) int32 and the (n_theta, 2) cos / sin table."""
    o = origin(G, res)
    L = lookup_table(ref, G, res)
    q = np.asarray(query, dtype=np.float64).reshape(-1, 2)
    th0, tx0, ty0 = (float(v) for v in centre)
    cs = angle_table(th0, n_theta, d_theta)
    c, s = cs[:, 0:1], cs[:, 1:2]
    x, y = q[None, :, 0], q[None, :, 1]
    X = (c * x - s * y) + tx0
    Y = (s * x + c * y) + ty0
    ix = np.floor((X - o) / res)      # (n_theta, n) floats: integers, exact far beyond int32
    iy = np.floor((Y - o) / res)
    S = np.zeros((n_theta, ny, nx), dtype=np.int32)
    for j in range(ny):
        yy = iy + (j - ny // 2)
        oky = (yy >= 0) & (yy < G)
        yi = np.where(oky, yy, 0).astype(np.int64)
        for i in range(nx):
            xx = ix + (i - nx // 2)
            ok = oky & (xx >= 0) & (xx < G)
            xi = np.where(ok, xx, 0).astype(np.int64)
            S[:, j, i] = np.where(ok, L[yi, xi], 0).sum(axis=1, dtype=np.int64)
    return S, cs


def best(S):
    """(score, (k, j, i)): the maximum, ties to the smallest flat index."""
    flat = int(np.argmax(S.reshape(-1)))      # np.argmax returns the first maximum
    k, j, i = np.unravel_index(flat, S.shape)
    return int(S[k, j, i]), (int(k), int(j), int(i))


def transform(cs, index, centre, res, nx, ny):
    k, j, i = index
    c, s = cs[k]
    return np.array([[c, -s, float(centre[1]) + (i - nx // 2) * res],
                     [s, c, float(centre[2]) + (j - ny // 2) * res],
                     [0.0, 0.0, 1.0]])


def match(query, ref, centre=(0.0, 0.0, 0.0), **params):
    """(tf, score, (k, j, i), S) of one pair."""
    p = dict(res=0.05, G=512, n_theta=240, d_theta=2 * np.pi / 240, nx=61, ny=61)
    p.update(params)
    S, cs = score_volume(query, ref, centre, **p)
    score, index = best(S)
    return transform(cs, index, centre, p["res"], p["nx"], p["ny"]), score, index, S
