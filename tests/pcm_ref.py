"""NumPy restatement of the pairwise-consistency rule of include/slamhip.h
(slam_pcm_adjacency_f64, slam_pcm_select): what csrc/pcm_kernels.hip must
reproduce bit for bit.

An SE(2) element is (c, s, x, y), here the last axis of an array.  ``mul`` and
``inv`` round every operation individually, as NumPy's elementwise arithmetic
does.  Closure l = (a, b, Z) measures X_b = X_a Z; two closures are consistent
when the cycle through both and the chain closes to within ``tol^2 + drift^2 n``
in translation and in the squared chord of the rotation, n the chain length the
cycle spans.  ``select`` is the min-degree peel (ties: the highest index).
tests/test_pcm.py pins both to plain Python double loops."""
import numpy as np


def mul(A, B):
    Ac, As, Ax, Ay = (A[..., k] for k in range(4))
    Bc, Bs, Bx, By = (B[..., k] for k in range(4))
    return np.stack([Ac * Bc - As * Bs, As * Bc + Ac * Bs, (Ac * Bx - As * By) + Ax, (As * Bx + Ac * By) + Ay], axis=-1)


def inv(A):
    Ac, As, Ax, Ay = (A[..., k] for k in range(4))
    return np.stack([Ac, -As, -(Ac * Ax + As * Ay), As * Ax - Ac * Ay], axis=-1)


def elements(poses):
    """float64[N][4] of (N, 3) poses (x, y, theta): one scalar np.cos / np.sin
    call per pose, as ``slamhip.se2.pose_to_mat`` makes them."""
    return np.array([[np.cos(p[2]), np.sin(p[2]), p[0], p[1]] for p in np.asarray(poses, dtype=np.float64)]
                    ).reshape(-1, 4)


def from_mats(T):
    """float64[L][4] of (L, 3, 3) SE(2) matrices."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 3, 3)
    return np.stack([T[:, 0, 0], T[:, 1, 0], T[:, 0, 2], T[:, 1, 2]], axis=-1)


def prepare(X, a, b, Z):
    """(V, U, Di), float64[L][4] each."""
    V = X[a]
    D = mul(mul(V, Z), inv(X[b]))
    return V, mul(inv(V), D), inv(D)


def pair_terms(X, a, b, Z, rows=None):
    """(dt, dr, n) float64[R][L] of E = mul(mul(U_l, Di_m), V_l) for the rows l
    (all by default) against every m: valid for the rule where l < m."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    V, U, Di = prepare(X, a, b, Z)
    rows = np.arange(len(a)) if rows is None else np.asarray(rows)
    E = mul(mul(U[rows, None, :], Di[None, :, :]), V[rows, None, :])
    n = (np.abs(a[rows, None] - a[None, :]) + np.abs(b[rows, None] - b[None, :])).astype(np.float64)
    dt = E[..., 2] * E[..., 2] + E[..., 3] * E[..., 3]
    dr = E[..., 1] * E[..., 1] + (1 - E[..., 0]) * (1 - E[..., 0])
    return dt, dr, n


def consistent(X, a, b, Z, tol, block=512):
    """bool[L][L]: symmetric, the diagonal clear.  ``tol`` = (trans_tol,
    trans_drift, rot_tol, rot_drift)."""
    tt0, ttd, tr0, trd = (np.float64(v) for v in tol)
    L = len(a)
    upper = np.zeros((L, L), dtype=bool)
    with np.errstate(invalid="ignore"):
        for r0 in range(0, L, block):
            rows = np.arange(r0, min(L, r0 + block))
            dt, dr, n = pair_terms(X, a, b, Z, rows)
            ok = (dt <= tt0 * tt0 + (ttd * ttd) * n) & (dr <= tr0 * tr0 + (trd * trd) * n)
            upper[rows] = ok & (np.arange(L)[None, :] > rows[:, None])
    return upper | upper.T


def pack(adj):
    """uint32[L][ceil(L / 32)]: bit m of row l is bit m & 31 of word m >> 5."""
    L = len(adj)
    W = (L + 31) // 32
    bits = np.zeros((L, W * 32), dtype=np.uint64)
    bits[:, :L] = adj
    return (bits.reshape(L, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def unpack(words, L):
    words = np.asarray(words, dtype=np.uint32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(len(words), -1)[:, :L] \
        .astype(bool)


def adjacency(X, a, b, Z, tol):
    """``(adj uint32[L][W], deg int32[L])``."""
    adj = consistent(X, a, b, Z, tol)
    return pack(adj), adj.sum(1).astype(np.int32)


def select(adj, deg, min_size=2):
    """``(order int32[L], keep uint8[L], steps)`` of packed rows and their
    popcounts."""
    L = len(deg)
    nb = unpack(adj, L)
    deg = np.array(deg, dtype=np.int64)
    alive = np.ones(L, dtype=bool)
    order = np.full(L, -1, np.int32)
    idx = np.arange(L)
    steps = 0
    while alive.sum() > 1:
        low = deg[alive].min()
        r = idx[alive & (deg == low)].max()
        if low == alive.sum() - 1:
            break
        alive[r] = False
        order[r] = steps
        deg[nb[r] & alive] -= 1
        steps += 1
    keep = alive if alive.sum() >= min_size else np.zeros(L, dtype=bool)
    return order, keep.astype(np.uint8), steps


def consistency(poses, a, b, Zmats, tol, min_size=2):
    """``(keep bool[L], deg, order, steps, adj words)`` of (N, 3) poses and
    (L, 3, 3) relative transforms: the whole of ``slamhip.pcm.consistency``."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) == 0:
        return np.zeros(0, bool), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.zeros((0, 0), np.uint32)
    adj, deg = adjacency(elements(poses), a, b, from_mats(Zmats), tol)
    order, keep, steps = select(adj, deg, min_size)
    return keep.astype(bool), deg, order, steps, adj
