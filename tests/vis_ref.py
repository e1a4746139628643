"""NumPy restatement of the visibility rule of include/slamhip.h
(slam_vis_tables_f64, slam_vis_check_f64): what csrc/vis_kernels.hip must
reproduce bit for bit, and the verdict of slamhip.vis.VisParams.passes.

Every product and sum is a NumPy operation of its own (NumPy never contracts),
np.sqrt is the IEEE square root, and the sector of a point is np.argmax (the
first maximum) over the same host-made table as tests/sig_ref.py::tables.  The
counts are integers, so the comparison with the device is ``np.array_equal``.
tests/test_vis.py pins this file to plain double loops and hand-placed cases."""
import numpy as np

DEFAULTS = dict(sectors=360, window=1, margin=0.15, min_agree=0.25, max_conflict=0.02)


def dirs(S):
    """float64[S][2]: one scalar np.cos / np.sin call per entry."""
    return np.array([[np.cos((k + 0.5) * 2 * np.pi / S), np.sin((k + 0.5) * 2 * np.pi / S)] for k in range(S)])


def sectors(x, y, d):
    """The first maximum of (c_k x) + (s_k y) per point; 0 where a coordinate is
    not finite (no comparison with NaN holds)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    k = np.zeros(len(x), np.int64)
    fin = np.isfinite(x) & np.isfinite(y)
    if fin.any():
        with np.errstate(over="ignore", invalid="ignore"):
            proj = (d[None, :, 0] * x[fin, None]) + (d[None, :, 1] * y[fin, None])
        k[fin] = np.argmax(proj, axis=1)
    return k


def table(points, d):
    """float64[S]: R2 of one scan ((m, 2) rows)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = (x * x) + (y * y)
    keep = np.isfinite(r2)
    out = np.full(len(d), np.inf)
    np.minimum.at(out, sectors(x[keep], y[keep], d), r2[keep])
    return out


def tables_packed(pts, off, d):
    """(float64[n_scans][S], flagged): the tables of packed scans; a scan whose
    offsets descend or leave [0, P] keeps +inf and sets ``flagged``."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(off, dtype=np.int64)
    out = np.full((len(off) - 1, len(d)), np.inf)
    flagged = False
    for s in range(len(off) - 1):
        p0, p1 = int(off[s]), int(off[s + 1])
        if p0 < 0 or p1 < p0 or p1 > len(pts):
            flagged = True
            continue
        out[s] = table(pts[p0:p1], d)
    return out, flagged


def direction(points, M, R2, d, margin, W):
    """(agree, conflict, n) of the points of scan A through the 3x3 ``M``
    against scan B's table ``R2``; also the per-point (agree, conflict) masks."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    S = len(d)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        qx = ((M[0, 0] * x) + (M[0, 1] * y)) + M[0, 2]
        qy = ((M[1, 0] * x) + (M[1, 1] * y)) + M[1, 2]
        rq = np.sqrt((qx * qx) + (qy * qy))
        k = sectors(qx, qy, d)
        idx = (k[:, None] + np.arange(-W, W + 1)[None, :]) % S
        e = R2[idx]                                     # (n, 2W + 1)
        seen = np.isfinite(e)
        re = np.sqrt(e)
        agree = (seen & (np.abs(re - rq[:, None]) <= margin)).any(axis=1)
        conflict = ~agree & seen.all(axis=1) & (rq + margin < re.min(axis=1, initial=np.inf))
    return int(agree.sum()), int(conflict.sum()), len(p), agree, conflict


def inverse(T):
    """The rigid inverse as the kernel takes it: the transposed rotation and
    (-((T00 tx) + (T10 ty)), -((T01 tx) + (T11 ty)))."""
    T = np.asarray(T, dtype=np.float64)
    tx, ty = T[0, 2], T[1, 2]
    return np.array([[T[0, 0], T[1, 0], -((T[0, 0] * tx) + (T[1, 0] * ty))],
                     [T[0, 1], T[1, 1], -((T[0, 1] * tx) + (T[1, 1] * ty))],
                     [0.0, 0.0, 1.0]])


def edge(src_pts, dst_pts, T, d, margin=DEFAULTS["margin"], W=DEFAULTS["window"], R2_src=None, R2_dst=None):
    """The six counts (agree0, conflict0, n0, agree1, conflict1, n1) of the edge
    icp(pc1 = src, pc2 = dst) -> T."""
    R2_src = table(src_pts, d) if R2_src is None else R2_src
    R2_dst = table(dst_pts, d) if R2_dst is None else R2_dst
    T = np.asarray(T, dtype=np.float64).reshape(3, 3)
    a0, c0, n0 = direction(src_pts, T, R2_dst, d, margin, W)[:3]
    a1, c1, n1 = direction(dst_pts, inverse(T), R2_src, d, margin, W)[:3]
    return np.array([a0, c0, n0, a1, c1, n1], np.int64)


def check_packed(pts, off, src, dst, tf, S=DEFAULTS["sectors"], margin=DEFAULTS["margin"], W=DEFAULTS["window"],
                 tables=None):
    """(counts int64[B][6], flagged) of B edges over packed scans; an edge that
    names a scan outside [0, n_scans) or one with bad offsets gets -1."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(off, dtype=np.int64)
    d = dirs(S)
    n_scans = len(off) - 1
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 3, 3)
    if tables is None:
        tables = tables_packed(pts, off, d)[0]
    out = np.full((len(src), 6), -1, np.int64)
    flagged = False

    def bad(s):
        return s < 0 or s >= n_scans or off[s] < 0 or off[s + 1] < off[s] or off[s + 1] > len(pts)

    for b, (s, t) in enumerate(zip(src, dst)):
        s, t = int(s), int(t)
        if bad(s) or bad(t):
            flagged = True
            continue
        out[b] = edge(pts[off[s]:off[s + 1]], pts[off[t]:off[t + 1]], tf[b], d, margin, W, tables[s], tables[t])
    return out, flagged


def shares(counts):
    """(agree (B, 2), conflict (B, 2)): agree_d / n_d and conflict_d / (agree_d
    + conflict_d), 0 where the denominator is not positive."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 6).astype(np.float64)
    a, k, n = c[:, 0::3], c[:, 1::3], c[:, 2::3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, a / n, 0.0), np.where(a + k > 0, k / (a + k), 0.0)


def passes(counts, min_agree=DEFAULTS["min_agree"], max_conflict=DEFAULTS["max_conflict"]):
    """The verdict: both directions have agree_d >= min_agree n_d and conflict_d
    <= max_conflict (agree_d + conflict_d); an edge with an empty scan (or
    flagged, -1) fails."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
    a, k, n = c[:, 0::3], c[:, 1::3], c[:, 2::3]
    ok = (n > 0) & (a >= min_agree * n) & (k <= max_conflict * (a + k))
    return ok.all(axis=1)


def candidate_key(counts, order):
    """The key that orders the candidates of an edge no candidate of which
    passes: (conflict0 + conflict1, -(agree0 + agree1), order); the smallest wins."""
    c = np.asarray(counts, dtype=np.int64).reshape(6)
    return (int(c[1] + c[4]), -int(c[0] + c[3]), int(order))
