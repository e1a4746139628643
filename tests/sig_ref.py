"""NumPy restatement of the scan-signature rule of include/slamhip.h
(slam_sig_build, slam_sig_match): what csrc/sig_kernels.hip must reproduce bit
for bit.

A scan's signature is S uint32 masks (sector s, bit = ring) of the cells its
points fall into: ring from r2 = x*x + y*y against the squared ring edges,
sector the first maximum of c_s*x + s_s*y.  d(i, j, k) = sum_s popcount(sig_i[s]
^ sig_j[(s + k) % S]); d_ij the minimum over k, k_ij the first k attaining it; j
is a candidate of row i iff d_ij * den <= num * (n_i + n_j); a row's K best
candidates are ordered by (d_ij, j).

``distances`` takes the circular correlation through an FFT over the sectors
(sums of at most 4,096 products of bits: the rounded result is exact);
tests/test_sig.py pins it, and ``signature``, to plain double loops."""
import numpy as np

RINGS = 32


def tables(S, r_min=0.0, dr=0.4):
    """``(dirs float64[S][2], edges2 float64[33])`` as the caller of
    slam_sig_build makes them: one scalar np.cos / np.sin call per entry."""
    dirs = np.array([[np.cos((s + 0.5) * 2 * np.pi / S), np.sin((s + 0.5) * 2 * np.pi / S)] for s in range(S)])
    edges2 = np.array([(r_min + k * dr) ** 2 for k in range(RINGS + 1)])
    return dirs, edges2


def signature(points, dirs, edges2):
    """``(sig uint32[S], ring uint8[32], n)`` of one scan ((m, 2) rows)."""
    S = len(dirs)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    r2 = x * x + y * y
    r = np.searchsorted(edges2, r2, side="right") - 1   # NaN sorts past every edge
    keep = (r >= 0) & (r < RINGS)
    x, y, r = x[keep], y[keep], r[keep]
    proj = dirs[None, :, 0] * x[:, None] + dirs[None, :, 1] * y[:, None]
    s = np.argmax(proj, axis=1) if len(x) else np.zeros(0, np.int64)   # the first maximum
    sig = np.zeros(S, np.uint32)
    np.bitwise_or.at(sig, s, (np.uint32(1) << r.astype(np.uint32)))
    bits = (sig[:, None] >> np.arange(RINGS, dtype=np.uint32)[None, :]) & np.uint32(1)
    ring = bits.sum(0).astype(np.uint8)
    return sig, ring, int(ring.sum())


def signatures(scans, dirs, edges2):
    """``(sig uint32[N][S], ring uint8[N][32], n int32[N])``."""
    out = [signature(s, dirs, edges2) for s in scans]
    S = len(dirs)
    return (np.array([o[0] for o in out], np.uint32).reshape(len(out), S),
            np.array([o[1] for o in out], np.uint8).reshape(len(out), RINGS),
            np.array([o[2] for o in out], np.int32))


def ring_counts(sig):
    """``(ring uint8[N][32], n int32[N])`` of finished masks."""
    sig = np.asarray(sig, np.uint32)
    bits = (sig[:, :, None] >> np.arange(RINGS, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    ring = bits.sum(1)
    return ring.astype(np.uint8), ring.sum(1).astype(np.int32)


def distances(sig, rows=None, block=None, col0=0):
    """``(d int64[len(rows)][N - col0], k int64[len(rows)][N - col0])``: d_ij
    and k_ij of the given rows (all rows by default) against the scans from
    ``col0`` on."""
    sig = np.asarray(sig, np.uint32)
    N, S = sig.shape
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    bits = ((sig[:, None, :] >> np.arange(RINGS, dtype=np.uint32)[None, :, None]) & np.uint32(1)).astype(np.float64)
    n = bits.sum((1, 2)).astype(np.int64)
    F = np.ascontiguousarray(np.fft.rfft(bits, axis=2).transpose(2, 0, 1))   # (S / 2 + 1, N, 32)
    Fc = np.ascontiguousarray(F[:, col0:, :].transpose(0, 2, 1))             # (S / 2 + 1, 32, N - col0)
    nc = N - col0
    block = block if block is not None else max(1, int(4e6 // (max(nc, 1) * len(F))))
    d = np.empty((len(rows), nc), np.int64)
    k = np.empty((len(rows), nc), np.int64)
    for b0 in range(0, len(rows), block):
        rb = rows[b0:b0 + block]
        # corr[k, i, j] = sum_s,r B_i[s][r] B_j[(s + k) % S][r]: the transform over k of conj(F_i) . F_j
        corr = np.fft.irfft(np.matmul(np.conj(F[:, rb, :]), Fc), n=S, axis=0)
        np.rint(corr, out=corr)
        kk = np.argmax(corr, axis=0)   # the first maximum of corr is the first minimum of d
        k[b0:b0 + block] = kk
        best = np.take_along_axis(corr, kk[None], axis=0)[0].astype(np.int64)
        d[b0:b0 + block] = n[rb][:, None] + n[None, col0:] - 2 * best
    return d, k


def lower_bound(ring, rows=None):
    """``LB int64[len(rows)][N]``: sum_r |ring_i[r] - ring_j[r]|."""
    ring = np.asarray(ring, np.int64)
    rows = np.arange(len(ring)) if rows is None else np.asarray(rows, dtype=np.int64)
    return np.abs(ring[rows][:, None, :] - ring[None, :, :]).sum(2)


def match(sig, start, n_rows, num=1, den=4, K=1, rows=None):
    """``(j, d, k int64[len(rows)][K], count int64[len(rows)])`` of
    slam_sig_match for the given rows (default: all ``n_rows``)."""
    sig = np.asarray(sig, np.uint32)
    N = len(sig)
    rows = np.arange(n_rows) if rows is None else np.asarray(rows, dtype=np.int64)
    n = ring_counts(sig)[1].astype(np.int64)
    out_j = np.full((len(rows), K), -1, np.int64)
    out_d = np.full((len(rows), K), -1, np.int64)
    out_k = np.full((len(rows), K), -1, np.int64)
    count = np.zeros(len(rows), np.int64)
    if len(rows) == 0:
        return out_j, out_d, out_k, count
    start = np.asarray(start, dtype=np.int64)
    col0 = int(min(start[rows].min(), N))   # no row looks left of it
    if col0 == N:
        return out_j, out_d, out_k, count
    D, Kk = distances(sig, rows, col0=col0)
    cols = np.arange(col0, N)
    for a, i in enumerate(rows):
        cand = (cols >= start[i]) & (D[a] * den <= num * (n[i] + n[col0:]))
        js = cols[cand]
        count[a] = len(js)
        order = np.lexsort((js, D[a][js - col0]))[:K]   # by (d, j)
        js = js[order]
        out_j[a, :len(js)] = js
        out_d[a, :len(js)] = D[a][js - col0]
        out_k[a, :len(js)] = Kk[a][js - col0]
    return out_j, out_d, out_k, count


def candidates(sig, start, n_rows, num=1, den=4):
    """The (i, j, k) of every row's best candidate, in the order the greedy
    pass visits them (the last row first)."""
    j, _, k, _ = match(sig, start, n_rows, num, den, 1)
    out = [(int(i), int(j[i, 0]), int(k[i, 0])) for i in range(n_rows) if j[i, 0] >= 0]
    out.reverse()
    return out
