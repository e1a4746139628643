"""NumPy restatement of the descriptor-matching rule of include/slamhip.h
(slam_desc_match_batch): what csrc/desc_kernels.hip must reproduce bit for bit.

A descriptor is 32 bytes.  ``hamming``: d = popcount(A[a] xor B[b]), forward
and backward first-index nearest neighbours, cross-checked.  ``l2``: d = the
integer sum of squared byte differences, forward only.  Matches ordered by
(d, a); the score is the left-to-right float64 sum of the first ``n_matches``
distances (d, or the float32 square root of d), +inf when there are fewer."""
import numpy as np

METRICS = ("hamming", "l2")


def _rows(x):
    x = np.zeros((0, 32), np.uint8) if x is None else np.asarray(x)
    return x.reshape(-1, 32).astype(np.uint8)


def distance_matrix(A, B, metric):
    """int64 (len(A), len(B)).  Both metrics as |a|^2 + |b|^2 - 2 a.b over
    float64 (bits for hamming, bytes for l2): every product and partial sum is
    an integer below 2^53, so the BLAS product is exact in any order."""
    A, B = _rows(A), _rows(B)
    if metric == "hamming":
        a, b = np.unpackbits(A, axis=1).astype(np.float64), np.unpackbits(B, axis=1).astype(np.float64)
    elif metric == "l2":
        a, b = A.astype(np.float64), B.astype(np.float64)
    else:
        raise ValueError(metric)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    return d.astype(np.int64)


def matches(A, B, metric):
    """int64 (count, 3) rows (a, b, d), ordered by (d, a)."""
    A, B = _rows(A), _rows(B)
    if len(A) == 0 or len(B) == 0:
        return np.zeros((0, 3), np.int64)
    D = distance_matrix(A, B, metric)
    a = np.arange(len(A))
    fwd = D.argmin(axis=1)            # the first minimum
    if metric == "hamming":
        bwd = D.argmin(axis=0)
        a = a[bwd[fwd] == a]
    b = fwd[a]
    d = D[a, b]
    order = np.lexsort((a, d))
    return np.stack([a[order], b[order], d[order]], axis=1)


def score(rows, n_matches, metric):
    """(score, count, first n_matches rows or -1s)."""
    count = len(rows)
    if count < n_matches:
        return np.inf, count, np.full((n_matches, 3), -1, np.int64)
    best = rows[:n_matches]
    total = 0.0
    for d in best[:, 2]:
        total += float(d) if metric == "hamming" else float(np.sqrt(np.float32(d)))
    return total, count, best


def match_pairs(descs, qi, ti, n_matches, metric):
    """score float64[B], count int64[B], matches int64[B][n_matches][3]."""
    B = len(qi)
    s, c, m = np.zeros(B), np.zeros(B, np.int64), np.zeros((B, n_matches, 3), np.int64)
    for k, (i, j) in enumerate(zip(qi, ti)):
        s[k], c[k], m[k] = score(matches(descs[i], descs[j], metric), n_matches, metric)
    return s, c, m


def similarity_matrix(descs, start, n_matches, metric):
    """The reference's dist_mat (src/loop_closure_detection.py:103-110)."""
    M = len(descs)
    out = np.full((M, M), np.inf)
    for i in range(M):
        for j in range(int(start[i]), M):
            out[i, j] = score(matches(descs[i], descs[j], metric), n_matches, metric)[0]
    return out
