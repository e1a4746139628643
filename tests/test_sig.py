"""CPU tests of the scan-signature rule (include/slamhip.h, slam_sig_*): the
NumPy restatement tests/sig_ref.py against plain double loops, the properties
the kernels rely on (the ring-count bound, the shift of a rolled signature) and
the recall the detector is built for."""
import numpy as np
import pytest

import sig_ref


def plain_signature(points, dirs, edges2):
    """The rule of include/slamhip.h, point by point, in Python floats."""
    S = len(dirs)
    sig = [0] * S
    for x, y in points:
        x, y = float(x), float(y)
        r2 = x * x + y * y
        ring = [r for r in range(32) if float(edges2[r]) <= r2 < float(edges2[r + 1])]
        if not ring:
            continue
        best, best_s = None, 0
        for s in range(S):
            v = float(dirs[s][0]) * x + float(dirs[s][1]) * y
            if best is None or v > best:
                best, best_s = v, s
        sig[best_s] |= 1 << ring[0]
    ring = [sum((m >> r) & 1 for m in sig) for r in range(32)]
    return np.array(sig, np.uint32), np.array(ring, np.uint8), sum(ring)


def plain_distance(a, b):
    """(d, k): the minimum over k of sum_s popcount(a[s] ^ b[(s + k) % S]) and the first k attaining it."""
    S = len(a)
    ds = [sum(bin(int(a[s]) ^ int(b[(s + k) % S])).count("1") for s in range(S)) for k in range(S)]
    return min(ds), ds.index(min(ds))


def edge_case_points(edges2):
    """Ring edges hit exactly (r2 == edges2[k] for points on an axis), the
    origin, points past the last ring and just inside it, a NaN."""
    on_edges = [(float(np.sqrt(e)), 0.0) for e in edges2[::3]] + [(0.0, -float(np.sqrt(e))) for e in edges2[1::5]]
    return np.array(on_edges + [(0.0, 0.0), (-0.0, 0.0), (13.0, 0.1), (-9.1, 9.1), (12.79, 0.0), (3.0, 4.0),
                                (np.nan, 1.0), (1e-200, 0.0)])


def tie_tables(S):
    """Sector tables with duplicate entries: sectors 2 m and 2 m + 1 share a
    direction, so every point ties between two sectors and the smaller wins."""
    dirs, edges2 = sig_ref.tables(S)
    dirs[1::2] = dirs[0::2]
    return dirs, edges2


@pytest.mark.parametrize("S", [8, 24, 64, 128])
def test_signature_against_plain_loop(S):
    rng = np.random.default_rng(S)
    dirs, edges2 = sig_ref.tables(S)
    clouds = [edge_case_points(edges2), rng.uniform(-14, 14, size=(300, 2)), np.zeros((1, 2)),
              rng.uniform(20, 30, size=(5, 2))]
    for tab in ((dirs, edges2), tie_tables(S), sig_ref.tables(S, r_min=0.5, dr=0.25)):
        for pts in clouds:
            got, want = sig_ref.signature(pts, *tab), plain_signature(pts, *tab)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    # what the cases are there for
    sig, ring, n = sig_ref.signature(edge_case_points(edges2), dirs, edges2)
    assert sig[0] & 1 and n > 8                                     # the origin: ring 0, sector 0 of an all-way tie
    assert sig_ref.signature(clouds[3], dirs, edges2)[2] == 0       # past the last ring: empty
    assert not sig_ref.signature(clouds[1], *tie_tables(S))[0][1::2].any()   # ties go to the smaller sector
    exact = np.array([[float(np.sqrt(edges2[3])), 0.0]])            # r2 == edges2[3] exactly: ring 3, not 2
    assert float(exact[0, 0]) ** 2 == edges2[3] and sig_ref.signature(exact, dirs, edges2)[1][3] == 1


@pytest.mark.parametrize("S", [8, 24, 64, 72, 128])
def test_distances_against_plain_loop_and_bound(S):
    rng = np.random.default_rng(100 + S)
    dens = rng.uniform(0.05, 0.95, size=14)
    sig = np.array([[sum(1 << r for r in range(32) if rng.random() < p) for _ in range(S)] for p in dens], np.uint32)
    sig[3] = 0
    sig[5] = np.roll(sig[4], 3)
    d, k = sig_ref.distances(sig)
    ring, n = sig_ref.ring_counts(sig)
    lb = sig_ref.lower_bound(ring)
    for i in range(len(sig)):
        assert n[i] == sum(bin(int(m)).count("1") for m in sig[i])
        for j in range(len(sig)):
            assert (d[i, j], k[i, j]) == plain_distance(sig[i], sig[j])
    assert (lb <= d).all() and (lb < d).any() and (lb[np.arange(14), np.arange(14)] == 0).all()
    assert d[4, 5] == 0 and k[4, 5] == 3
    rows = np.array([5, 0, 13])
    d2, k2 = sig_ref.distances(sig, rows, block=2)
    assert np.array_equal(d2, d[rows]) and np.array_equal(k2, k[rows])


def test_rolled_signature_gives_its_shift():
    rng = np.random.default_rng(5)
    for S in (8, 64, 128):
        a = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)
        for k in (0, 1, S // 2, S - 1):
            b = np.roll(a, k)   # b[(s + k) % S] == a[s]
            d, kk = sig_ref.distances(np.stack([a, b]))
            assert d[0, 1] == 0 and kk[0, 1] == k
            assert d[1, 0] == 0 and kk[1, 0] == (S - k) % S


def test_match_orders_by_d_then_j_and_counts():
    rng = np.random.default_rng(9)
    base = rng.integers(0, 1 << 32, size=16, dtype=np.uint64).astype(np.uint32)
    sig = np.stack([base, np.roll(base, 2), base ^ np.uint32(1), base, ~base, np.roll(base ^ np.uint32(1), 5)])
    j, d, k, count = sig_ref.match(sig, np.zeros(6, np.int64), 2, 1, 4, 4)
    assert j[0].tolist() == [0, 1, 3, 2] and d[0].tolist() == [0, 0, 0, 16] and k[0].tolist() == [0, 2, 0, 0]
    assert count.tolist() == [5, 5]   # all but the complement
    j, d, k, count = sig_ref.match(sig, np.array([4, 6]), 2, 0, 1, 3)
    assert j.tolist() == [[-1, -1, -1], [-1, -1, -1]] and count.tolist() == [0, 0]
    assert sig_ref.candidates(sig, np.array([1, 2, 3, 6, 6, 6]), 3, 1, 4) == [(2, 5, 5), (1, 3, 14), (0, 1, 2)]


def turned(scans, angles):
    """Every scan in a frame turned by its angle."""
    out = []
    for s, a in zip(scans, angles):
        c, sn = np.cos(a), np.sin(a)
        out.append(np.stack([c * s[:, 0] + sn * s[:, 1], -sn * s[:, 0] + c * s[:, 1]], axis=1))
    return out


@pytest.mark.parametrize("n_scans, seed, n_beams", [(1200, 7, 1081), (2000, 3, 361)])
def test_recall_on_turned_loop_sequences(n_scans, seed, n_beams):
    """Every scan's frame turned at random; 64 sectors, 32 rings of 0.4 m, the
    last 5 m of path excluded, threshold 1/4.  Of the rows with a true revisit
    within 0.1 m at most 1 % may lack a best candidate whose true pose lies
    within 0.5 m."""
    from slamhip import lcd, synthetic
    seq = synthetic.make_loop_sequence(n_scans, seed=seed, n_beams=n_beams)
    scans = turned(seq.scans, np.random.default_rng(1).uniform(-np.pi, np.pi, n_scans))
    sig = sig_ref.signatures(scans, *sig_ref.tables(64))[0]
    start, n_rows = lcd.path_starts(seq.truth, 5)
    j = sig_ref.match(sig, start, n_rows, 1, 4, 1)[0][:, 0]
    xy = seq.truth[:, :2]
    dist = np.sqrt(((xy[:n_rows, None, :] - xy[None, :, :]) ** 2).sum(2))
    later = np.arange(n_scans)[None, :] >= start[:n_rows, None]
    revisit = (later & (dist <= 0.1)).any(1)
    found = (j >= 0) & (dist[np.arange(n_rows), np.maximum(j, 0)] <= 0.5)
    missed = int((revisit & ~found).sum())
    print(f"rows with a revisit {int(revisit.sum())}, of them found {int((revisit & found).sum())}")
    assert revisit.sum() > 500
    assert missed <= 0.01 * revisit.sum(), (missed, int(revisit.sum()))
