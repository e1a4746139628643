"""CPU tests of the pairwise-consistency rule (include/slamhip.h, slam_pcm_*):
the NumPy restatement tests/pcm_ref.py against plain double loops, the bit
layout, the properties of the peel, the host-side argument checks of the entry
points, and the selection the feature is built for on a drifting chain."""
import math

import numpy as np
import pytest

import pcm_ref

TOL = (0.2, 0.1, 0.1, 0.03)   # trans_tol, trans_drift, rot_tol, rot_drift


def plain_mul(A, B):
    return (A[0] * B[0] - A[1] * B[1], A[1] * B[0] + A[0] * B[1],
            (A[0] * B[2] - A[1] * B[3]) + A[2], (A[1] * B[2] + A[0] * B[3]) + A[3])


def plain_inv(A):
    return (A[0], -A[1], -(A[0] * A[2] + A[1] * A[3]), A[1] * A[2] - A[0] * A[3])


def plain_adjacency(X, a, b, Z, tol):
    """The rule of include/slamhip.h, pair by pair, in Python floats: a list of
    L rows of ceil(L / 32) words and the degrees."""
    tt0, ttd, tr0, trd = (float(v) for v in tol)
    X = [tuple(float(v) for v in x) for x in X]
    Z = [tuple(float(v) for v in z) for z in Z]
    L = len(a)
    V = [X[a[l]] for l in range(L)]
    D = [plain_mul(plain_mul(V[l], Z[l]), plain_inv(X[b[l]])) for l in range(L)]
    Di = [plain_inv(d) for d in D]
    U = [plain_mul(plain_inv(V[l]), D[l]) for l in range(L)]
    W = (L + 31) // 32
    words = [[0] * W for _ in range(L)]
    for l in range(L):
        for m in range(l + 1, L):
            E = plain_mul(plain_mul(U[l], Di[m]), V[l])
            n = float(abs(int(a[l]) - int(a[m])) + abs(int(b[l]) - int(b[m])))
            dt = E[2] * E[2] + E[3] * E[3]
            dr = E[1] * E[1] + (1 - E[0]) * (1 - E[0])
            if dt <= tt0 * tt0 + (ttd * ttd) * n and dr <= tr0 * tr0 + (trd * trd) * n:
                words[l][m >> 5] |= 1 << (m & 31)
                words[m][l >> 5] |= 1 << (l & 31)
    return words, [sum(bin(w).count("1") for w in row) for row in words]


def plain_select(words, deg, min_size=2):
    L = len(deg)
    deg = list(deg)
    alive = [True] * L
    order = [-1] * L
    steps = 0
    while True:
        live = [l for l in range(L) if alive[l]]
        if not live:
            break
        low = min(deg[l] for l in live)
        r = max(l for l in live if deg[l] == low)   # the highest index among the lowest degrees
        if low == len(live) - 1:
            break
        alive[r] = False
        order[r] = steps
        for m in live:
            if m != r and (words[r][m >> 5] >> (m & 31)) & 1:
                deg[m] -= 1
        steps += 1
    if sum(alive) < min_size:
        alive = [False] * L
    return order, [int(v) for v in alive], steps


def random_case(L, seed, N=40, noise=0.05):
    """A noisy chain of N poses and L closures: true relative transforms with
    noise, every fourth one wrong, so that both verdicts occur."""
    rng = np.random.default_rng(seed)
    truth = np.cumsum(rng.normal(0, 0.3, size=(N, 3)), axis=0)
    poses = truth + np.cumsum(rng.normal(0, 0.01, size=(N, 3)), axis=0)
    X, T = pcm_ref.elements(poses), pcm_ref.elements(truth)
    a, b = rng.integers(0, N, L), rng.integers(0, N, L)
    Z = pcm_ref.mul(pcm_ref.inv(T[a]), T[b])
    Z[:, 2:] += rng.normal(0, noise, size=(L, 2))
    Z[3::4, 2:] += rng.uniform(-2, 2, size=(len(Z[3::4]), 2))
    return X, a, b, Z


@pytest.mark.parametrize("L", [1, 31, 32, 33, 65])
def test_restatement_against_plain_loops_and_layout(L):
    X, a, b, Z = random_case(L, L)
    adj, deg = pcm_ref.adjacency(X, a, b, Z, TOL)
    words, pdeg = plain_adjacency(X, a, b, Z, TOL)
    assert adj.dtype == np.uint32 and adj.shape == (L, (L + 31) // 32) and deg.dtype == np.int32
    assert adj.tolist() == words and deg.tolist() == pdeg
    full = pcm_ref.unpack(adj, L)
    assert np.array_equal(full, full.T) and not full.diagonal().any()
    assert np.array_equal(pcm_ref.pack(full), adj)
    if L % 32:   # bits past L are zero
        assert not (adj[:, -1] >> np.uint32(L % 32)).any()
    if L >= 31:
        assert 0 < full.sum() < L * (L - 1)   # both verdicts occur
    for min_size in (1, 2, L + 1):
        got = pcm_ref.select(adj, deg, min_size)
        want = plain_select(words, pdeg, min_size)
        assert got[0].tolist() == want[0] and got[1].tolist() == want[1] and got[2] == want[2]
    kept = np.nonzero(pcm_ref.select(adj, deg, 1)[1])[0]
    assert full[np.ix_(kept, kept)].sum() == len(kept) * (len(kept) - 1)   # what is kept is a clique


def _graph(L, pairs):
    full = np.zeros((L, L), dtype=bool)
    for l, m in pairs:
        full[l, m] = full[m, l] = True
    return pcm_ref.pack(full), full.sum(1).astype(np.int32)


def test_peel_properties():
    L = 40
    adj, deg = _graph(L, [(l, m) for l in range(L) for m in range(l)])
    order, keep, steps = pcm_ref.select(adj, deg)
    assert steps == 0 and keep.all() and (order == -1).all()       # all consistent: nothing to do
    adj, deg = _graph(L, [])
    order, keep, steps = pcm_ref.select(adj, deg, min_size=1)      # nothing consistent: index 0 is left
    assert steps == L - 1 and keep.tolist() == [1] + [0] * (L - 1)
    assert order.tolist() == [-1] + list(range(L - 2, -1, -1))
    order, keep, steps = pcm_ref.select(adj, deg, min_size=2)
    assert steps == L - 1 and not keep.any() and order[0] == -1
    # a path 0 - 1 - 2 - 3 - 4: at every step the end of the path ties at degree 1 with closure 0 and the higher
    # index goes: 4, 3, 2, and {0, 1} is left.  The lowest-index rule would remove 0, 1, 2 and leave {3, 4}.
    adj, deg = _graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    order, keep, steps = pcm_ref.select(adj, deg)
    assert order.tolist() == [-1, -1, 2, 1, 0] and keep.tolist() == [1, 1, 0, 0, 0] and steps == 3


def test_nan_closure_is_peeled():
    X, a, b, Z = random_case(33, 7, noise=0.0)
    a[:] = a[0]
    b[:] = b[0]
    Z[:] = Z[0]                         # 33 copies of one closure: a clique
    Z[17, 2] = np.nan
    adj, deg = pcm_ref.adjacency(X, a, b, Z, TOL)
    assert deg[17] == 0 and (np.delete(deg, 17) == 31).all()
    order, keep, steps = pcm_ref.select(adj, deg)
    assert steps == 1 and order[17] == 0 and not keep[17] and keep.sum() == 32
    words, pdeg = plain_adjacency(X, a, b, Z, TOL)
    assert adj.tolist() == words


def drifting_case(seed):
    """160 chain poses with drift (``lap_graph_c4``'s dead reckoning), its 60
    true loop edges with 2 cm of noise and about 20 random outliers, shuffled:
    ``(poses, a, b, Z (L, 3, 3), inlier bool[L])``."""
    from slamhip import se2, synthetic
    guess, ea, eb, tf, _ = synthetic.lap_graph_c4(seed, poses_per_side=10, num_loops=4, n_loops=60)
    N = len(guess)
    a, b, Z = ea[N - 1:].copy(), eb[N - 1:].copy(), tf[N - 1:].copy()
    assert N == 160 and len(a) == 60
    rng = np.random.default_rng(100 + seed)
    Z[:, :2, 2] += rng.normal(0, 0.02, (60, 2))
    oa, ob = rng.integers(0, N, 20), rng.integers(0, N, 20)
    far = np.abs(oa - ob) > 1
    th = rng.uniform(-np.pi, np.pi, 20)
    x = rng.uniform(-1.5, 1.5, 20)
    y = rng.uniform(-1.5, 1.5, 20)
    oZ = np.stack([se2.pose_to_mat((x[k], y[k], th[k])) for k in range(20)])
    a, b, Z = np.r_[a, oa[far]], np.r_[b, ob[far]], np.concatenate([Z, oZ[far]])
    inlier = np.r_[np.ones(60, bool), np.zeros(int(far.sum()), bool)]
    p = rng.permutation(len(a))
    return guess, a[p], b[p], Z[p], inlier[p]


@pytest.mark.parametrize("seed", [0, 2])
def test_selection_on_a_drifting_chain(seed):
    """Every outlier is rejected and at least 57 of the 60 inliers are kept."""
    poses, a, b, Z, inlier = drifting_case(seed)
    keep, deg, order, steps, _ = pcm_ref.consistency(poses, a, b, Z, TOL)
    print(f"seed {seed}: kept {int(keep[inlier].sum())} of {int(inlier.sum())} inliers, "
          f"{int(keep[~inlier].sum())} of {int((~inlier).sum())} outliers, {steps} steps")
    assert (~inlier).sum() >= 15
    assert not keep[~inlier].any()
    assert keep[inlier].sum() >= 57


def test_host_only_argument_checks():
    """The entry points validate before any launch: no GPU needed."""
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 106
    assert lib.slam_pcm_work_size(0) == 0 and lib.slam_pcm_work_size(1) >= 96
    assert lib.slam_pcm_work_size(65536) >= 96 * 65536
    assert lib.slam_pcm_work_size(-1) == -1 and lib.slam_pcm_work_size(65537) == -3
    assert b"65536" in lib.slam_last_error()
    one = 8   # a non-null, aligned address that is never dereferenced: every call below fails before a launch

    def adjacency(X=one, N=4, a=one, b=one, Z=one, L=3, tol=(0.1, 0.1, 0.1, 0.1), adj=one, deg=one, work=one):
        return lib.slam_pcm_adjacency_f64(X, N, a, b, Z, L, *tol, adj, deg, work, None)
    for kw in (dict(X=None), dict(a=None), dict(b=None), dict(Z=None), dict(adj=None), dict(deg=None),
               dict(work=None), dict(N=0), dict(L=-1), dict(tol=(-0.1, 0.1, 0.1, 0.1)), dict(tol=(0.1, -1.0, 0.1, 0.1)),
               dict(tol=(0.1, 0.1, -0.1, 0.1)), dict(tol=(0.1, 0.1, 0.1, -0.1)), dict(tol=(math.nan, 0.1, 0.1, 0.1)),
               dict(work=4)):
        assert adjacency(**kw) == -1, kw
        assert lib.slam_last_error() != b""
    assert adjacency(L=65537) == -3
    assert adjacency(L=0) == 0 and lib.slam_last_error() == b""

    def select(adj=one, deg=one, L=3, min_size=2, order=one, keep=one, steps=one):
        return lib.slam_pcm_select(adj, deg, L, min_size, order, keep, steps, None)
    for kw in (dict(adj=None), dict(deg=None), dict(order=None), dict(keep=None), dict(steps=None), dict(L=-1),
               dict(min_size=-1)):
        assert select(**kw) == -1, kw
    assert select(L=65537) == -3
    assert select(L=0) == 0
    assert lib.slam_pcm_set_peel_slots(3) == -1 and lib.slam_pcm_set_peel_slots(128) == -1
    assert lib.slam_pcm_set_peel_slots(16) == 0 and lib.slam_pcm_set_peel_slots(0) == 0
