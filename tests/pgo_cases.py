"""Test graphs for the SGD relaxation's kernel paths and block edges (no GPU).

The relaxation (csrc/pgo_kernels.hip, sgd_relax_kernel) groups nodes in blocks
of ``bs = 2^shift`` and treats an edge (a, b) differently by where a and b sit
in their blocks, so the graphs here place edges by hand on those positions
instead of drawing them at random:

* ``lap_graph``  poses on a circle plus one transform per listed pair, each
  perturbed so that no residual is near zero (the heading residual's wrap
  point ``x % 2 pi`` at x ~ 0 is ill-conditioned: the last bit of sincos /
  atan2 decides between 0 and 2 pi there, and no test can pin it);
* ``structural`` / ``islands`` / ``dense``  edge lists (ORDER MATTERS: the
  relaxation is sequential);
* ``residual_margin``  a restatement of ``pgo_oracle.sgd_step`` that also
  reports how far every applied heading residual stays from that wrap point
  and how many components the clamp |beta| > |r| cut;
* ``case`` / ``dense_case``  the graphs the tests use, with their oracle
  results, built once per process and read-only;
* ``orient_case`` / ``orient_tf_case``  inputs of the orientation kernels.

tests/test_pgo_cases.py checks these inputs on the CPU (margin, relations,
restatement == oracle); tests/test_pgo_paths_gpu.py runs them on the GPU.
"""
import functools

import numpy as np

import pgo_oracle as po

TWO_PI = 2 * np.pi
LRS = (1.0, 0.02)
SIGMA = 0.1

# N of the automatic-dispatch cases: tiny graphs, one block +- one node, and
# both sides of every dispatch boundary (BR 1 -> 2, LDS -> global, sh 6 -> 7,
# sh 8, sh 9 with its overflow loop).
AUTO_STRUCTURAL = (3, 4, 63, 64, 65, 128, 129, 4096, 4097, 6144, 6145, 131072, 131073, 262145, 524289)
AUTO_ISLANDS = (200, 4097, 6145, 131073)
# (path, forced shift or -1, N): every path that can hold the graph
FORCED = ((0, -1, 200), (1, -1, 4200), (2, 6, 200), (2, 7, 200), (2, 6, 4200), (2, 7, 4200), (2, 9, 2200),
          (2, 10, 2200))
DENSE_E = (63, 64, 65, 1023, 1024, 1025, 2049)
DENSE_N = 300
# (in_lds, rounds, shift) each automatic case is meant to run on
AUTO_PLAN = {3: (True, 1, 6), 4: (True, 1, 6), 63: (True, 1, 6), 64: (True, 1, 6), 65: (True, 1, 6),
             128: (True, 1, 6), 129: (True, 1, 6), 200: (True, 1, 6), 4096: (True, 1, 6), 4097: (True, 2, 6),
             6144: (True, 2, 6), 6145: (False, 1, 6), 131072: (False, 1, 6), 131073: (False, 1, 7),
             262145: (False, 1, 8), 524289: (False, 1, 9)}
# N -> the plan fields that differ between N and N + 1; the plan changes nowhere else up to 524,290
PLAN_BOUNDARIES = {4096: {"rounds"}, 6144: {"in_lds", "rounds", "threads"}, 131072: {"shift"}, 262144: {"shift"},
                   524288: {"shift"}}

# Seeds: constants, the smallest for which the wrap margin of both steps is
# >= 1e-3 (ten times what test_pgo_cases.py asserts for every case).  Seed 0
# does for every graph but the 2,049-edge dense one.
MARGIN = 1e-4
SEEDS = {}                  # (kind, N, shift) -> seed, default 0
DENSE_SEEDS = {2049: 1}     # E -> seed, default 0


def _pose_mat(p):
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0.0, 0.0, 1.0]])


def lap_graph(N, pairs, seed):
    """(poses, ea, eb, tf): node i on a circle of radius 2 m with 256 nodes per
    lap, heading wrap(phi_i + pi / 2), noise N(0, 0.01 m) / N(0, 0.02 rad); the
    transform of pair (a, b) is the exact relative transform of those poses
    with its translation perturbed by N(0, 0.05 m) and its rotation by a
    uniform draw from [0.3, 1.2] rad (mutually inconsistent edges)."""
    rng = np.random.default_rng(seed)
    phi = TWO_PI * np.arange(N) / 256.0
    poses = np.stack([2.0 * np.cos(phi), 2.0 * np.sin(phi), po.wrap(phi + np.pi / 2)], axis=1)
    poses[:, :2] += rng.normal(0.0, 0.01, (N, 2))
    poses[:, 2] += rng.normal(0.0, 0.02, N)
    ea = np.array([a for a, _ in pairs], dtype=np.int32)
    eb = np.array([b for _, b in pairs], dtype=np.int32)
    tf = np.zeros((len(pairs), 3, 3))
    for k, (a, b) in enumerate(pairs):
        rel = np.linalg.inv(_pose_mat(poses[a])) @ _pose_mat(poses[b])
        t = rel[:2, 2] + rng.normal(0.0, 0.05, 2)
        th = np.arctan2(rel[1, 0], rel[0, 0]) + rng.uniform(0.3, 1.2)
        tf[k] = _pose_mat([t[0], t[1], th])
    return poses, ea, eb, tf


def _fit(pairs, N, hi=None):
    """Pairs inside [0, hi] (default N - 1), a != b, first occurrence only."""
    hi = N - 1 if hi is None else hi
    out = []
    for a, b in pairs:
        if 0 <= a <= hi and 0 <= b <= hi and a != b and (a, b) not in out:
            out.append((int(a), int(b)))
    return out


def structural(N, bs):
    """Edges on the positions node_of() and the whole-block loops distinguish."""
    last = ((N - 1) // bs) * bs     # first node of the last block
    return _fit([
        (0, N - 1),                 # a = 0, b = N - 1: every block between them ramps
        (0, 2),                     # one block; every other block is tail
        (N - 3, N - 1),             # inside the (partial) last block
        (3, bs - 1),                # b on the last node of a's block
        (bs - 1, bs + 1),           # a on a block's last node (no remainder of a's block), adjacent blocks
        (bs - 2, bs),               # adjacent blocks, b on a block's first node
        (bs, 2 * bs),               # a on a block's first node: bs - 1 + bs explicit nodes
        (bs - 1, 2 * bs - 1),       # a and b both on last nodes
        (5, N - 6),
        (last - 3, N - 1),          # from the block before into the partial last block
        (N - 1, 4), (2 * bs, 7),    # reversed: skipped by the compaction, still in pass 1's gamma scan
        (10, 11),                   # odometry-shaped: never a loop edge
        (7, 9), (7, 40), (7, (N - 1) // 2),       # consecutive edges out of node 7 (cached sincos)
        (N // 5, 4 * N // 5), (2 * N // 5, 3 * N // 5),       # nested
        (N // 6, N // 2 + 1), (N // 3, 5 * N // 6),           # overlapping
    ], N)


def islands(N, bs):
    """Edges only inside [10, 40], [bs + 5, 3 bs - 7] and [4 bs, 5 bs - 1], none
    reaching the last three nodes: nodes 0..10, the gaps and the end are covered
    by no edge (1 / M = inf there), and nothing moves the last node's block
    explicitly."""
    a1, b1 = bs + 5, 3 * bs - 7
    a2, b2 = 4 * bs, 5 * bs - 1
    return _fit([
        (10, 40), (12, 20), (40, 13),
        (a1, b1), (a1 + 1, a1 + 3), (a1 + 2, 2 * bs - 1), (2 * bs - 1, 2 * bs + 1), (2 * bs, b1), (b1, a1 + 4),
        (a2, a2 + 2), (a2 + 1, b2), (a2, a2 + bs // 2), (a2 + 3, a2 + 4), (a2 + bs // 2, b2),
    ], N, hi=N - 4)


def dense(N, E, seed):
    """E distinct random pairs: ~5 % adjacent, ~10 % reversed, the rest a < b."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < E:
        u = rng.random()
        if u < 0.05:
            a = int(rng.integers(0, N - 1))
            a, b = (a, a + 1) if rng.random() < 0.5 else (a + 1, a)
        else:
            a, b = sorted(int(v) for v in rng.choice(N, size=2, replace=False))
            if b - a == 1:
                continue
            if u < 0.15:
                a, b = b, a
        if (a, b) not in seen:
            seen.add((a, b))
            out.append((a, b))
    return out


def is_active(a, b):
    """The edges pass 2 applies: loop edges (|a - b| != 1) with a < b."""
    return abs(int(a) - int(b)) != 1 and int(a) < int(b)


def residual_margin(poses, ea, eb, tf, lr, sigma_v=SIGMA):
    """``pgo_oracle.sgd_step`` restated (same operations in the same order: the
    poses are bit-identical), in place on ``poses``.  Returns (poses, margin,
    clamped, unclamped): the smallest distance of an applied edge's raw heading
    residual (before ``% 2 pi``) to a multiple of 2 pi, and how many beta
    components the clamp replaced by r / left alone."""
    N = len(poses)
    sigma = np.eye(3) * sigma_v
    loops = [e for e in range(len(ea)) if abs(int(ea[e]) - int(eb[e])) != 1]
    M = np.zeros((N, 3))
    gamma = np.full(3, np.inf)
    for e in loops:
        a, b = int(ea[e]), int(eb[e])
        R = po._rot(poses[a][2])
        dW = np.diag(np.linalg.inv(R @ sigma @ R.T))
        if b >= a + 1:
            M[a + 1:b + 1] = M[a + 1:b + 1] + dW
            if np.dot(gamma, gamma) > np.dot(dW, dW):
                gamma = dW
    margin, clamped, unclamped = np.inf, 0, 0
    for e in loops:
        a, b = int(ea[e]), int(eb[e])
        if b < a + 1:
            continue
        R = po._rot(poses[a][2])
        r = po._mat_pose(po._pose_mat(poses[a]) @ tf[e]) - poses[b]
        raw = r[2]
        margin = min(margin, abs(raw - TWO_PI * np.round(raw / TWO_PI)))
        r[2] = r[2] % TWO_PI
        d = 2 * np.linalg.inv(R.T @ sigma @ R) @ r.reshape(-1, 1)
        for j in range(3):
            alpha = 1 / gamma[j]
            alpha *= lr
            tw = np.sum(1 / M[a + 1:b + 1, j])
            beta = (b - a) * d[j, 0] * alpha
            if np.abs(beta) > np.abs(r[j]):
                beta = r[j]
                clamped += 1
            else:
                unclamped += 1
            ramp = np.cumsum(beta / M[a + 1:b + 1, j] / tw)
            poses[a + 1:b + 1, j] = poses[a + 1:b + 1, j] + ramp
            poses[b + 1:, j] = poses[b + 1:, j] + ramp[-1]
    return poses, margin, clamped, unclamped


class Case:
    """A graph and the oracle's single steps from its initial poses (one per
    learning rate in LRS; never chained: after an lr = 1 step a closed edge's
    residual sits on the wrap point).  Arrays are read-only and shared."""

    def __init__(self, name, N, shift, pairs, seed):
        self.name, self.N, self.shift, self.pairs, self.seed = name, N, shift, pairs, seed
        self.poses, self.ea, self.eb, self.tf = lap_graph(N, pairs, seed)
        self.ref = {}
        for lr in LRS:
            self.ref[lr] = po.sgd_step(self.poses.copy(), self.ea, self.eb, self.tf, lr, SIGMA)
        for a in (self.poses, self.ea, self.eb, self.tf, *self.ref.values()):
            a.setflags(write=False)

    @property
    def active(self):
        return [(int(a), int(b)) for a, b in zip(self.ea, self.eb) if is_active(a, b)]

    def first_a(self):
        """Smallest active a: nodes up to it are never written (N if no edge applies)."""
        return min((a for a, _ in self.active), default=self.N)


@functools.lru_cache(maxsize=None)
def case(kind, N, shift):
    """kind 'structural' or 'islands' for N nodes and blocks of 2^shift."""
    pairs = {"structural": structural, "islands": islands}[kind](N, 1 << shift)
    return Case(f"{kind}-N{N}-sh{shift}", N, shift, pairs, SEEDS.get((kind, N, shift), 0))


def graph_keys():
    """(kind, N, shift) of every structural / islands graph the GPU tests run:
    the automatic cases with the shift of their intended plan, the forced ones
    with the forced shift (6 on the one-wave paths)."""
    keys = [("structural", N, AUTO_PLAN[N][2]) for N in AUTO_STRUCTURAL]
    keys += [("islands", N, AUTO_PLAN[N][2]) for N in AUTO_ISLANDS]
    for _, sh, N in FORCED:
        keys += [(kind, N, 6 if sh < 0 else sh) for kind in ("structural", "islands")]
    return list(dict.fromkeys(keys))


@functools.lru_cache(maxsize=None)
def dense_case(E):
    seed = DENSE_SEEDS.get(E, 0)
    return Case(f"dense-E{E}", DENSE_N, 6, dense(DENSE_N, E, seed), seed)


@functools.lru_cache(maxsize=None)
def inactive_case():
    """Only adjacent and reversed edges: the compaction keeps none (K = 0)."""
    pairs = [(5, 6), (40, 3), (7, 6), (199, 0), (100, 20), (21, 22)]
    return Case("inactive", 200, 6, pairs, 0)


def relations(pairs, N, shift):
    """Which structural relations the ACTIVE edges of a graph show, from
    (a, b, shift) alone (the kernel's node_of and whole-block loops)."""
    bs = 1 << shift
    nblk = ((N - 1) >> shift) + 1
    act = [(a, b) for a, b in pairs if is_active(a, b)]
    rel = set()
    for k, (a, b) in enumerate(act):
        ba, bb = a >> shift, b >> shift
        n1 = min(N, (ba + 1) << shift) - (a + 1)
        n2 = min(N, (bb + 1) << shift) - (bb << shift) if bb > ba else 0
        rel.add("a=0" if a == 0 else "a>0")
        if b == N - 1:
            rel.add("b=N-1")
        if ba == bb:
            rel.add("same block")
        if bb == ba + 1:
            rel.add("adjacent blocks")
        if (b + 1) % bs == 0:
            rel.add("b on a block's last node")
        if (a + 1) % bs == 0:
            rel.add("a on a block's last node")
        if bb == nblk - 1 and N % bs != 0:
            rel.add("b in the partial last block")
        if bb - ba >= 2:
            rel.add("whole block inside a ramp")
        if bb < nblk - 1:
            rel.add("whole block in a tail")
        if n1 + n2 > 2 * 256:
            rel.add("more than 2 x 256 explicit nodes")
        if k + 2 < len(act) and act[k + 1][0] == a and act[k + 2][0] == a:
            rel.add("three consecutive edges out of one node")
    if any(not is_active(a, b) for a, b in pairs) and act:
        rel.add("inactive edges interleaved")
    return rel


def expected_relations(N, shift):
    """The relations structural(N, 2^shift) must show: each one as soon as N
    has room for the edge that carries it."""
    bs = 1 << shift
    want = {"a=0", "b=N-1", "same block"}                      # (0, N - 1), (0, 2): N >= 3
    if N >= 5:
        want.add("a>0")                                        # (N - 3, N - 1)
    if N >= bs:
        want.add("b on a block's last node")                   # (3, bs - 1)
    if N > bs:
        want.add("whole block in a tail")                      # (0, 2) with a second block
    if N >= bs + 2:
        want |= {"adjacent blocks", "a on a block's last node"}   # (bs - 1, bs + 1)
    if N % bs:
        want.add("b in the partial last block")                # (0, N - 1)
    if N > 2 * bs:
        want.add("whole block inside a ramp")                  # (0, N - 1) spans block 1
        if shift >= 9:
            want.add("more than 2 x 256 explicit nodes")       # (bs, 2 bs): 2 bs - 1 > 512
    if N >= 41:
        want |= {"three consecutive edges out of one node", "inactive edges interleaved"}
    return want


def covered(pairs, N):
    """Nodes some active edge's ramp (a, b] covers."""
    c = np.zeros(N, dtype=bool)
    for a, b in pairs:
        if is_active(a, b):
            c[a + 1:b + 1] = True
    return c


# ---- orientation ------------------------------------------------------------

ORIENT_N = (0, 1, 2, 3, 257, 258, 259, 513)
ORIENT_TF_N = (1, 2, 257, 258)


def zero_runs(N):
    """Two runs of identical consecutive positions [lo, hi] (as far as N has
    room): one early, one across the 256-thread block edge of orient_kernel
    (thread t of block k handles node 1 + 256 k + t)."""
    return [(lo, hi) for lo, hi in ((1, 3), (254, 258)) if hi < N]


def orient_case(N, seed=0):
    """(N, 3) poses: a random walk with steps of ~0.1 m, headings unrelated to
    the steps, and the zero-length steps of zero_runs(N)."""
    rng = np.random.default_rng(1000 + N + seed)
    step = rng.normal(0.0, 0.1, (N, 2))
    for lo, hi in zero_runs(N):
        step[lo + 1:hi + 1] = 0.0
    poses = np.concatenate([np.cumsum(step, axis=0), rng.uniform(-3.0, 3.0, (N, 1))], axis=1)
    poses.setflags(write=False)
    return poses


def orient_tf_case(N, seed=0):
    """(poses, tfs): N - 1 rotation-only transforms of pairs (i, i - 1).  The
    update theta_i = theta_{i-1} + delta_i must read the OLD theta_{i-1}: the
    deltas are drawn so that the new one is more than 0.1 rad away."""
    rng = np.random.default_rng(2000 + N + seed)
    poses = np.concatenate([rng.normal(0.0, 1.0, (N, 2)), rng.uniform(-3.0, 3.0, (N, 1))], axis=1)
    delta = rng.uniform(-1.0, 1.0, max(N - 1, 0))      # delta[i - 1] belongs to node i
    for i in range(2, N):
        if abs(poses[i - 2, 2] + delta[i - 2] - poses[i - 1, 2]) <= 0.2:
            delta[i - 2] += 0.5
    tfs = np.stack([_pose_mat([0.0, 0.0, d]) for d in delta]) if N > 1 else np.zeros((0, 3, 3))
    poses.setflags(write=False)
    tfs.setflags(write=False)
    return poses, tfs


def orient_from_tf_ref(poses, tfs):
    """The reverse-order loop of ``pgo_oracle.recompute_orientation``."""
    for i in range(len(poses) - 1, 0, -1):
        t = tfs[i - 1]
        poses[i][2] = poses[i - 1][2] + np.arctan2(t[1][0], t[0][0])
    return poses
