"""CPU tests of the visibility check: the NumPy restatement tests/vis_ref.py
against plain double loops and hand-placed cases, the separation of right and
wrong stage-1 edges, the host-side argument checks of the built library and the
opt-in defaults of the stages.  tests/test_vis_gpu.py compares the device with
the restatement."""
import functools
import inspect
import math
import os

import numpy as np
import pytest

import vis_ref as ref

import slamhip.vis  # noqa: F401  (the feature under test: absent before it)
from slamhip import se2, synthetic

INF = float("inf")


# ---------------------------------------------------------------- plain double loops

def plain_sector(x, y, d):
    best, best_k = (d[0][0] * x) + (d[0][1] * y), 0
    for k in range(1, len(d)):
        v = (d[k][0] * x) + (d[k][1] * y)
        if v > best:
            best, best_k = v, k
    return best_k


def plain_table(points, d):
    out = [INF] * len(d)
    for x, y in points:
        x, y = float(x), float(y)
        r2 = (x * x) + (y * y)
        if not math.isfinite(r2):
            continue
        k = plain_sector(x, y, d)
        out[k] = min(out[k], r2)
    return np.array(out)


def plain_direction(points, M, R2, d, margin, W):
    S = len(d)
    agree = conflict = 0
    for x, y in points:
        x, y = float(x), float(y)
        qx = ((M[0][0] * x) + (M[0][1] * y)) + M[0][2]
        qy = ((M[1][0] * x) + (M[1][1] * y)) + M[1][2]
        rq = math.sqrt((qx * qx) + (qy * qy))
        k = plain_sector(qx, qy, d)
        ag, all_seen, lo = False, True, INF
        for w in range(-W, W + 1):
            e = float(R2[(k + w) % S])
            if not math.isfinite(e):
                all_seen = False
                continue
            re = math.sqrt(e)
            ag = ag or abs(re - rq) <= margin
            lo = min(lo, re)
        if ag:
            agree += 1
        elif all_seen and rq + margin < lo:
            conflict += 1
    return agree, conflict, len(points)


def pack(scans):
    lens = [len(s) for s in scans]
    off = np.zeros(len(scans) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    pts = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in scans]) if scans else np.zeros((0, 2))
    return pts, off


def test_restatement_against_plain_loops():
    """Tables and both directions of five edges over 6 small ragged scans, at
    S = 3, 8 and 45 and windows 0..2, with the edges' right transforms and with
    one 0.3 m off (so that all three outcomes occur)."""
    seq = synthetic.make_sequence(6, seed=9, n_beams=61, dropout=0.3)
    assert len({len(s) for s in seq.scans}) > 2
    seen = np.zeros(3, dtype=np.int64)
    for S, W in ((3, 0), (3, 1), (8, 0), (8, 1), (45, 2)):
        d = ref.dirs(S)
        tabs = [ref.table(s, d) for s in seq.scans]
        for s, t in zip(seq.scans, tabs):
            assert np.array_equal(t, plain_table(s, d))
        for i in range(1, 6):
            T = np.linalg.inv(se2.pose_to_mat(seq.truth[i - 1])) @ se2.pose_to_mat(seq.truth[i])
            T[2] = (0.0, 0.0, 1.0)
            for shift in (0.0, 0.3):
                Ts = T.copy()
                Ts[0, 2] += shift
                got = ref.edge(seq.scans[i], seq.scans[i - 1], Ts, d, 0.15, W)
                a = plain_direction(seq.scans[i], Ts, tabs[i - 1], d, 0.15, W)
                b = plain_direction(seq.scans[i - 1], ref.inverse(Ts), tabs[i], d, 0.15, W)
                assert tuple(got) == a + b, (S, W, i, shift)
                seen += (got[0] + got[3], got[1] + got[4], got[2] + got[5] - got[0] - got[1] - got[3] - got[4])
    assert (seen > 0).all(), seen      # agreeing, conflicting and unknown points all occur


def test_points_that_are_not_finite_take_no_part():
    d = ref.dirs(8)
    pts = np.array([[1.0, 0.5], [np.nan, 1.0], [np.inf, 0.0], [1e200, 1e200], [-2.0, 0.25]])
    t = ref.table(pts, d)
    assert np.array_equal(t, plain_table(pts, d)) and np.isfinite(t).sum() == 2
    got = ref.direction(pts, np.eye(3), t, d, 0.25, 1)[:3]
    with np.errstate(all="ignore"):
        assert got == plain_direction(pts, np.eye(3), t, d, 0.25, 1) == (2, 0, 5)


# ---------------------------------------------------------------- hand-placed cases

MARGIN, S8 = 0.25, 8

# Eight sector centres with dyadic entries, mirror images of each other in both axes (np.cos / np.sin give
# centres that differ in the last bit, so with them no point off the origin ties exactly): a point on a
# half-axis projects equally onto the two sectors beside it.  The rule takes any table of centres.
TIE_DIRS = np.array([[1.0, 0.5], [0.5, 1.0], [-0.5, 1.0], [-1.0, 0.5], [-1.0, -0.5], [-0.5, -1.0], [0.5, -1.0],
                     [1.0, -0.5]])


def axis_sectors():
    """(centres, the sectors of the four half-axes): each half-axis ties between
    two sectors and the first takes it: 0 (not 7), 1, 3 and 5."""
    d = TIE_DIRS
    return d, [int(ref.sectors([x], [y], d)[0]) for x, y in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))]


def hand_cases():
    """name -> (src scan, dst scan, T, W, expected six counts).  Dyadic
    coordinates on the axes (multiples of 1/8), margin 0.25, the S = 8 centres
    ``TIE_DIRS``: every product, sum and square root below is exact."""
    I = np.eye(3)
    below = np.nextafter(1.75, 0.0)
    cases = {
        # |re - rq| == margin on both sides of the surface: agrees
        "at_margin": ([[1.75, 0.0], [2.25, 0.0]], [[2.0, 0.0]], I, 0, [2, 0, 2, 1, 0, 1]),
        # rq + margin == re is no conflict (it agrees); one ulp nearer conflicts; one ulp beyond the far side is unknown
        "one_ulp": ([[1.75, 0.0], [below, 0.0], [np.nextafter(2.25, 3.0), 0.0]], [[2.0, 0.0]], I, 0, None),
        # the origin: every projection is 0, sector 0; r2 = 0
        "origin": ([[0.0, 0.0]], [[0.0, 0.0]], I, 0, [1, 0, 1, 1, 0, 1]),
    }
    return cases


def test_hand_placed_margin_and_ulp():
    d, ax = axis_sectors()
    cases = hand_cases()
    src, dst, T, W, want = cases["at_margin"]
    assert list(ref.edge(src, dst, T, d, MARGIN, W)) == want
    src, dst, T, W, _ = cases["one_ulp"]
    a, c, n, am, cm = ref.direction(src, T, ref.table(dst, d), d, MARGIN, W)
    assert (a, c, n) == (1, 1, 3)
    assert list(am) == [True, False, False] and list(cm) == [False, True, False]
    assert np.nextafter(1.75, 0.0) + MARGIN < 2.0 and 1.75 + MARGIN == 2.0     # the two sides of the strict <
    assert plain_direction(src, T, ref.table(dst, d), d, MARGIN, W) == (1, 1, 3)


def test_hand_placed_ties_and_origin():
    d, ax = axis_sectors()
    # the +x half-axis lies between sectors S - 1 and 0, whose centres mirror each other in it
    assert d[0, 0] == d[S8 - 1, 0] and d[0, 1] == -d[S8 - 1, 1]
    assert (d[0, 0] * 2.0) + (d[0, 1] * 0.0) == (d[S8 - 1, 0] * 2.0) + (d[S8 - 1, 1] * 0.0)
    assert ax == [0, 1, 3, 5]                               # the tie goes to 0, not to S - 1; the others likewise
    assert [plain_sector(x, y, d) for x, y in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))] == ax
    t = ref.table([[2.0, 0.0]], d)
    assert t[0] == 4.0 and np.isinf(t[1:]).all()
    assert int(ref.sectors([0.0], [0.0], d)[0]) == 0        # the origin
    assert ref.table([[0.0, 0.0]], d)[0] == 0.0
    src, dst, T, W, want = hand_cases()["origin"]
    assert list(ref.edge(src, dst, T, d, MARGIN, W)) == want


def test_hand_placed_unseen_entry():
    """Window 1 around the +x half-axis' sector 0: entries 7, 0 and 1."""
    d, ax = axis_sectors()
    R2 = np.full(S8, np.inf)
    R2[[7, 0, 1]] = 4.0
    pts = [[1.0, 0.0], [2.0, 0.0]]
    assert ref.direction(pts, np.eye(3), R2, d, MARGIN, 1)[:3] == (1, 1, 2)    # 1 m: free space; 2 m: the surface
    for hole in (7, 1):
        R = R2.copy()
        R[hole] = np.inf
        # the unseen entry blocks the conflict of the near point, not the agreement of the far one
        assert ref.direction(pts, np.eye(3), R, d, MARGIN, 1)[:3] == (1, 0, 2), hole
        assert plain_direction(pts, np.eye(3), R, d, MARGIN, 1) == (1, 0, 2)
    R = R2.copy()
    R[0] = np.inf                                            # the point's own sector unseen, a neighbour agrees
    assert ref.direction(pts, np.eye(3), R, d, MARGIN, 1)[:3] == (1, 0, 2)
    R = R2.copy()
    R[1] = 1.0                                               # the minimum over the window decides the conflict
    assert ref.direction([[0.5, 0.0]], np.eye(3), R, d, MARGIN, 1)[:3] == (0, 1, 1)
    assert ref.direction([[0.875, 0.0]], np.eye(3), R, d, MARGIN, 1)[:3] == (1, 0, 1)
    assert ref.direction([[1.5, 0.0]], np.eye(3), R, d, MARGIN, 1)[:3] == (0, 0, 1)   # behind the nearest: unknown


def quarter_turn_case():
    """A transform of exactly 90 degrees (entries 0 and +-1) with a dyadic
    translation: (src, dst, T, expected counts at W = 0)."""
    T = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.25], [0.0, 0.0, 1.0]])
    src = [[2.0, 0.0], [0.0, -1.0]]          # -> (0, 2.25) and (1, 0.25)
    dst = [[0.0, 2.25], [0.0, -3.0]]         # <- (2, 0) and (-3.25, 0)
    return src, dst, T


def test_hand_placed_quarter_turn_and_inverse():
    d, ax = axis_sectors()
    src, dst, T = quarter_turn_case()
    Ti = ref.inverse(T)
    assert np.array_equal(Ti, [[0.0, 1.0, -0.25], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])    # -0.0 == 0.0
    assert np.array_equal(Ti @ T, np.eye(3)) and np.array_equal(T @ Ti, np.eye(3))
    q = (Ti @ np.c_[np.asarray(dst), np.ones(2)].T).T[:, :2]
    assert np.array_equal(q, [[2.0, 0.0], [-3.25, 0.0]])
    # direction 0: (2, 0) lands on dst's (0, 2.25): agrees; (0, -1) lands at (1, 0.25), in a sector dst never saw
    # direction 1: (0, 2.25) lands on src's (2, 0): agrees; (0, -3) lands at (-3.25, 0), a sector src never saw
    assert list(ref.edge(src, dst, T, d, MARGIN, 0)) == [1, 0, 2, 1, 0, 2]
    # the transform itself in place of its inverse would map dst's points elsewhere
    wrong = ref.direction(dst, T, ref.table(src, d), d, MARGIN, 0)[:3]
    assert wrong != (1, 0, 2)
    # a second source point in front of dst's surface: (1.5, 0) -> (0, 1.75), 0.5 m short of 2.25
    assert list(ref.edge(src + [[1.5, 0.0]], dst, T, d, MARGIN, 0))[:3] == [1, 1, 3]


# ---------------------------------------------------------------- the verdict and the candidate key

def test_verdict():
    vis = slamhip.vis
    p = vis.VisParams()
    assert (p.sectors, p.window, p.margin, p.min_agree, p.max_conflict) == (360, 1, 0.15, 0.25, 0.02)
    assert p.tables_key == (360,) and vis.VisParams(sectors=64, margin=0.3).tables_key == (64,)
    counts = np.array([[980, 5, 1000, 990, 0, 1000],      # passes
                       [250, 5, 1000, 990, 0, 1000],      # agree == min_agree n, conflict 5 / 255 <= 0.02
                       [249, 0, 1000, 990, 0, 1000],      # too few agree in direction 0
                       [980, 5, 1000, 980, 21, 1000],     # conflict 21 / 1001 > 0.02 in direction 1
                       [980, 20, 1000, 980, 20, 1000],    # 20 / 1000 == 0.02: passes
                       [0, 0, 0, 0, 0, 10],               # an empty scan fails
                       [-1, -1, -1, -1, -1, -1]])         # flagged on the device
    want = [True, True, False, False, True, False, False]
    assert list(p.passes(counts)) == want and list(ref.passes(counts)) == want
    a, c = vis.shares(counts)
    ra, rc = ref.shares(counts)
    assert np.array_equal(a, ra) and np.array_equal(c, rc)
    assert a[0, 0] == 0.98 and c[3, 1] == 21 / 1001 and a[5, 0] == 0 and c[5, 0] == 0
    for bad in (dict(sectors=2), dict(sectors=1025), dict(window=-1), dict(sectors=8, window=4), dict(margin=-0.1),
                dict(margin=float("nan")), dict(min_agree=1.5), dict(max_conflict=-0.1), dict(sectors=8.5)):
        with pytest.raises(ValueError):
            vis.VisParams(**bad)
    assert vis.VisParams(sectors=3, window=1).window == 1   # the whole circle
    with pytest.raises(Exception):
        p.margin = 1.0                                      # frozen
    assert np.array_equal(vis.sector_dirs(360), ref.dirs(360))


def test_candidate_key_order():
    """Fewest conflicts, then most agreeing points, then the order ICP result,
    refined, init; a passing repair candidate goes before any key."""
    from slamhip import pipeline
    vis = slamhip.vis
    icp = [100, 700, 1000, 90, 650, 1000]
    refined = [900, 30, 1000, 880, 40, 1000]
    init = [850, 30, 1000, 860, 40, 1000]
    keys = [vis.candidate_key(c, o) for o, c in enumerate((icp, refined, init))]
    assert keys == [ref.candidate_key(c, o) for o, c in enumerate((icp, refined, init))]
    assert keys == [(1350, -190, 0), (70, -1780, 1), (70, -1710, 2)] and min(keys) == keys[1]
    none = [False, False, False]
    assert pipeline.choose_candidate([icp, refined, init], none, [0, 1, 2]) == 1
    assert pipeline.choose_candidate([icp, init, init], none, [0, 1, 2]) == 1          # a full tie: the order
    assert pipeline.choose_candidate([refined, icp, icp], none, [0, 1, 2]) == 0        # the ICP result is candidate 0
    assert pipeline.choose_candidate([icp, init], none, [0, 2]) == 1                   # no usable refinement
    assert pipeline.choose_candidate([icp, refined, init], [False, False, True], [0, 1, 2]) == 2
    assert pipeline.choose_candidate([icp, refined, init], [False, True, True], [0, 1, 2]) == 1


# ---------------------------------------------------------------- right and wrong stage-1 edges

@functools.lru_cache(maxsize=None)
def loop600():
    """``make_loop_sequence(600, 3)``, its 599 oracle ICP edges (the fixture
    tests/golden/vis_loop600_icp.npz, written by tests/golden/gen_vis.py: three
    minutes of oracle ICP on one core), the restatement's counts of them and the
    tables.  Once per session."""
    from conftest import GOLDEN
    seq = synthetic.make_loop_sequence(600, 3)
    with np.load(os.path.join(GOLDEN, "vis_loop600_icp.npz"), allow_pickle=False) as z:
        tf = z["tf"]
    assert tf.shape == (599, 3, 3)
    d = ref.dirs(360)
    tabs = np.stack([ref.table(s, d) for s in seq.scans])
    counts = np.stack([ref.edge(seq.scans[i], seq.scans[i - 1], tf[i - 1], d, R2_src=tabs[i], R2_dst=tabs[i - 1])
                       for i in range(1, 600)])
    return seq, tf, counts, tabs


CORNERS = [152, 264, 416, 528]


def test_fixture_edges_are_the_oracles():
    """A wrong corner edge and a right edge, computed here by the oracle."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    try:
        import gen_vis
    finally:
        sys.path.remove(GOLDEN)
    seq, tf, _, _ = loop600()
    for i in (152, 300):
        assert np.abs(gen_vis.oracle_edge(seq, i) - tf[i - 1]).max() <= 1e-9, i   # the tolerance of icp() elsewhere


def test_separation_of_right_and_wrong_edges():
    """All 599 edges (no cut to the corners' neighbourhoods: the oracle's
    edges come from the fixture).  The failing edges are exactly the four
    corners; a passing edge has conflict share <= 0.01 (measured: 0.0066) and
    a failing one >= 0.5 (measured: 0.7475), in its worse direction."""
    seq, tf, counts, _ = loop600()
    ok = ref.passes(counts)
    agree, conflict = ref.shares(counts)
    print("passing: smaller agree share", agree[ok].min(), "larger conflict share", conflict[ok].max())
    print("failing: smaller agree share", agree[~ok].min(axis=1), "larger conflict share", conflict[~ok].max(axis=1))
    assert list(np.nonzero(~ok)[0] + 1) == CORNERS
    assert conflict[ok].max() <= 0.01
    assert conflict[~ok].max(axis=1).min() >= 0.5
    assert agree[ok].min() >= 0.9 and agree[~ok].min(axis=1).max() <= 0.25
    # the truth: a corner edge passes at its true transform, so the check flags the ICP result, not the place
    d = ref.dirs(360)
    for i in CORNERS:
        T = np.linalg.inv(se2.pose_to_mat(seq.truth[i - 1])) @ se2.pose_to_mat(seq.truth[i])
        T[2] = (0.0, 0.0, 1.0)
        assert ref.passes(ref.edge(seq.scans[i], seq.scans[i - 1], T, d))[0], i


# ---------------------------------------------------------------- host-side argument checks (no GPU)

def _aligned(nbytes):
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, a + (-a) % 64


def test_host_validation():
    """Null arrays, S, W, the margin and negative sizes are refused, and B = 0
    and n_scans = 0 succeed, before anything touches a device."""
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 108
    EINVAL = -1
    keep, p = _aligned(256)      # never dereferenced: every call below returns before a launch

    def check(pts=p, n_scans=4, P=100, S=360, tables=p, B=0, margin=0.15, W=1, out=p):
        return lib.slam_vis_check_f64(pts, p, n_scans, P, p, S, tables, p, p, p, B, margin, W, out, None)

    assert check() == 0
    assert check(n_scans=0) == 0
    for kw in ({"pts": None}, {"tables": None}, {"out": None}, {"pts": None, "B": 3}):
        assert check(**kw) == EINVAL and b"null" in lib.slam_last_error(), kw
    assert check(B=-1) == EINVAL and check(n_scans=-1) == EINVAL and check(P=-1) == EINVAL
    for S in (2, 0, -5, 1025):
        assert check(S=S) == EINVAL and b"S =" in lib.slam_last_error(), S
    assert check(S=3, W=1) == 0 and check(S=1024, W=511) == 0 and check(S=8, W=3) == 0
    for S, W in ((3, 2), (8, 4), (1024, 512), (360, -1), (360, 2 ** 31 - 1)):
        assert check(S=S, W=W) == EINVAL and b"W =" in lib.slam_last_error(), (S, W)
    for m in (-0.1, float("inf"), float("nan")):
        assert check(margin=m) == EINVAL and b"margin" in lib.slam_last_error(), m
    assert check(margin=0.0) == 0
    assert check(pts=p + 8) == EINVAL and b"aligned" in lib.slam_last_error()

    def tables(pts=p, n_scans=0, P=100, S=360, dirs=p, out=p):
        return lib.slam_vis_tables_f64(pts, p, n_scans, P, dirs, S, out, None)

    assert tables() == 0
    for kw in ({"pts": None}, {"dirs": None}, {"out": None}):
        assert tables(**kw) == EINVAL and b"null" in lib.slam_last_error(), kw
    assert tables(n_scans=-1) == EINVAL and tables(P=-1) == EINVAL
    assert tables(S=2) == EINVAL and tables(S=1025) == EINVAL and tables(S=3) == 0 and tables(S=1024) == 0
    del keep


def test_stages_take_verify_none_by_default():
    from slamhip import pipeline
    import src.icp
    import src.loop_closure_detection as lcd
    for fn in (pipeline.scan_matching, pipeline.manual_loop_closures, pipeline.proximity_loop_closures,
               pipeline.signature_loop_closures, pipeline.image_loop_closures, pipeline.image_stage,
               lcd.detect_proximity, lcd.detect_signatures):
        par = inspect.signature(fn).parameters
        assert par["verify"].default is None, fn.__name__
    par = inspect.signature(pipeline.scan_matching).parameters
    assert par["repair"].default == "refine-from-init" and par["repair_refine"].default is None
    assert list(par)[:7] == ["odometry", "lidar_points", "icp_max_iters", "icp_epsilon", "scanset", "refine",
                             "refine_gates"]                  # the new keywords come last
    r = pipeline.ScanMatchResult(np.zeros((1, 3)), np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0, np.int64))
    assert r.verify_ok is None and r.verify_counts is None and r.repaired is None and r.repair_source is None
    assert callable(pipeline.check_edges) and callable(src.icp.check_visibility)
    with pytest.raises(TypeError):
        pipeline.scan_matching(np.zeros((1, 3)), [np.zeros((3, 2))], verify=True)
    with pytest.raises(ValueError):
        pipeline.scan_matching(np.zeros((1, 3)), [np.zeros((3, 2))], repair="again")


def test_driver_flags():
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("main_batched_vis", os.path.join(PKG, "scripts", "main_batched.py"))
    mb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mb)
    a = mb.parse(["synthetic:loop:10"])
    assert a.edge_check == "none" and a.scan_matching_repair == "refine-from-init" and mb.edge_check_params(a) == {}
    a = mb.parse(["synthetic:loop:10", "--edge-check", "visibility", "--edge-check-margin", "0.2",
                  "--edge-check-sectors", "180", "--edge-check-max-conflict", "0.05", "--edge-check-min-agree", "0.3",
                  "--scan-matching-repair", "none"])
    v = mb.edge_check_params(a)["verify"]
    assert (v.sectors, v.window, v.margin, v.min_agree, v.max_conflict) == (180, 1, 0.2, 0.3, 0.05)
    assert a.scan_matching_repair == "none"
    with pytest.raises(SystemExit):
        mb.parse(["synthetic:loop:10", "--edge-check-sectors", "2"])
