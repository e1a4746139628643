"""Batched SLAM driver: the GPU flow of ``scripts/main.py`` stages 1-3.

The reference runs its hot path from ``scripts/main.py``:

* stage 1, scan matching (``scripts/main.py:236-263``): ``icp.icp`` on every
  consecutive pair (i, i-1) with init ``pose_to_mat(odom_i - odom_{i-1})``,
  fanned out over a joblib pool, then the serial odometry chain
  ``P_i = mat_to_pose(pose_to_mat(P_{i-1}) @ T_i)`` and a ``PoseGraph``;
* stage 2, manual loop closures (``scripts/main.py:298-307``): ``icp.icp``
  with an identity init for every annotated (i, j); the constraint is added
  when the returned error is below 30; or, opt-in, the reference's lidar-only
  detector (``src/loop_closure_detection.py:11-39``) with its candidate search
  on the GPU (``proximity_loop_closures``); or, opt-in, its image detector
  (``:81-163``) from the ORB descriptors on, every image pair matched on the
  GPU (``image_loop_closures``; extracting the keypoints needs OpenCV and
  stays out of scope); or, opt-in and without a counterpart in the reference,
  candidates from the scans' own rotation-invariant signatures
  (``signature_loop_closures``, ``slamhip.sig``); then, opt-in and without a
  counterpart either, the closures checked against each other and the
  inconsistent ones removed (``verify_loop_closures``, ``slamhip.pcm``); and,
  opt-in in stage 1 and in every loop-closure stage, each edge judged on its
  own by scan visibility (``verify=``, ``slamhip.vis``): a stage-1 edge that
  fails is re-matched from its odometry init (``repair_edges``), a closure that
  fails is not added;
* stage 3, optimisation (``scripts/main.py:322-334``): ``optimization_max_iters``
  SGD steps with learning rate 1/(k+1), then the orientation recompute.

Here each ICP stage is ONE batched kernel launch (``slamhip.icp.IcpBatch``),
the SGD steps run on a device-resident ``SgdSolver`` (poses stay in HBM for
all steps), and the Gauss-Newton solve (``slamhip.gn``) is available as an
alternative optimiser.  Results equal the reference flow's: the per-pair ICP
results are the reference's (tests/test_icp_gpu.py), the chain is composed on
the host with the reference's own arithmetic, and the SGD/orientation kernels
match ``oracle/pgo_oracle.py`` (tests/test_pipeline_gpu.py).
"""
from dataclasses import dataclass

import numpy as np

from . import se2

LOOP_CLOSURE_ICP_ERROR = 30.0   # scripts/main.py:306 (manual path; --loop-closure-icp-error for detection)


@dataclass
class ScanMatchResult:
    poses: np.ndarray      # (S, 3) corrected poses (odometry chain of the ICP edges)
    tf: np.ndarray         # (S-1, 3, 3) transforms[-1] of every pair (i, i-1)
    err: np.ndarray        # (S-1,) ICP errors
    iters: np.ndarray      # (S-1,) ICP iterations
    refine_status: np.ndarray = None    # (S-1,) slamhip.plicp statuses of the point-to-line refinement (refine=...)
    refine_inliers: np.ndarray = None   # (S-1,) its inliers
    refine_obs: np.ndarray = None       # (S-1,) its observability
    refine_taken: np.ndarray = None     # (S-1,) bool: the edges whose transform is the refined one
    verify_ok: np.ndarray = None        # (S-1,) bool: the ICP edges that pass the visibility check (verify=...)
    verify_counts: np.ndarray = None    # (S-1, 6) its counts of the ICP edges (slamhip.vis)
    repaired: np.ndarray = None         # (S-1,) bool: the edges whose transform is not the ICP result's
    repair_source: np.ndarray = None    # (S-1,) 0 the ICP result, 1 refined from the odometry init, 2 the init itself


REFINE_GATES = (0.5, 0.0)   # (min_overlap, min_observability) of slamhip.plicp.apply_refinement


def refine_edges(scanset, src, dst, tf, refine, gates=REFINE_GATES):
    """The point-to-line refinement of the ICP edges icp(pc1 = src[b], pc2 =
    dst[b]) -> ``tf`` (new, opt-in; ``slamhip.plicp``): ONE launch over the
    resident ``scanset``, then ``apply_refinement`` with ``gates`` = (min_overlap,
    min_observability).  ``refine``: the ``PlicpParams``.  Returns the transforms,
    the mask of those that took the refinement and the ``PlicpResult``."""
    from . import plicp as _plicp
    if not isinstance(refine, _plicp.PlicpParams):
        raise TypeError(f"refine must be a slamhip.plicp.PlicpParams or None, got {type(refine).__name__}")
    src = np.asarray(src, dtype=np.int64)
    res = _plicp.refine_batch(scanset, src, dst, tf, refine)
    out, taken = _plicp.apply_refinement(tf, scanset.lens[src], res, gates[0], gates[1])
    return out, taken, res


def _edge_transforms(scanset, src, dst, tf, refine, gates):
    """``tf`` itself without a refinement (the default), else ``refine_edges``' transforms."""
    return tf if refine is None else refine_edges(scanset, src, dst, tf, refine, gates)[0]


EDGE_REPAIRS = ("none", "refine-from-init")


def _vis_params(verify):
    from . import vis as _vis
    if not isinstance(verify, _vis.VisParams):
        raise TypeError(f"verify must be a slamhip.vis.VisParams or None, got {type(verify).__name__}")
    return _vis


def check_edges(scanset, src, dst, tf, params):
    """The visibility check of the edges icp(pc1 = src[b], pc2 = dst[b]) ->
    ``tf[b]`` over the resident ``scanset`` (new, opt-in; ``slamhip.vis``): ONE
    launch.  ``params``: the ``VisParams``.  Returns the ``VisResult``."""
    return _vis_params(params).check_batch(scanset, src, dst, tf, params)


def choose_candidate(counts, ok, order):
    """Which candidate transform of one edge to take.  ``counts``: (C, 6)
    visibility counts, ``ok``: (C,) verdicts, ``order``: (C,) ranks (0 the ICP
    result, 1 refined from the init, 2 the init).  The passing candidate of the
    lowest rank above 0, else the smallest key ``(conflict0 + conflict1,
    -(agree0 + agree1), order)`` of them all.  Returns its position."""
    from . import vis as _vis
    order = [int(o) for o in order]
    passing = [c for c in range(len(order)) if ok[c] and order[c] > 0]
    if passing:
        return min(passing, key=lambda c: order[c])
    return min(range(len(order)), key=lambda c: _vis.candidate_key(counts[c], order[c]))


def repair_edges(scanset, src, dst, tf, inits, verify, repair="refine-from-init", repair_refine=None):
    """Checks the edges icp(pc1 = src[b], pc2 = dst[b]) -> ``tf[b]`` that were
    started from ``inits`` (``check_edges``) and, with ``repair`` =
    "refine-from-init", re-matches those that fail: ONE
    ``slamhip.plicp.refine_batch`` launch of the gated point-to-line metric from
    their inits (``repair_refine``: its ``PlicpParams``, None for the defaults),
    ONE check of the two candidates per failing edge — the refined transform
    where its status is CONVERGED or MAX_ITERS, then the init itself — and
    ``choose_candidate``.  A passing edge keeps its row bit for bit; "none" only
    flags.  Returns (transforms, the ``VisResult`` of ``tf``, source (B,) int64:
    0 ``tf``'s row, 1 refined from the init, 2 the init)."""
    _vis = _vis_params(verify)
    if repair not in EDGE_REPAIRS:
        raise ValueError(f"unknown repair {repair!r} ({' | '.join(EDGE_REPAIRS)})")
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 3, 3)
    first = _vis.check_batch(scanset, src, dst, tf, verify)
    out = tf.copy()
    source = np.zeros(len(tf), dtype=np.int64)
    bad = np.nonzero(~first.ok)[0]
    if repair == "none" or len(bad) == 0:
        return out, first, source
    from . import plicp as _plicp
    rp = repair_refine if repair_refine is not None else _plicp.PlicpParams()
    if not isinstance(rp, _plicp.PlicpParams):
        raise TypeError(f"repair_refine must be a slamhip.plicp.PlicpParams or None, got {type(rp).__name__}")
    start = np.ascontiguousarray(np.asarray(inits, dtype=np.float64).reshape(-1, 3, 3)[bad])
    rr = _plicp.refine_batch(scanset, src[bad], dst[bad], start, rp)
    usable = (rr.status == _plicp.CONVERGED) | (rr.status == _plicp.MAX_ITERS)
    nb = len(bad)
    second = _vis.check_batch(scanset, np.concatenate([src[bad], src[bad]]), np.concatenate([dst[bad], dst[bad]]),
                              np.concatenate([rr.tf, start]), verify)
    for e, b in enumerate(bad):
        cand = [(0, tf[b], first.counts[b], first.ok[b])]
        if usable[e]:
            cand.append((1, rr.tf[e], second.counts[e], second.ok[e]))
        cand.append((2, start[e], second.counts[nb + e], second.ok[nb + e]))
        c = choose_candidate([x[2] for x in cand], [x[3] for x in cand], [x[0] for x in cand])
        out[b] = cand[c][1]
        source[b] = cand[c][0]
    return out, first, source


def scan_matching(odometry, lidar_points, icp_max_iters=100, icp_epsilon=0.05, scanset=None, refine=None,
                  refine_gates=REFINE_GATES, verify=None, repair="refine-from-init", repair_refine=None):
    """Stage 1 (``scripts/main.py:236-256``) as one batched ICP launch.  With
    ``refine`` a ``slamhip.plicp.PlicpParams`` (new, opt-in) every ICP edge is
    refined with the point-to-line metric before the chain is composed; the
    default None leaves every output as it is.  With ``verify`` a
    ``slamhip.vis.VisParams`` (new, opt-in) every ICP edge is checked by scan
    visibility first and a failing one is re-matched from its odometry init
    (``repair_edges``; ``repair="none"`` only flags); ``refine`` then runs on
    the repaired transforms.  ``verify=None`` leaves every output as it is."""
    from . import icp as _icp
    if verify is not None:
        _vis_params(verify)
    if repair not in EDGE_REPAIRS:
        raise ValueError(f"unknown repair {repair!r} ({' | '.join(EDGE_REPAIRS)})")
    odometry = np.asarray(odometry, dtype=np.float64)
    S = len(odometry)
    if len(lidar_points) != S:
        raise ValueError(f"{len(lidar_points)} scans for {S} odometry poses")
    if S < 2:
        return ScanMatchResult(odometry.copy(), np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0, np.int64))
    # per pair, like the reference (scalar np.cos/np.sin: no SIMD-path rounding differences)
    inits = np.stack([se2.pose_to_mat(odometry[i] - odometry[i - 1]) for i in range(1, S)])
    ss = scanset if scanset is not None else _icp.ScanSet(lidar_points)
    batch = _icp.IcpBatch(ss, np.arange(1, S), np.arange(0, S - 1), inits,
                          epsilon=icp_epsilon, max_iters=icp_max_iters)
    batch.launch()
    r = batch.result()
    tf0, checked = r.tf, {}
    if verify is not None:
        tf0, first, source = repair_edges(ss, np.arange(1, S), np.arange(0, S - 1), r.tf, inits, verify, repair,
                                          repair_refine)
        checked = dict(verify_ok=first.ok, verify_counts=first.counts, repaired=source != 0, repair_source=source)
    if refine is not None:
        tf, taken, rr = refine_edges(ss, np.arange(1, S), np.arange(0, S - 1), tf0, refine, refine_gates)
        return ScanMatchResult(se2.compose_chain(odometry[0], tf), tf, r.err, r.iters, rr.status, rr.inliers, rr.obs,
                               taken, **checked)
    poses = se2.compose_chain(odometry[0], tf0)
    return ScanMatchResult(poses, tf0, r.err, r.iters, **checked)


@dataclass
class ClosureCheck:
    """What a loop-closure stage's ``verify`` did (its last returned value)."""
    checked: int           # candidates that passed the stage's error threshold and were checked
    rejected: int          # those of them that failed the visibility check
    ok: np.ndarray         # (B,) bool per candidate: checked and passed
    counts: np.ndarray     # (B, 6) int64 visibility counts, 0 where the candidate was not checked


def verify_closures(scanset, src, dst, tfs, passed, verify):
    """The visibility check (``slamhip.vis``) of the loop-closure candidates
    icp(pc1 = src[b], pc2 = dst[b]) -> ``tfs[b]`` that ``passed`` their stage's
    error threshold, in ONE launch.  Returns the ``ClosureCheck``."""
    _vis = _vis_params(verify)
    passed = np.asarray(passed, dtype=bool)
    idx = np.nonzero(passed)[0]
    ok = np.zeros(len(passed), dtype=bool)
    counts = np.zeros((len(passed), 6), dtype=np.int64)
    if len(idx):
        res = _vis.check_batch(scanset, np.asarray(src, dtype=np.int64)[idx], np.asarray(dst, dtype=np.int64)[idx],
                               np.ascontiguousarray(np.asarray(tfs, dtype=np.float64)[idx]), verify)
        ok[idx] = res.ok
        counts[idx] = res.counts
    return ClosureCheck(len(idx), int(len(idx) - ok.sum()), ok, counts)


def read_manual_loop_closures(fname):
    """``np.loadtxt(fname, dtype=int)`` rows (i, j) as ``scripts/main.py:300``
    reads them (a single row is accepted too)."""
    m = np.loadtxt(fname, dtype=int)
    return np.atleast_2d(m).reshape(-1, 2)


LOOP_CLOSURE_INITS = ("identity", "csm")


def check_loop_closure_init(init):
    if init not in LOOP_CLOSURE_INITS:
        raise ValueError(f"unknown loop-closure init {init!r} ({' | '.join(LOOP_CLOSURE_INITS)})")


def loop_closure_inits(scanset, src, dst, init="identity", csm=None):
    """(B, 3, 3) initial transforms of the loop-closure ICP launch
    icp(pc1 = src[b], pc2 = dst[b]): ``"identity"`` (the reference's
    ``np.eye(3)``, the default) or ``"csm"`` — the batched correlative scan
    match of the same pairs (``slamhip.csm.csm_batch``; ``csm``: its
    ``CsmParams``, None for the defaults), for loops closed at another heading."""
    check_loop_closure_init(init)
    if init == "identity":
        return np.broadcast_to(np.eye(3), (len(src), 3, 3))
    from . import csm as _csm
    return _csm.csm_batch(scanset, src, dst, params=csm if csm is not None else _csm.CsmParams()).tf


def manual_loop_closures(pg, lidar_points, matches, max_iters=100, epsilon=0.05,
                         err_thresh=LOOP_CLOSURE_ICP_ERROR, scanset=None, init="identity", csm=None, refine=None,
                         refine_gates=REFINE_GATES, verify=None):
    """Stage 2, manual path (``scripts/main.py:298-307``): ICP(pc_i, pc_j,
    init = I) for every annotated pair in ONE launch; constraints are added
    in file order (``add_constraint`` overwrites a repeated (i, j) in place,
    networkx semantics), exactly as the reference's serial loop does.
    ``init="csm"`` (new, opt-in) starts every ICP from the correlative scan
    match of its pair instead of the identity (``loop_closure_inits``).
    ``refine`` (a ``slamhip.plicp.PlicpParams``; new, opt-in): acceptance stays
    the rule above on the point-to-point error, and an accepted constraint
    carries the point-to-line refinement of its transform where
    ``apply_refinement`` allows it (``refine_edges``).
    ``verify`` (a ``slamhip.vis.VisParams``; new, opt-in): a match below the
    error threshold is added only if the transform that would be added (after
    ``refine``) also passes the visibility check (``verify_closures``).
    Returns the boolean mask of accepted matches; with ``verify`` the mask and
    the ``ClosureCheck``, which says how many the check rejected."""
    from . import icp as _icp
    check_loop_closure_init(init)
    if verify is not None:
        _vis_params(verify)
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    if len(matches) == 0:
        none = np.zeros(0, dtype=bool)
        return none if verify is None else (none, ClosureCheck(0, 0, none.copy(), np.zeros((0, 6), np.int64)))
    ss = scanset if scanset is not None else _icp.ScanSet(lidar_points)
    inits = loop_closure_inits(ss, matches[:, 0], matches[:, 1], init, csm)
    batch = _icp.IcpBatch(ss, matches[:, 0], matches[:, 1], inits, epsilon=epsilon, max_iters=max_iters)
    batch.launch()
    r = batch.result()
    ok = r.err < err_thresh
    tfs = _edge_transforms(ss, matches[:, 0], matches[:, 1], r.tf, refine, refine_gates)
    report = None
    if verify is not None:
        report = verify_closures(ss, matches[:, 0], matches[:, 1], tfs, ok, verify)
        ok = ok & report.ok
    for (i, j), t, good in zip(matches, tfs, ok):
        if good:
            add_loop_constraint(pg, int(i), int(j), t.copy(), "icp")   # icp(pc_i, pc_j): X_i = X_j T
    return ok if verify is None else (ok, report)


def proximity_loop_closures(pg, lidar_points, min_dist_along_path=2, max_dist=1, err_thresh=110, max_iters=100,
                            epsilon=0.05, scanset=None, init="identity", csm=None, refine=None,
                            refine_gates=REFINE_GATES, verify=None):
    """Stage 2 without annotations: the reference's ``detect_proximity``
    (``src/loop_closure_detection.py:11-39``) on resident data.  The candidate
    pairs come from the GPU search of ``slamhip.lcd`` (the nearest pose at
    least ``min_dist_along_path`` further along the path, within ``max_dist``;
    O(N) memory), every candidate's icp(pc_j, pc_i) runs in ONE launch over
    the resident ``scanset`` by index (no second upload of the scans), and the
    reference's greedy pass is replayed on the results: reverse order, each
    node used once, ``error < err_thresh``, the constraint in the "relative"
    convention.  ``init="csm"`` starts every ICP from the correlative scan
    match of its pair.  ``refine`` and ``verify``: as in
    ``manual_loop_closures``; the greedy pass sees only the candidates that
    pass the check.  Returns the candidates, a list of (i, j) in the order the
    pass visits them, and the boolean mask of those accepted; with ``verify``
    also the ``ClosureCheck``."""
    from . import icp as _icp
    from . import lcd as _lcd
    check_loop_closure_init(init)
    if verify is not None:
        _vis_params(verify)
    cand = _lcd.proximity_candidates_device(pg.poses, min_dist_along_path, max_dist)
    accepted = np.zeros(len(cand), dtype=bool)
    if not cand:
        return (cand, accepted) if verify is None else \
            (cand, accepted, ClosureCheck(0, 0, accepted.copy(), np.zeros((0, 6), np.int64)))
    pairs = np.asarray(cand, dtype=np.int64)
    ss = scanset if scanset is not None else _icp.ScanSet(lidar_points)
    src, dst = pairs[:, 1], pairs[:, 0]   # icp(pc_j, pc_i), reference :33-35
    batch = _icp.IcpBatch(ss, src, dst, loop_closure_inits(ss, src, dst, init, csm), epsilon=epsilon,
                          max_iters=max_iters)
    batch.launch()
    r = batch.result()
    tfs = _edge_transforms(ss, src, dst, r.tf, refine, refine_gates)
    report = None if verify is None else verify_closures(ss, src, dst, tfs, r.err < err_thresh, verify)
    used = set()
    for b, (i, j) in enumerate(cand):
        if i in used or j in used:
            continue
        if float(r.err[b]) < err_thresh and (report is None or report.ok[b]):
            add_loop_constraint(pg, i, j, tfs[b].copy(), "relative")   # X_j = X_i T (src/pose_graph.py)
            used.update((i, j))
            accepted[b] = True
    return (cand, accepted) if verify is None else (cand, accepted, report)


SIGNATURE_LOOP_CLOSURE_INITS = LOOP_CLOSURE_INITS + ("signature",)


def signature_loop_closures(pg, lidar_points, min_dist_along_path=5, max_frac=(1, 4), err_thresh=110, max_iters=100,
                            epsilon=0.05, scanset=None, init="signature", csm=None, params=None, refine=None,
                            refine_gates=REFINE_GATES, verify=None):
    """Stage 2 from the scans alone (new; the reference has no counterpart):
    the shape of ``proximity_loop_closures`` with the candidates of
    ``slamhip.sig`` — for every scan i the scan j, at least
    ``min_dist_along_path`` further along the path, whose rotation-invariant
    signature is closest, kept when ``d_ij <= max_frac (n_i + n_j)``.  The
    poses only exclude the recent path, so a loop that drift has opened wide is
    proposed all the same.  Every candidate's icp(pc_j, pc_i) runs in ONE launch
    over the resident ``scanset``, then the same greedy pass and the "relative"
    convention.  ``init="signature"`` (the default here, and only here) starts
    every ICP from the pure rotation by -2 pi k_ij / S of the best shift;
    ``"identity"`` and ``"csm"`` as elsewhere.  ``params``: the
    ``slamhip.sig.SigParams``.  For revisits in the direction of travel (at any
    rotation of the scan frame): see ``slamhip.sig``.  ``refine`` and
    ``verify``: as in ``proximity_loop_closures``.  Returns the candidates, a
    list of (i, j, k) in the order the pass visits them, and the boolean mask
    of those accepted; with ``verify`` also the ``ClosureCheck``."""
    from . import icp as _icp
    from . import sig as _sig
    if init not in SIGNATURE_LOOP_CLOSURE_INITS:
        raise ValueError(f"unknown loop-closure init {init!r} ({' | '.join(SIGNATURE_LOOP_CLOSURE_INITS)})")
    if verify is not None:
        _vis_params(verify)
    params = params if params is not None else _sig.SigParams()
    ss = scanset if scanset is not None else _icp.ScanSet(lidar_points)
    cand = _sig.signature_candidates_device(ss, pg.poses, min_dist_along_path, params, max_frac)
    accepted = np.zeros(len(cand), dtype=bool)
    if not cand:
        return (cand, accepted) if verify is None else \
            (cand, accepted, ClosureCheck(0, 0, accepted.copy(), np.zeros((0, 6), np.int64)))
    triples = np.asarray(cand, dtype=np.int64)
    src, dst = triples[:, 1], triples[:, 0]   # icp(pc_j, pc_i), as the proximity stage
    inits = _sig.shift_inits(triples[:, 2], params.sectors) if init == "signature" else \
        loop_closure_inits(ss, src, dst, init, csm)
    batch = _icp.IcpBatch(ss, src, dst, inits, epsilon=epsilon, max_iters=max_iters)
    batch.launch()
    r = batch.result()
    tfs = _edge_transforms(ss, src, dst, r.tf, refine, refine_gates)
    report = None if verify is None else verify_closures(ss, src, dst, tfs, r.err < err_thresh, verify)
    used = set()
    for b, (i, j, _) in enumerate(cand):
        if i in used or j in used:
            continue
        if float(r.err[b]) < err_thresh and (report is None or report.ok[b]):
            add_loop_constraint(pg, i, j, tfs[b].copy(), "relative")   # X_j = X_i T (src/pose_graph.py)
            used.update((i, j))
            accepted[b] = True
    return (cand, accepted) if verify is None else (cand, accepted, report)


def image_stage(pg, lidar_points, descriptors, image_rate=1, min_dist_along_path=5, image_err_thresh=125,
                n_matches=10, icp_err_thresh=30, metric="hamming", scanset=None, init="identity", csm=None,
                refine=None, refine_gates=REFINE_GATES, verify=None):
    """``image_loop_closures`` with everything it computed: ``(good, accepted,
    dist_mat, icp_result)`` (``icp_result`` None without a selected pair; it is
    the point-to-point result with ``refine`` too); with ``verify`` also the
    ``ClosureCheck``."""
    from . import desc as _desc
    from . import icp as _icp
    check_loop_closure_init(init)
    if verify is not None:
        _vis_params(verify)
    ds = descriptors if isinstance(descriptors, _desc.DescriptorSet) else _desc.DescriptorSet(descriptors)
    start = _desc.image_starts(pg.poses, min_dist_along_path, image_rate)
    if len(start) != len(ds):
        raise ValueError(f"{len(ds)} images for {len(pg.poses)} poses at image_rate {image_rate}: "
                         f"expected {len(start)}")
    dist_mat = _desc.similarity_matrix(ds, start, n_matches, metric)
    good = _desc.select_matches(dist_mat, image_err_thresh)
    accepted = np.zeros(len(good), dtype=bool)
    if not good:
        return (good, accepted, dist_mat, None) if verify is None else \
            (good, accepted, dist_mat, None, ClosureCheck(0, 0, accepted.copy(), np.zeros((0, 6), np.int64)))
    pairs = np.asarray(good, dtype=np.int64) * int(image_rate)
    ss = scanset if scanset is not None else _icp.ScanSet(lidar_points)
    src, dst = pairs[:, 0], pairs[:, 1]   # icp(pc_i, pc_j), reference :136-142
    batch = _icp.IcpBatch(ss, src, dst, loop_closure_inits(ss, src, dst, init, csm), epsilon=0.05, max_iters=100)
    batch.launch()
    r = batch.result()
    accepted[:] = r.err < icp_err_thresh
    tfs = _edge_transforms(ss, src, dst, r.tf, refine, refine_gates)
    report = None
    if verify is not None:
        report = verify_closures(ss, src, dst, tfs, accepted, verify)
        accepted &= report.ok
    for (i, j), t, ok in zip(pairs, tfs, accepted):
        if ok:
            add_loop_constraint(pg, int(i), int(j), t.copy(), "icp")   # icp(pc_i, pc_j): X_i = X_j T
    return (good, accepted, dist_mat, r) if verify is None else (good, accepted, dist_mat, r, report)


def image_loop_closures(pg, lidar_points, descriptors, image_rate=1, min_dist_along_path=5,
                        image_err_thresh=125, n_matches=10, icp_err_thresh=30,
                        metric="hamming", scanset=None, init="identity", csm=None, refine=None,
                        refine_gates=REFINE_GATES, verify=None):
    """Stage 2 from image descriptors: the reference's
    ``detect_images_direct_similarity`` (``src/loop_closure_detection.py:84-159``)
    after the keypoints.  ``descriptors``: one (n, 32) uint8 array per image
    (image m belongs to scan m * ``image_rate``), or a resident
    ``slamhip.desc.DescriptorSet``.  The starts (:84-91), every image pair
    (i, j >= start[i]) matched on the GPU in one launch (``slamhip.desc``;
    ``metric`` "hamming" is the reference's ``approximate_match=False``, "l2"
    the exact search its default approximates), the column rule (:126-131),
    icp(pc_i, pc_j) of every selected pair in ONE launch over the resident
    ``scanset``, and the constraint where ``err < icp_err_thresh``, in the "icp"
    convention.  ``refine`` and ``verify``: as in ``manual_loop_closures``.
    Returns the selected (i, j) image pairs and the boolean mask of those
    accepted; with ``verify`` also the ``ClosureCheck``."""
    out = image_stage(pg, lidar_points, descriptors, image_rate, min_dist_along_path, image_err_thresh, n_matches,
                      icp_err_thresh, metric, scanset, init, csm, refine, refine_gates, verify)
    return out[:2] if verify is None else out[:2] + out[4:]


def add_loop_constraint(pg, i, j, T, convention):
    """``pg.add_constraint(i, j, T)`` recording the measurement convention
    (src/pose_graph.py) when the graph type supports it — the reference's
    own PoseGraph (or any duck-typed graph) gets the plain call."""
    try:
        pg.add_constraint(i, j, T, convention=convention)
    except TypeError:
        pg.add_constraint(i, j, T)


def verify_loop_closures(pg, params=None, remove=True, details=False):
    """Checks the loop closures of ``pg`` against each other (new, opt-in;
    ``slamhip.pcm``: pairwise consistency over the chain ``pg.poses`` as they
    stand, that is before optimisation) and removes the rejected edges
    (``pg.remove_constraint``) unless ``remove`` is false.  The closures are
    the edges added by ``add_constraint`` that carry a convention, in networkx
    order; an "icp" edge (i, j, T), X_i = X_j T, is checked as (a = j, b = i,
    Z = T).  ``params``: the ``slamhip.pcm.PcmParams``.  Returns the edges as a
    list of (i, j, T), the boolean mask of those kept, and the number of
    constraint edges without a convention, which stay in place unverified;
    with ``details`` also the ``slamhip.pcm.PcmResult`` (None without a closure)."""
    from . import pcm as _pcm
    _, conv, added = pg.edge_kinds()
    edges, a, b = [], [], []
    for (i, j, T), c in zip(pg.graph.edges(data="object"), conv):
        if c == 1:      # "icp"
            a.append(j)
            b.append(i)
        elif c == 2:    # "relative"
            a.append(i)
            b.append(j)
        else:
            continue
        edges.append((i, j, T))
    unverified = int((added & (conv == 0)).sum())
    res, keep = None, np.zeros(0, dtype=bool)
    if edges:
        res = _pcm.consistency(pg.poses, a, b, np.stack([T for _, _, T in edges]), params)
        keep = res.keep
    if remove:
        for (i, j, _), ok in zip(edges, keep):
            if not ok:
                pg.remove_constraint(i, j)
    return (edges, keep, unverified, res) if details else (edges, keep, unverified)


def optimize(pg, lidar_points, optimization_max_iters=50, icp_max_iters=100, icp_epsilon=0.05,
             icp_recompute=False, method="sgd", gn_iterations=10, gn_loss=None, gn_loss_scale=1.0,
             gn_robust_edges="loops", gn_drop_below=None, report=None):
    """Stage 3 (``scripts/main.py:322-334``): SGD steps with learning rate
    1/(k+1) on device-resident poses, then the orientation recompute; or, with
    ``method="gn"``, the Gauss-Newton solve followed by the same recompute.
    Updates ``pg.poses`` in place.

    ``gn_loss`` (new, opt-in; ``method="gn"`` only) runs the robust solve
    (``optimize_pose_graph(loss=...)``; ``gn_loss_scale`` in units of
    sqrt(information) x metres).  With ``gn_drop_below`` = R the loop
    closures (edges with |b - a| != 1) whose final ratio is below R are then
    removed from the graph (``pg.remove_constraint``, as
    ``verify_loop_closures(remove=True)`` removes edges) and the plain
    iterations run once more on what is left; the removed (a, b) pairs go to
    ``report["gn_dropped"]`` when a dict is given."""
    import src.pose_graph_optimization as pgo_drop_in
    if gn_loss in (None, "none"):
        gn_loss = None
    if method != "gn" and (gn_loss is not None or gn_drop_below is not None):
        raise ValueError("gn_loss / gn_drop_below need method='gn'")
    if gn_drop_below is not None and gn_loss is None:
        raise ValueError("gn_drop_below needs a gn_loss")
    if method == "sgd":
        from . import pgo as _pgo
        ea, eb, tf = pg.edge_arrays()
        solver = _pgo.SgdSolver(pg.poses, ea, eb, tf)
        for k in range(optimization_max_iters):
            solver.step(1.0 / float(k + 1))
        pg.poses[...] = solver.host_poses()
    elif method == "gn" and gn_loss is not None:
        _, wts = pgo_drop_in.optimize_pose_graph(pg, iterations=gn_iterations, loss=gn_loss, loss_scale=gn_loss_scale,
                                                 robust_edges=gn_robust_edges, return_weights=True)
        if gn_drop_below is not None:
            loops = np.abs(wts["eb"].astype(np.int64) - wts["ea"]) != 1
            drop = np.flatnonzero(loops & wts["robust"] & (wts["ratio"] < gn_drop_below))
            pairs = [(int(wts["ea"][e]), int(wts["eb"][e])) for e in drop]
            for a, b in pairs:
                pg.remove_constraint(a, b)
            if report is not None:
                report["gn_dropped"] = pairs
            pgo_drop_in.optimize_pose_graph(pg, iterations=gn_iterations)
    elif method == "gn":
        pgo_drop_in.optimize_pose_graph(pg, iterations=gn_iterations)
    else:
        raise ValueError(f"unknown optimiser {method!r} (sgd | gn)")
    pgo_drop_in.recompute_pose_graph_orientation(pg, lidar_points, icp_max_iters, icp_epsilon, -1,
                                                 icp_recompute=icp_recompute)
    return pg
