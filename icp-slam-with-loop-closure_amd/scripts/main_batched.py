#!/usr/bin/env python3
"""Batched GPU driver with the command line of the reference's scripts/main.py.

Runs the reference's program flow (``scripts/main.py:66-181`` flags,
``:230-339`` stages) with every ICP stage as one batched MI355X launch:

  scan_matching  ->  loop_closure (manual annotations)  ->  optimization

and writes the same artefacts under ``--results-dir``:
``icp_pose_graph.{pickle,g2o}`` (or ``odometry_pose_graph.*`` with
``--skip-icp``), ``loop_closure_pose_graph.*``, ``optim.*``, and the occupancy
grids of src/visualization.py:74-98 (``<name>_og.png``, ``<name>.map`` with
``--save-map-files``; names odometry / icp / final) built on the GPU.

Inputs: ``dataset`` is an ``.npz`` scan stream (slamhip.dataset.save) or a
generator spec ``synthetic:<walk|loop>:<n_scans>[:<seed>]``; for ``loop``
datasets ``--manual-loop-closures auto`` uses the generator's ground-truth
loop pairs.  ``--loop-closure-init csm`` (new, opt-in) starts every
loop-closure ICP from the batched correlative scan match of its pair
(slamhip.csm) instead of the reference's identity; ``--csm-window-m``,
``--csm-angle-window-deg`` and ``--csm-angle-step-deg`` size its search.
``--loop-closure-detection proximity`` (new, opt-in; used when no manual file
is given) finds the loop closures itself: the reference's ``detect_proximity``
with the candidate search on the GPU (slamhip.lcd) and the candidates' ICP on
the resident scans; ``--proximity-min-dist-along-path``, ``--proximity-max-dist``
and ``--proximity-icp-error`` default to the reference's 2 / 1 / 110.
``--loop-closure-detection descriptors`` (new, opt-in) is the reference's image
detector from the ORB descriptors on: ``--descriptors FILE.npz`` (arrays
``desc`` uint8 (D, 32) and ``off`` int64 (M + 1); image m belongs to scan
m * ``--image-downsample``), or ``--descriptors auto`` for a synthetic loop
dataset (slamhip.synthetic.make_descriptors); every image pair is matched on
the GPU (slamhip.desc, ``--descriptor-metric hamming|l2``), then the
reference's selection and one ICP launch.  ``--image-match-error``,
``--keypoint-n-matches``, ``--image-downsample`` and ``--min-dist-along-path``
feed it (scripts/main.py's defaults 2500 / 20 / 1 / 5 when unset) and
``--loop-closure-icp-error`` is its ICP threshold.
``--loop-closure-detection signatures`` (new, opt-in; no counterpart in the
reference) proposes the loop closures from the scans alone: rotation-invariant
scan signatures matched on the GPU (slamhip.sig), the poses only excluding the
recent path; ``--signature-sectors``, ``--signature-ring-width``,
``--signature-min-dist-along-path``, ``--signature-max-frac NUM/DEN``,
``--signature-icp-error`` and ``--signature-init signature|identity|csm``
(default: the rotation the match found) feed it.
``--loop-closure-consistency`` (new, opt-in) checks the loop closures against
each other at the end of the stage and removes those outside the pairwise
consistent set (slamhip.pcm); ``--consistency-trans-tol``,
``--consistency-rot-tol``, ``--consistency-trans-drift`` and
``--consistency-rot-drift`` are its tolerances.
``--edge-check visibility`` (new, opt-in) verifies every ICP edge on its own by
scan visibility (slamhip.vis): a scan-matching edge that fails is re-matched
from its odometry init (``--scan-matching-repair refine-from-init``, the
default, or ``none`` to flag only), and a loop closure below its error
threshold is added only if it passes too; ``--edge-check-margin``,
``--edge-check-sectors``, ``--edge-check-max-conflict`` and
``--edge-check-min-agree`` feed it, and the printed summary counts the edges
flagged, repaired and rejected.
``--save-map FILE`` (new, opt-in) writes the last occupancy grid built, with its
origin and cell width, as one ``.npz`` (slamhip.loc.save_map) that
scripts/localize.py reads; ``--map-check`` (new, opt-in) scores every scan at
the pose the grid was built from against that grid (slamhip.loc.score_poses)
and writes ``<name>_map_check.npz`` into the results directory.
Out of scope here (flags accepted, ignored): ORB keypoint extraction from
images (OpenCV) and the matplotlib figures.

    python icp-slam-with-loop-closure_amd/scripts/main_batched.py synthetic:loop:2000:3 \\
        --manual-loop-closures auto --results-dir /tmp/results
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

STAGES = ["scan_matching", "loop_closure", "optimization"]


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("dataset")
    p.add_argument("--program-start", default="scan_matching", choices=STAGES)
    p.add_argument("--program-end", default="optimization", choices=STAGES)
    p.add_argument("--skip-icp", action="store_true")
    p.add_argument("--icp-max-iters", default=100, type=int)
    p.add_argument("--icp-epsilon", default=0.05, type=float)
    p.add_argument("--pose-graph")
    p.add_argument("--n-jobs", default=-1, type=int, help="accepted; the GPU path needs no host pool")
    p.add_argument("--dataset-start", default=0, type=int)
    p.add_argument("--dataset-end", type=int)
    p.add_argument("--optimization-max-iters", default=50, type=int)
    p.add_argument("--manual-loop-closures",
                   help="text file of (i, j) rows, or 'auto' for a synthetic loop dataset's ground truth")
    p.add_argument("--loop-closure-icp-error", default=30, type=float,
                   help="descriptors: a selected pair is accepted below this ICP error; the manual path uses the "
                        "reference's fixed 30")
    p.add_argument("--loop-closure-init", default="identity", choices=["identity", "csm"],
                   help="identity = the reference's ICP start (default); csm = correlative scan match of every pair")
    p.add_argument("--loop-closure-detection", default="none",
                   choices=["none", "proximity", "descriptors", "signatures"],
                   help="without --manual-loop-closures: none (default), proximity = the reference's "
                        "detect_proximity with the candidate search on the GPU, descriptors = its image "
                        "detector from the ORB descriptors on, matched on the GPU, or signatures = candidates "
                        "from the scans' rotation-invariant signatures, matched on the GPU")
    p.add_argument("--signature-sectors", default=64, type=int,
                   help="signatures: angular sectors, a multiple of 8 in 8..128")
    p.add_argument("--signature-ring-width", default=0.4, type=float, help="signatures: width of the 32 rings (m)")
    p.add_argument("--signature-min-dist-along-path", default=5, type=float,
                   help="signatures: least path length between the two scans of a candidate (m)")
    p.add_argument("--signature-max-frac", default="1/4",
                   help="signatures: NUM/DEN, a candidate differs in at most that share of the two scans' cells")
    p.add_argument("--signature-icp-error", default=110, type=float,
                   help="signatures: a candidate is accepted below this ICP error")
    p.add_argument("--signature-init", default="signature", choices=["signature", "identity", "csm"],
                   help="signatures: ICP start: the rotation the match found (default), identity or csm")
    p.add_argument("--loop-closure-consistency", action="store_true",
                   help="check the loop closures against each other at the end of the loop-closure stage and remove "
                        "those outside the pairwise consistent set (slamhip.pcm)")
    p.add_argument("--consistency-trans-tol", default=None, type=float,
                   help="consistency: floor of a cycle's translation (m)")
    p.add_argument("--consistency-rot-tol", default=None, type=float,
                   help="consistency: floor of the chord of a cycle's rotation")
    p.add_argument("--consistency-trans-drift", default=None, type=float,
                   help="consistency: translation drift per square root of a chain step (m)")
    p.add_argument("--consistency-rot-drift", default=None, type=float,
                   help="consistency: rotation drift (chord) per square root of a chain step")
    p.add_argument("--icp-refine", default="none", choices=["none", "point-to-line"],
                   help="refine every ICP edge (scan matching and accepted loop closures) with the gated "
                        "point-to-line metric of slamhip.plicp (new, opt-in; default: none)")
    p.add_argument("--refine-max-dist", default=0.5, type=float, help="refinement: the correspondence gate (m)")
    p.add_argument("--refine-min-overlap", default=0.5, type=float,
                   help="refinement: an edge keeps its point-to-point transform below this share of inliers")
    p.add_argument("--refine-min-observability", default=0.0, type=float,
                   help="refinement: ... and below this observability of the translation (0: off)")
    p.add_argument("--edge-check", default="none", choices=["none", "visibility"],
                   help="verify every ICP edge (scan matching and loop closures below their error threshold) by scan "
                        "visibility (slamhip.vis; new, opt-in; default: none)")
    p.add_argument("--edge-check-margin", default=0.15, type=float,
                   help="edge check: a range within this of the other scan's agrees, one shorter by more conflicts (m)")
    p.add_argument("--edge-check-sectors", default=360, type=int, help="edge check: bearings of a scan's range table")
    p.add_argument("--edge-check-max-conflict", default=0.02, type=float,
                   help="edge check: largest share of conflicting points among those that agree or conflict")
    p.add_argument("--edge-check-min-agree", default=0.25, type=float,
                   help="edge check: least share of a scan's points that agree")
    p.add_argument("--scan-matching-repair", default="refine-from-init", choices=["none", "refine-from-init"],
                   help="edge check: re-match a failing scan-matching edge from its odometry init with the gated "
                        "point-to-line metric (default), or only flag it")
    p.add_argument("--descriptors", help="descriptors: an .npz with desc (D, 32) uint8 and off (M + 1) int64, or "
                                         "'auto' for a synthetic loop dataset")
    p.add_argument("--descriptor-metric", default="hamming", choices=["hamming", "l2"],
                   help="descriptors: hamming = cross-checked brute force (default), l2 = the exact search the "
                        "reference's FLANN matcher approximates")
    p.add_argument("--proximity-min-dist-along-path", default=2, type=float,
                   help="proximity: least path length between the two poses of a candidate (m)")
    p.add_argument("--proximity-max-dist", default=1, type=float,
                   help="proximity: largest distance between the two poses of a candidate (m)")
    p.add_argument("--proximity-icp-error", default=110, type=float,
                   help="proximity: a candidate is accepted below this ICP error")
    p.add_argument("--csm-window-m", default=1.5, type=float,
                   help="csm: half-width of the shift search (m), in cells of 0.05 m")
    p.add_argument("--csm-angle-window-deg", default=180.0, type=float, help="csm: half-width of the angle search")
    p.add_argument("--csm-angle-step-deg", default=1.5, type=float, help="csm: angle bin spacing")
    p.add_argument("--icp-recompute", action="store_true")
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "gn"],
                   help="sgd = the reference's relaxation (default); gn = Gauss-Newton")
    p.add_argument("--gn-iterations", default=10, type=int)
    p.add_argument("--gn-loss", default="none", choices=["none", "huber", "cauchy", "gm", "dcs", "gnc-gm"],
                   help="gn: robust loss on the loop closures by per-edge reweighting on the GPU (slamhip.robust; "
                        "new, opt-in; none = the plain solve)")
    p.add_argument("--gn-loss-scale", default=1.0, type=float,
                   help="gn loss: its scale c, in units of sqrt(information) x metres, NOT a chi-square quantile (the "
                        "informations 2 I / 5 I are not covariances); with information 5, 0.3 turns gm / dcs at a "
                        "residual of about 0.13 m")
    p.add_argument("--gn-drop-below", default=None, type=float, metavar="R",
                   help="gn loss: after the robust solve remove the loop closures whose final weight ratio is below "
                        "R (0.5 is a usual choice), then run the plain iterations once more")
    p.add_argument("--results-dir", default="results")
    p.add_argument("--cell-width", default=0.1, type=float)
    p.add_argument("--hit-odds", default=5, type=int)
    p.add_argument("--miss-odds", default=2, type=int)
    for f in ("--produce-odometry-map", "--skip-occupancy-grid", "--save-map-files", "--occupancy-grid-mle"):
        p.add_argument(f, action="store_true")
    p.add_argument("--save-map", metavar="FILE",
                   help="write the last occupancy grid built, its origin and cell width as one .npz for "
                        "scripts/localize.py (slamhip.loc; new, opt-in)")
    p.add_argument("--map-check", action="store_true",
                   help="score every scan at its pose against the grid built from those poses and write "
                        "<name>_map_check.npz into the results directory (slamhip.loc.score_poses; new, opt-in)")
    p.add_argument("--map-check-d-cap", default=20, type=int, help="map check: cap of the distance field (cells)")
    # reference flags for figures (accepted, not used here) and image matching (--loop-closure-detection descriptors)
    for f, kw in (("--figure-dpi", dict(type=int)), ("--figure-width", dict(type=float)),
                  ("--figure-height", dict(type=float)), ("--image-downsample", dict(type=int)),
                  ("--image-match-error", dict(type=float)), ("--keypoint-n-matches", dict(type=int)),
                  ("--image-pointcloud-downsample", dict(type=int)), ("--min-dist-along-path", dict(type=int))):
        p.add_argument(f, **kw)
    for f in ("--save-icp-images", "--no-save-matches", "--no-save-dist-mat"):
        p.add_argument(f, action="store_true")
    a = p.parse_args(argv)
    if STAGES.index(a.program_end) < STAGES.index(a.program_start):
        p.error("--program-end precedes --program-start")
    if a.gn_loss != "none" and a.optimizer != "gn":
        p.error("--gn-loss needs --optimizer gn")
    if a.gn_drop_below is not None and a.gn_loss == "none":
        p.error("--gn-drop-below needs a --gn-loss")
    if not a.gn_loss_scale > 0:
        p.error("--gn-loss-scale must be positive")
    if (a.save_map or a.map_check) and a.skip_occupancy_grid:
        p.error("--save-map / --map-check need the occupancy grid (drop --skip-occupancy-grid)")
    if not 1 <= a.map_check_d_cap <= 255:
        p.error("--map-check-d-cap in 1..255 expected")
    if a.program_start != "scan_matching" and not a.pose_graph:
        p.error("starting after scan matching needs --pose-graph")
    if a.loop_closure_detection == "descriptors" and not a.descriptors:
        p.error("--loop-closure-detection descriptors needs --descriptors FILE.npz (or auto)")
    try:
        num, den = (int(v) for v in a.signature_max_frac.split("/"))
        if not 0 <= num <= den or den < 1:
            raise ValueError
        a.signature_max_frac = (num, den)
    except ValueError:
        p.error("--signature-max-frac NUM/DEN with integers 0 <= NUM <= DEN, DEN >= 1 expected")
    if any(v is not None and not v >= 0 for v in (a.consistency_trans_tol, a.consistency_rot_tol,
                                                  a.consistency_trans_drift, a.consistency_rot_drift)):
        p.error("--consistency-* tolerances >= 0 expected")
    if not (np.isfinite(a.refine_max_dist) and a.refine_max_dist >= 0 and 0 <= a.refine_min_overlap <= 1
            and 0 <= a.refine_min_observability <= 1):
        p.error("--refine-max-dist >= 0 and --refine-min-overlap, --refine-min-observability in [0, 1] expected")
    try:
        edge_check_params(a)
    except ValueError as e:
        p.error(f"--edge-check-*: {e}")
    if not (8 <= a.signature_sectors <= 128 and a.signature_sectors % 8 == 0 and a.signature_ring_width > 0):
        p.error("--signature-sectors a multiple of 8 in 8..128 and --signature-ring-width > 0 expected")
    if not (a.csm_window_m >= 0 and 0 < a.csm_angle_step_deg and 0 <= a.csm_angle_window_deg <= 180):
        p.error("--csm-window-m >= 0, --csm-angle-step-deg > 0 and 0 <= --csm-angle-window-deg <= 180 expected")
    return a


def consistency_params(a):
    """PcmParams of the --consistency-* flags, its defaults where unset."""
    from slamhip.pcm import PcmParams
    flags = dict(trans_tol=a.consistency_trans_tol, rot_tol=a.consistency_rot_tol,
                 trans_drift=a.consistency_trans_drift, rot_drift=a.consistency_rot_drift)
    return PcmParams(**{k: v for k, v in flags.items() if v is not None})


def refine_params(a):
    """(PlicpParams, gates) of the --icp-refine / --refine-* flags as the keywords
    of the pipeline's stages; empty without a refinement."""
    if a.icp_refine == "none":
        return {}
    from slamhip.plicp import PlicpParams
    return {"refine": PlicpParams(max_dist=a.refine_max_dist),
            "refine_gates": (a.refine_min_overlap, a.refine_min_observability)}


def edge_check_params(a):
    """The VisParams of the --edge-check-* flags as the ``verify`` keyword of the
    pipeline's stages; empty without a check."""
    from slamhip.vis import VisParams
    params = VisParams(sectors=a.edge_check_sectors, margin=a.edge_check_margin, min_agree=a.edge_check_min_agree,
                       max_conflict=a.edge_check_max_conflict)
    return {} if a.edge_check == "none" else {"verify": params}


def closure_check(stage_out, report_entry, a):
    """Splits a loop-closure stage's return value into its usual values and,
    with --edge-check, the check's counts for the printed summary."""
    if a.edge_check == "none":
        return stage_out
    *usual, check = stage_out
    report_entry["edge_check"] = {"method": a.edge_check, "checked": check.checked, "rejected": check.rejected}
    return usual[0] if len(usual) == 1 else tuple(usual)


def csm_params(a):
    """CsmParams of the --csm-* flags: a (2 w + 1)^2 window of 0.05 m cells, angle
    bins of the given step over +-window (the defaults give CsmParams())."""
    from slamhip.csm import CsmParams
    res = CsmParams().res
    side = 2 * int(round(a.csm_window_m / res)) + 1
    n_theta = max(1, int(round(2 * a.csm_angle_window_deg / a.csm_angle_step_deg)))
    return CsmParams(res=res, n_theta=n_theta, d_theta=2 * np.pi / (360.0 / a.csm_angle_step_deg), nx=side, ny=side)


IMAGE_DEFAULTS = dict(image_match_error=2500.0, keypoint_n_matches=20, image_downsample=1, min_dist_along_path=5)


def image_params(a):
    """The four image-matching flags, scripts/main.py's defaults where unset."""
    return {k: (getattr(a, k) if getattr(a, k) is not None else v) for k, v in IMAGE_DEFAULTS.items()}


def load_descriptors(a, n_scans, image_rate):
    """One (n, 32) uint8 array per image: image m of scan m * image_rate of the
    (sliced) dataset."""
    if a.descriptors == "auto":
        from slamhip import synthetic
        parts = a.dataset.split(":")
        if len(parts) < 3 or parts[:2] != ["synthetic", "loop"]:
            raise SystemExit("--descriptors auto needs a synthetic:loop dataset")
        seed = int(parts[3]) if len(parts) > 3 else 0
        seq = synthetic.make_loop_sequence(int(parts[2]), seed=seed, n_beams=3)   # the lap layout only
        per_scan = synthetic.make_descriptors(seq, seed)
        return per_scan[a.dataset_start:a.dataset_start + n_scans][::image_rate]
    with np.load(a.descriptors, allow_pickle=False) as z:
        desc, off = z["desc"], z["off"]
    return [desc[off[m]:off[m + 1]] for m in range(len(off) - 1)]


def save_map(a, poses, scans, name, report):
    """src/visualization.py:83-98 without the figures: the occupancy grid of
    `poses` (GPU), optionally its MLE, saved as <name>_og.png (+ <name>.map)."""
    if a.skip_occupancy_grid:
        return
    import src.produce_occupancy_grid as pog
    t0 = time.perf_counter()
    og, (min_x, min_y) = pog.produce_occupancy_grid(np.asarray(poses), scans, a.cell_width, kHitOdds=a.hit_odds,
                                                    kMissOdds=a.miss_odds)
    if a.save_map or a.map_check:
        map_outputs(a, og, (min_x, min_y), np.asarray(poses), scans, name, report)
    if a.occupancy_grid_mle:
        og = pog.grid_mle(og, unknown_empty=True)
    pog.save_image(og, os.path.join(a.results_dir, "%s_og.png" % name))
    if a.save_map_files:
        pog.save_grid(og, os.path.join(a.results_dir, "%s.map" % name), a.cell_width)
    report["map_" + name] = {"cells": list(og.shape), "origin": [float(min_x), float(min_y)],
                             "s": round(time.perf_counter() - t0, 3)}


def map_outputs(a, og, origin, poses, scans, name, report):
    """--save-map: the grid as slamhip.loc's .npz (the last grid built wins);
    --map-check: every scan's cost on the grid's distance field at its pose."""
    from slamhip import loc
    if a.save_map:
        loc.save_map(a.save_map, og, origin, a.cell_width)
    if a.map_check:
        t0 = time.perf_counter()
        field = loc.LikelihoodField(og, origin, a.cell_width, d_cap=a.map_check_d_cap)
        cost, mean = loc.score_poses(field, scans, poses)
        np.savez(os.path.join(a.results_dir, "%s_map_check.npz" % name), cost=cost, mean=mean, poses=poses,
                 d_cap=np.int64(a.map_check_d_cap))
        report["map_check_" + name] = {"scans": int(len(cost)), "mean_sq_cells": float(np.mean(mean)),
                                       "worst_scan": int(np.argmax(mean)), "worst_sq_cells": float(np.max(mean)),
                                       "s": round(time.perf_counter() - t0, 3)}


def run(a):
    from slamhip import dataset, pipeline
    import src.pose_graph as pose_graph

    os.makedirs(a.results_dir, exist_ok=True)
    out = lambda name: os.path.join(a.results_dir, name)   # noqa: E731
    report = {"dataset": a.dataset}
    odometry, scans, gt_pairs = dataset.load(a.dataset)
    end = a.dataset_end if a.dataset_end is not None else len(odometry)
    odometry = np.asarray(odometry)[a.dataset_start:end]
    scans = list(scans)[a.dataset_start:end]
    report["scans"] = len(scans)
    if a.produce_odometry_map:
        save_map(a, odometry, scans, "odometry", report)

    pg = None
    if a.program_start == "scan_matching":
        t0 = time.perf_counter()
        if a.skip_icp:
            pg = pose_graph.PoseGraph(odometry.copy())
            stem = "odometry_pose_graph"
        else:
            r = pipeline.scan_matching(odometry, scans, a.icp_max_iters, a.icp_epsilon, **refine_params(a),
                                       **edge_check_params(a), repair=a.scan_matching_repair)
            pg = pose_graph.PoseGraph(r.poses)
            stem = "icp_pose_graph"
            report["icp_mean_iters"] = float(np.mean(r.iters)) if len(r.iters) else 0.0
            if r.refine_status is not None:
                report["icp_refine"] = {"method": a.icp_refine, "edges": int(len(r.refine_status)),
                                        "taken": int(r.refine_taken.sum()),
                                        "status": np.bincount(r.refine_status, minlength=4).tolist()}
            if r.verify_ok is not None:
                report["edge_check"] = {"method": a.edge_check, "edges": int(len(r.verify_ok)),
                                        "flagged": int((~r.verify_ok).sum()), "repair": a.scan_matching_repair,
                                        "repaired": int(r.repaired.sum()),
                                        "repair_source": np.bincount(r.repair_source, minlength=3).tolist()}
        report["scan_matching_s"] = round(time.perf_counter() - t0, 3)
        if not a.skip_icp:
            save_map(a, pg.poses, scans, "icp", report)
        pg.save(out(stem + ".pickle"))
        pg.export_g2o(out(stem + ".g2o"))
    if a.program_end == "scan_matching":
        return report

    if pg is None:
        pg = pose_graph.PoseGraph(None)
        pg.load(a.pose_graph)
    if a.program_start in ("scan_matching", "loop_closure"):
        if a.manual_loop_closures is None and a.loop_closure_detection == "proximity":
            t0 = time.perf_counter()
            extra = {}
            cand, ok = closure_check(pipeline.proximity_loop_closures(
                pg, scans, a.proximity_min_dist_along_path, a.proximity_max_dist, a.proximity_icp_error,
                init=a.loop_closure_init, csm=csm_params(a) if a.loop_closure_init == "csm" else None,
                **refine_params(a), **edge_check_params(a)), extra, a)
            report["loop_closure_detection"] = {"method": "proximity", "candidates": len(cand),
                                                "accepted": int(ok.sum()), "init": a.loop_closure_init,
                                                "s": round(time.perf_counter() - t0, 3), **extra}
        elif a.manual_loop_closures is None and a.loop_closure_detection == "descriptors":
            ip = image_params(a)
            descriptors = load_descriptors(a, len(scans), ip["image_downsample"])
            t0 = time.perf_counter()
            extra = {}
            good, ok = closure_check(pipeline.image_loop_closures(
                pg, scans, descriptors, ip["image_downsample"],
                ip["min_dist_along_path"], ip["image_match_error"], ip["keypoint_n_matches"],
                a.loop_closure_icp_error, metric=a.descriptor_metric, init=a.loop_closure_init,
                csm=csm_params(a) if a.loop_closure_init == "csm" else None, **refine_params(a),
                **edge_check_params(a)), extra, a)
            report["loop_closure_detection"] = {"method": "descriptors", "metric": a.descriptor_metric,
                                                "selected": len(good), "accepted": int(ok.sum()),
                                                "init": a.loop_closure_init, "s": round(time.perf_counter() - t0, 3),
                                                **extra}
        elif a.manual_loop_closures is None and a.loop_closure_detection == "signatures":
            from slamhip.sig import SigParams
            t0 = time.perf_counter()
            extra = {}
            cand, ok = closure_check(pipeline.signature_loop_closures(
                pg, scans, a.signature_min_dist_along_path, a.signature_max_frac, a.signature_icp_error,
                init=a.signature_init, csm=csm_params(a) if a.signature_init == "csm" else None,
                params=SigParams(sectors=a.signature_sectors, dr=a.signature_ring_width), **refine_params(a),
                **edge_check_params(a)), extra, a)
            report["loop_closure_detection"] = {"method": "signatures", "candidates": len(cand),
                                                "accepted": int(ok.sum()), "init": a.signature_init,
                                                "s": round(time.perf_counter() - t0, 3), **extra}
        elif a.manual_loop_closures is None:
            print("image-based loop closure detection from images needs OpenCV (out of scope; see "
                  "--loop-closure-detection descriptors); no loop closures added",
                  file=sys.stderr)
        else:
            if a.manual_loop_closures == "auto":
                if gt_pairs is None:
                    raise SystemExit("--manual-loop-closures auto needs a synthetic:loop dataset")
                matches = gt_pairs - a.dataset_start
                matches = matches[(matches >= 0).all(1) & (matches < len(scans)).all(1)]
            else:
                matches = pipeline.read_manual_loop_closures(a.manual_loop_closures)
            t0 = time.perf_counter()
            extra = {}
            ok = closure_check(pipeline.manual_loop_closures(
                pg, scans, matches, init=a.loop_closure_init,
                csm=csm_params(a) if a.loop_closure_init == "csm" else None, **refine_params(a),
                **edge_check_params(a)), extra, a)
            report["loop_closures"] = {"annotated": int(len(matches)), "accepted": int(ok.sum()),
                                       "init": a.loop_closure_init, "s": round(time.perf_counter() - t0, 3), **extra}
        if a.loop_closure_consistency:
            t0 = time.perf_counter()
            edges, keep, unverified, res = pipeline.verify_loop_closures(pg, consistency_params(a), details=True)
            report["loop_closure_consistency"] = {"closures": len(edges), "kept": int(keep.sum()),
                                                  "removed": int(len(edges) - keep.sum()), "unverified": unverified,
                                                  "steps": res.steps if res is not None else 0,
                                                  "seconds": round(time.perf_counter() - t0, 3)}
        pg.save(out("loop_closure_pose_graph.pickle"))
        pg.export_g2o(out("loop_closure_pose_graph.g2o"))
    if a.program_end == "loop_closure":
        return report

    t0 = time.perf_counter()
    robust = {}
    pipeline.optimize(pg, scans, a.optimization_max_iters, a.icp_max_iters, a.icp_epsilon,
                      icp_recompute=a.icp_recompute, method=a.optimizer, gn_iterations=a.gn_iterations,
                      gn_loss=a.gn_loss, gn_loss_scale=a.gn_loss_scale, gn_drop_below=a.gn_drop_below, report=robust)
    report["optimization_s"] = round(time.perf_counter() - t0, 3)
    if a.gn_loss != "none":
        report["gn_loss"] = {"loss": a.gn_loss, "scale": a.gn_loss_scale}
        if a.gn_drop_below is not None:
            report["gn_loss"]["dropped"] = len(robust.get("gn_dropped", []))
            print(f"gn loss: dropped {report['gn_loss']['dropped']} loop closure(s) with ratio below {a.gn_drop_below}",
                  file=sys.stderr)
    save_map(a, pg.poses, scans, "final", report)
    pg.save(out("optim.pickle"))
    pg.export_g2o(out("optim.g2o"))
    return report


def main(argv=None):
    rep = run(parse(argv))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
