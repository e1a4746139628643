#!/usr/bin/env python3
"""Localises the scans of a dataset in a saved occupancy grid on the GPU
(slamhip.loc; kernels in csrc/loc_kernels.hip).

``--map FILE`` is the ``.npz`` that ``main_batched.py --save-map FILE`` wrote;
``dataset``, ``--dataset-start`` and ``--dataset-end`` are main_batched.py's.
``--guess odometry`` (default) tracks: every scan is searched in a window
around its odometry pose and refined; ``--guess none`` relocalises: windows
tile the whole map and the angle bins cover the full circle.  Writes
``localize.npz`` (poses (x, y, theta), status, iters, inliers, rms, search_cost,
search_index, scans) into ``--results-dir`` and prints a JSON summary.

    python icp-slam-with-loop-closure_amd/scripts/localize.py synthetic:loop:600:3 \\
        --map /tmp/results/map.npz --results-dir /tmp/results
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("dataset")
    p.add_argument("--map", required=True, help="the .npz of main_batched.py --save-map")
    p.add_argument("--dataset-start", default=0, type=int)
    p.add_argument("--dataset-end", type=int)
    p.add_argument("--every", default=1, type=int, help="localise every n-th scan of the slice")
    p.add_argument("--guess", default="odometry", choices=["odometry", "none"],
                   help="odometry = window search around the odometry pose (default); none = relocalise in the whole map")
    p.add_argument("--d-cap", default=20, type=int, help="cap of the distance field (cells, 1..255)")
    p.add_argument("--occ-min", default=0, type=int, help="a cell is occupied above this value")
    p.add_argument("--window-cells", type=int, help="shifts per axis (default: 21)")
    p.add_argument("--step", type=int, help="cells per shift (default: 1 with a guess, 2 without)")
    p.add_argument("--angle-bins", default=41, type=int, help="angle bins around the guess (ignored without one)")
    p.add_argument("--angle-step-deg", type=float,
                   help="angle bin spacing (default: 0.0125 rad with a guess, 3 degrees without)")
    p.add_argument("--refine-max-iters", default=30, type=int)
    p.add_argument("--min-inlier-frac", default=0.5, type=float)
    p.add_argument("--results-dir", default="results")
    a = p.parse_args(argv)
    if a.every < 1:
        p.error("--every >= 1 expected")
    try:
        loc_params(a)
    except ValueError as e:
        p.error(str(e))
    if not 1 <= a.d_cap <= 255 or not -128 <= a.occ_min <= 127:
        p.error("--d-cap in 1..255 and --occ-min in -128..127 expected")
    return a


def loc_params(a):
    """LocParams of the window flags, the defaults of the chosen mode where unset."""
    from slamhip.loc import LocParams
    track = a.guess == "odometry"
    side = a.window_cells if a.window_cells is not None else 21
    step = a.step if a.step is not None else (1 if track else 2)
    d_theta = np.deg2rad(a.angle_step_deg) if a.angle_step_deg is not None else (0.0125 if track else np.deg2rad(3.0))
    if not d_theta > 0:
        raise ValueError("--angle-step-deg > 0 expected")
    return LocParams(n_theta=a.angle_bins, d_theta=d_theta, nx=side, ny=side, step=step, max_iters=a.refine_max_iters,
                     min_inlier_frac=a.min_inlier_frac)


def run(a):
    from slamhip import dataset, loc
    from slamhip.icp import ScanSet

    os.makedirs(a.results_dir, exist_ok=True)
    grid, origin, cw = loc.load_map(a.map)
    odometry, scans, _ = dataset.load(a.dataset)
    end = a.dataset_end if a.dataset_end is not None else len(odometry)
    which = np.arange(a.dataset_start, end)[::a.every]
    odometry = np.asarray(odometry)[which]
    t0 = time.perf_counter()
    field = loc.LikelihoodField(grid, origin, cw, d_cap=a.d_cap, occ_min=a.occ_min)
    ss = ScanSet([scans[i] for i in which], field.device)
    idx = np.arange(len(which))
    params = loc_params(a)
    r = loc.localize(field, ss, idx, odometry, params) if a.guess == "odometry" else loc.relocalize(field, ss, idx, params)
    seconds = time.perf_counter() - t0
    np.savez(os.path.join(a.results_dir, "localize.npz"), poses=r.poses, status=r.refine.status, iters=r.refine.iters,
             inliers=r.refine.inliers, rms=r.refine.rms, search_cost=r.search.cost, search_index=r.search.index,
             scans=which)
    return {"dataset": a.dataset, "map": a.map, "cells": list(grid.shape), "guess": a.guess, "scans": int(len(which)),
            "status": np.bincount(r.refine.status, minlength=4).tolist(), "status_names": list(loc.STATUS_NAMES),
            "mean_rms_m": float(np.nanmean(r.refine.rms)) if len(which) else 0.0, "s": round(seconds, 3)}


def main(argv=None):
    print(json.dumps(run(parse(argv))))


if __name__ == "__main__":
    main()
