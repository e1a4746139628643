#!/usr/bin/env python3
"""Times the proximity loop-closure search (slam_lcd_nearest_f64) and the stage
built on it.

* Device time of the search at --sizes poses (default 50,000 and 8,000; laps of
  a circle, the generator of tests/test_lcd_gpu.py): poses, starts, outputs and
  the workspace resident on the device, HIP events around each call after a
  warm-up call, the median of --repeats calls.  Pair evaluations are counted
  from the starts (sum of N - start[i]) and reported per second and as a share
  of the fp64 vector issue rate DESIGN.md section 3.1 uses (4.9e12 candidates/s
  at 8 lane-instructions each: 3.92e13 lane-instructions/s), at the 6 fp64
  instructions a pair costs (2 subtractions, 2 products, 1 sum, 1 compare).
* Host time of src.loop_closure_detection.proximity_candidates (the N x N
  cdist matrix) at --host-size poses (default 8,000: 512 MB), one run, and
  that the device list equals it.
* With --stage N (default 50,000; 0 skips it): the C5 stand-in
  (synthetic.make_loop_sequence(N, seed 7), as tools/c5_pipeline.py) through
  stage 1, then slamhip.pipeline.proximity_loop_closures on the stage-1 poses
  and the resident ScanSet: wall time of the whole stage, of its candidate
  search alone, the candidates it finds and the closures it accepts.

Needs a GPU: there is no fallback.

    python tools/lcd_time.py --out profiles/lcd_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "icp-slam-with-loop-closure_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402

FP64_LANE_INSTR_PER_S = 8 * 4.9e12   # 1,024 SIMDs x 16 lanes per cycle x 2.4 GHz
FP64_INSTR_PER_PAIR = 6


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def time_search(poses, mdp, warmup, repeats):
    """Median device milliseconds of slam_lcd_nearest_f64 on resident data."""
    from slamhip import _abi, lcd
    from slamhip import device as dv
    t = dv.require_gpu()
    N = len(poses)
    start, n_rows = lcd.path_starts(poses, mdp)
    L = _abi.lib()
    n_work = int(L.slam_lcd_work_size(N))
    d_poses = dv.to_dev(poses[:, :3], np.float64)
    d_start = dv.to_dev(start[:n_rows], np.int32)
    work = dv.empty((n_work,), np.uint8)
    out_j, out_d = dv.empty((n_rows,), np.int32), dv.empty((n_rows,), np.float64)

    def timed():
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        _abi.check(L.slam_lcd_nearest_f64(dv.ptr(d_poses), N, dv.ptr(d_start), n_rows, dv.ptr(out_j), dv.ptr(out_d),
                                          dv.ptr(work), dv.stream_handle()), "slam_lcd_nearest_f64")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        timed()
    ms = [timed() for _ in range(repeats)]
    med = float(np.median(ms))
    pairs = int((N - start[:n_rows].astype(np.int64)).sum())
    rate = pairs / (med * 1e-3)
    return {"poses": N, "rows": n_rows, "pair_evaluations": pairs, "workspace_MiB": round(n_work / 2**20, 2),
            "gpu_ms": [round(m, 4) for m in ms], "gpu_ms_median": round(med, 4), "pairs_per_s": rate,
            "share_of_fp64_issue_rate": round(rate * FP64_INSTR_PER_PAIR / FP64_LANE_INSTR_PER_S, 4),
            "within_max_dist_1": int((out_d.cpu().numpy() <= 1).sum())}


def time_stage(n, seed, mdp, max_dist, err_thresh, warmup, repeats):
    import torch
    import src.pose_graph as pgm
    from slamhip import icp as k
    from slamhip import lcd, pipeline, synthetic
    t0 = time.perf_counter()
    seq = synthetic.make_loop_sequence(n, seed=seed)
    print(f"generated {n} scans in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
    pipeline.scan_matching(seq.odometry[:3], seq.scans[:3])     # warm-up
    ss = k.ScanSet(seq.scans)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r1 = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    rep = {"config": f"C5 stand-in: synthetic.make_loop_sequence({n}, seed={seed}), stage-1 poses",
           "scans": n, "ground_truth_loop_pairs": int(len(seq.loop_pairs)),
           "stage1_scan_matching_s": round(time.perf_counter() - t0, 3),
           "min_dist_along_path": mdp, "max_dist": max_dist, "err_thresh": err_thresh}
    rep["search_kernel"] = time_search(r1.poses, mdp, warmup, repeats)
    t0 = time.perf_counter()
    cand = lcd.proximity_candidates_device(r1.poses, mdp, max_dist)
    rep["candidate_search_wall_s"] = round(time.perf_counter() - t0, 4)   # path rule, upload, kernels, list
    pg = pgm.PoseGraph(r1.poses)
    t0 = time.perf_counter()
    cand2, ok = pipeline.proximity_loop_closures(pg, seq.scans, mdp, max_dist, err_thresh, scanset=ss)
    rep["stage_wall_s"] = round(time.perf_counter() - t0, 3)
    assert cand2 == cand
    rep["candidates"], rep["accepted"] = len(cand), int(ok.sum())
    # the same rule on the odometry the generator hands out (no chain drift), for comparison
    rep["candidates_on_input_odometry"] = len(lcd.proximity_candidates_device(seq.odometry, mdp, max_dist))
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[50000, 8000])
    ap.add_argument("--host-size", type=int, default=8000, help="poses for the host rule (0: skip)")
    ap.add_argument("--stage", type=int, default=50000, help="scans of the C5 stand-in stage (0: skip)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--min-dist-along-path", type=float, default=2)
    ap.add_argument("--max-dist", type=float, default=1)
    ap.add_argument("--icp-error", type=float, default=110)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)

    from test_lcd_gpu import lap_poses
    import src.loop_closure_detection as host
    from slamhip import lcd
    from slamhip import device as dv
    t = dv.require_gpu()
    rep = {"tool": "lcd_time", "commit": a.commit or commit(), "device": t.cuda.get_device_name(0),
           "poses": "laps of a circle of radius 3 m, step 0.05 m (tests/test_lcd_gpu.py lap_poses, seed 11)",
           "fp64_lane_instr_per_s": FP64_LANE_INSTR_PER_S, "fp64_instr_per_pair": FP64_INSTR_PER_PAIR,
           "search": [time_search(lap_poses(n), a.min_dist_along_path, a.warmup, a.repeats) for n in a.sizes]}
    if a.host_size:
        poses = lap_poses(a.host_size)
        t0 = time.perf_counter()
        want = host.proximity_candidates(poses, a.min_dist_along_path, a.max_dist)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        got = lcd.proximity_candidates_device(poses, a.min_dist_along_path, a.max_dist)
        dev_s = time.perf_counter() - t0
        rep["host"] = {"poses": a.host_size, "host_s": round(host_s, 3), "matrix_MB": a.host_size ** 2 * 8 // 10**6,
                       "cpu_threads": os.environ.get("OMP_NUM_THREADS"), "device_call_wall_s": round(dev_s, 4),
                       "candidates": len(want), "device_equals_host": got == want}
    if a.stage:
        rep["stage"] = time_stage(a.stage, a.seed, a.min_dist_along_path, a.max_dist, a.icp_error, a.warmup,
                                  a.repeats)
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.host_size and not rep["host"]["device_equals_host"]:
        raise SystemExit("device candidates differ from the host rule")


if __name__ == "__main__":
    main()
