#!/usr/bin/env python3
"""Times the robust Gauss-Newton (slamhip.robust) against the plain one.

Graph: config C4 (synthetic.lap_graph_c4(): 5,000 nodes, 20,000 edges) plus
--wrong (150) wrong closures.  Each joins the same lap position on two laps,
a pair C4 does not hold yet, so the places, the band and the border of C4's
plan stay as they are; its measurement is uniform in +-2 m, +-2 m, +-3 rad.

Measured as slamhip.gn.bench_c4 measures (one process, host clock around
each run, the median of --reps runs of --iterations steps replayed from the
HIP graph, the poses reset before each):

* the plain GaussNewton on that graph, iterations/s;
* RobustGaussNewton (gm, --scale) on it, iterations/s, and the ratio
  robust / plain;
* the replays alone by HIP events (no read-backs), per iteration;
* the reweighting kernel alone: HIP events around one replay of a graph of
  --launches launches, per launch.

Needs a GPU: there is no fallback.

    python tools/robust_time.py --out profiles/robust_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "icp-slam-with-loop-closure_amd")]

import numpy as np  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def c4_with_wrong_closures(n_wrong, seed=0):
    from slamhip import synthetic
    guess, ea, eb, tf, truth = synthetic.lap_graph_c4()
    per_lap, laps = 500, 10
    have = set(zip(ea.tolist(), eb.tolist()))
    rng = np.random.default_rng(1000 + seed)
    xa, xb, xt = [], [], []
    while len(xa) < n_wrong:
        pos = int(rng.integers(per_lap))
        l1, l2 = sorted(rng.choice(laps, 2, replace=False))
        a, b = pos + per_lap * int(l1), pos + per_lap * int(l2)
        if (a, b) in have:
            continue
        have.add((a, b))
        x, y, th = rng.uniform([-2.0, -2.0, -3.0], [2.0, 2.0, 3.0])
        c, s = np.cos(th), np.sin(th)
        xa.append(a)
        xb.append(b)
        xt.append(np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]]))
    wrong = np.r_[np.zeros(len(ea), dtype=bool), np.ones(n_wrong, dtype=bool)]
    return guess, np.r_[ea, xa], np.r_[eb, xb], np.concatenate([tf, np.stack(xt)]), truth, wrong


def timed_runs(s, guess, iterations, reps):
    """bench_c4's timing of one solver: (seconds of each run, the last run's history)."""
    import torch
    from slamhip import device as dv
    start = dv.to_dev(guess, np.float64, s.poses.device)
    s.run(2)            # the eager run
    s.run(iterations)   # the capture of the graph the timed runs replay
    dts = []
    for _ in range(reps):
        s.poses.copy_(start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = s.run(iterations)
        dts.append(time.perf_counter() - t0)
    return dts, hist


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wrong", type=int, default=150)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)
    import torch
    from slamhip import gn, robust
    guess, ea, eb, tf, truth, wrong = c4_with_wrong_closures(a.wrong)
    plan = gn.GnPlan(len(guess), ea, eb)

    def err(p):
        return round(float(np.linalg.norm(p[:, :2] - truth[:, :2], axis=1).max()), 4)

    plain = gn.GaussNewton(guess, ea, eb, tf, plan=plan)
    dt_p, chi_p = timed_runs(plain, guess, a.iterations, a.reps)
    err_p = err(plain.host_poses())
    rob = robust.RobustGaussNewton(guess, ea, eb, tf, "gm", a.scale, plan=plan)
    dt_r, cost_r = timed_runs(rob, guess, a.iterations, a.reps)
    err_r = err(rob.host_poses())
    # the same plain solver again after the robust one: the spread between its two passes
    dt_p2, _ = timed_runs(plain, guess, a.iterations, a.reps)

    def events(fn, per):
        """Device microseconds of fn() by HIP events, divided by `per`: one figure per repetition."""
        fn()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(round(e0.elapsed_time(e1) * 1e3 / per, 3))
        return out

    # the reweighting kernel alone: a.launches of them captured into one HIP graph (eager launches
    # from Python are bound by the host's 10-20 us per call, not by the device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(a.launches):
            rob.reweight()
    us = events(g.replay, a.launches)
    # the replays alone, without a run's read-backs: device time per iteration of either solver
    key = [k for k in plain._graphs if k[0] == a.iterations][0]
    rp_plain = events(plain._graphs[key][0].replay, a.iterations)
    rp_rob = events(rob._graphs[key][0].replay, a.iterations)
    med_p, med_r, med_p2 = (float(np.median(d)) for d in (dt_p, dt_r, dt_p2))
    ips = lambda d: round(a.iterations / d, 2)   # noqa: E731
    rep = {"tool": "robust_time", "commit": a.commit or commit(),
           "graph": f"C4 + {a.wrong} wrong closures: {len(guess)} nodes / {len(ea)} edges", "ordering": plan.ordering,
           "band_W": plan.W, "border_scalars": plan.nv - plan.nv_band,
           "timing": f"median of {a.reps} runs of {a.iterations} iterations (HIP graph replay, host clock around "
                     "each run)",
           "plain_iters_per_sec": ips(med_p), "plain_best_worst": [ips(min(dt_p)), ips(max(dt_p))],
           "plain_again_iters_per_sec": ips(med_p2), "plain_again_best_worst": [ips(min(dt_p2)), ips(max(dt_p2))],
           "robust_loss": "gm", "robust_scale": a.scale,
           "robust_iters_per_sec": ips(med_r), "robust_best_worst": [ips(min(dt_r)), ips(max(dt_r))],
           "robust_over_plain": round(med_p / med_r, 4), "robust_over_plain_again": round(med_p2 / med_r, 4),
           "robust_minus_plain_us_per_iter": round((med_r - med_p) / a.iterations * 1e6, 2),
           "robust_run_note": "a robust run also reads back the cost partials and the final ratios (one extra "
                              "weights-only launch and two copies per run)",
           "replay_only_us_per_iter": {"plain": rp_plain, "robust": rp_rob,
                                       "plain_median": float(np.median(rp_plain)),
                                       "robust_median": float(np.median(rp_rob)),
                                       "note": "HIP events around one replay of each solver's graph, no read-backs; "
                                               "the poses are not reset in between (converged)"},
           "reweight_kernel_us": us, "reweight_kernel_us_median": round(float(np.median(us)), 3),
           "reweight_kernel_note": f"HIP events around one replay of a graph of {a.launches} launches, per launch "
                                   "(its device time plus the gap between two dependent kernels)",
           "plain_chi2_first_last": [float(chi_p[0]), float(chi_p[-1])],
           "robust_cost_first_last": [float(cost_r[0]), float(cost_r[-1])],
           "max_position_error_m": {"plain": err_p, "robust": err_r},
           "wrong_edge_ratio_max": float(rob.ratios[wrong].max()),
           "right_loop_ratio_min": float(rob.ratios[rob.mask & ~wrong].min()),
           "fused_back_fallbacks": gn.FUSED_BACK_FALLBACKS}
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
