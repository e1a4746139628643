#!/usr/bin/env python3
"""Times the pairwise-consistency check of the loop closures
(slam_pcm_adjacency_f64, slam_pcm_select) and measures the basis of its default
tolerances.

Every GPU step runs as a child process of its own under ``timeout``, one at a
time; a step that fails ends the run.

* ``c5``: the C5 stand-in (synthetic.make_loop_sequence(50,000, seed 7)) through
  stage 1 and slamhip.pipeline.signature_loop_closures (about 17k closures).
  - Among the closures that are right in the ground truth (both scans within
    0.5 m and the measured transform within 0.1 m / 0.02 rad of the true one), on
    --sample of them: the distribution of sqrt(dt) and sqrt(dr) of their pairs
    against the chain length n, and for every (tol, drift) of a grid of round
    values the share of true pairs it calls consistent.  The choice: per
    dimension, among the grid points that keep at least 99.5 % (so at least
    99 % jointly), the one with the smallest mean bound over the sampled pairs
    (the one that keeps most when none reaches 99.5 %).
  - Device time (HIP events, the median of --repeats after --warmup) of the
    adjacency pass and of the peel on all closures at the chosen tolerances,
    and what the check keeps of the closures that are right and wrong in the
    ground truth, there and at three tighter settings.
  - tests/pcm_ref.py on one thread on the first --host-size closures: its
    time, and that the device equals it.
* ``synthetic``: the same two times at L = 50,000 closures over a random chain,
  every fourth one wrong.

Needs a GPU: there is no fallback.

    python tools/pcm_time.py --out profiles/pcm_time.json
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

TRANS_TOL = (0.05, 0.1, 0.2, 0.5, 1.0, 2.0)
TRANS_DRIFT = (0.0, 0.001, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5)
ROT_TOL = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)
ROT_DRIFT = (0.0, 0.0002, 0.0005, 0.001, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1)
# (trans_tol, trans_drift, rot_tol, rot_drift) tighter than the choice: what they keep of the right and the wrong
TIGHTER = ((1.0, 0.05, 0.2, 0.01), (0.5, 0.02, 0.1, 0.005), (0.2, 0.01, 0.05, 0.002))
STEP_TIMEOUT_S = {"c5": 900, "synthetic": 300}


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def events(fn, warmup, repeats):
    """Device milliseconds of fn() per call: (list, median)."""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [round(m, 4) for m in ms], round(float(np.median(ms)), 4)


def time_device(X, a, b, Z, tol, warmup, repeats):
    """Adjacency and peel times on resident buffers, and the result."""
    from slamhip import _abi
    from slamhip import device as dv
    lib = _abi.lib()
    L, W = len(a), (len(a) + 31) // 32
    d_X, d_Z = dv.to_dev(X, np.float64), dv.to_dev(Z, np.float64)
    d_a, d_b = dv.to_dev(a, np.int32), dv.to_dev(b, np.int32)
    d_adj = dv.empty((L, W), np.int32)
    d_deg, d_order, d_steps = (dv.empty((n,), np.int32) for n in (L, L, 1))
    d_keep = dv.empty((L,), np.uint8)
    work = dv.empty((int(lib.slam_pcm_work_size(L)),), np.uint8)
    h = dv.stream_handle()

    def adjacency():
        _abi.check(lib.slam_pcm_adjacency_f64(dv.ptr(d_X), len(X), dv.ptr(d_a), dv.ptr(d_b), dv.ptr(d_Z), L, *tol,
                                              dv.ptr(d_adj), dv.ptr(d_deg), dv.ptr(work), h), "slam_pcm_adjacency_f64")

    def peel():
        _abi.check(lib.slam_pcm_select(dv.ptr(d_adj), dv.ptr(d_deg), L, 2, dv.ptr(d_order), dv.ptr(d_keep),
                                       dv.ptr(d_steps), h), "slam_pcm_select")
    adj_ms, adj_med = events(adjacency, warmup, repeats)
    peel_ms, peel_med = events(peel, warmup, repeats)
    _abi.check(lib.slam_pcm_status(h), "slam_pcm_status")
    steps = int(d_steps.cpu().numpy()[0])
    keep = d_keep.cpu().numpy().astype(bool)
    deg = d_deg.cpu().numpy()
    rep = {"closures": L, "ordered_pairs": L * (L - 1), "adjacency_MiB": round(L * W * 4 / 2**20, 1),
           "adjacency_gpu_ms": adj_ms, "adjacency_gpu_ms_median": adj_med,
           "ordered_pairs_per_s": L * (L - 1) / (adj_med * 1e-3),
           "peel_gpu_ms": peel_ms, "peel_gpu_ms_median": peel_med, "peel_steps": steps,
           "peel_us_per_step": round(peel_med * 1e3 / max(steps, 1), 3), "kept": int(keep.sum()),
           "mean_degree": round(float(deg.mean()), 1)}
    return rep, keep, d_adj, d_deg


def tolerance_basis(X, a, b, Z, sample):
    """The distribution of the true pairs' residuals and the grid."""
    import pcm_ref
    rng = np.random.default_rng(0)
    pick = np.sort(rng.choice(len(a), min(sample, len(a)), replace=False))
    dt, dr, n = pcm_ref.pair_terms(X, a[pick], b[pick], Z[pick])
    up = np.triu_indices(len(pick), 1)
    dt, dr, n = dt[up], dr[up], n[up]
    rt, rr = np.sqrt(dt), np.sqrt(dr)
    bins = [(0, 100), (100, 1000), (1000, 10000), (10000, 1 << 40)]
    dist = []
    for lo, hi in bins:
        m = (n >= lo) & (n < hi)
        if m.any():
            dist.append({"n_from": lo, "n_below": hi, "pairs": int(m.sum()),
                         "sqrt_dt_m_p50_p90_p99_max": [round(float(v), 5) for v in
                                                       (*np.percentile(rt[m], [50, 90, 99]), rt[m].max())],
                         "sqrt_dr_p50_p90_p99_max": [round(float(v), 6) for v in
                                                     (*np.percentile(rr[m], [50, 90, 99]), rr[m].max())]})

    def grid(res2, tols, drifts):
        rows, best, most = [], None, None
        for t in tols:
            for d in drifts:
                bound = t * t + (d * d) * n
                share = float((res2 <= bound).mean())
                rows.append([t, d, round(share, 5)])
                if share >= 0.995 and (best is None or bound.mean() < best[2]):
                    best = (t, d, float(bound.mean()), share)
                if most is None or share > most[3]:
                    most = (t, d, float(bound.mean()), share)
        return rows, best if best is not None else most   # no grid point reaches 99.5 %: the one that keeps most
    gt, bt = grid(dt, TRANS_TOL, TRANS_DRIFT)
    gr, br = grid(dr, ROT_TOL, ROT_DRIFT)
    joint = float(((dt <= bt[0] ** 2 + bt[1] ** 2 * n) & (dr <= br[0] ** 2 + br[1] ** 2 * n)).mean())
    return {"true_closures_sampled": int(len(pick)), "true_pairs": int(len(n)),
            "n_p50_p99_max": [float(v) for v in (*np.percentile(n, [50, 99]), n.max())], "by_chain_length": dist,
            "grid_translation_tol_drift_share": gt, "grid_rotation_tol_drift_share": gr,
            "chosen": {"trans_tol": bt[0], "trans_drift": bt[1], "rot_tol": br[0], "rot_drift": br[1],
                       "share_translation": round(bt[3], 5), "share_rotation": round(br[3], 5),
                       "share_joint": round(joint, 5)}}


def step_c5(a):
    import pcm_ref
    import torch
    import src.pose_graph as pgm
    from threadpoolctl import threadpool_limits
    from slamhip import icp, pcm, pipeline, synthetic
    t0 = time.perf_counter()
    seq = synthetic.make_loop_sequence(a.scans, seed=a.seed)
    print(f"generated {a.scans} scans in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
    ss = icp.ScanSet(seq.scans)
    r1 = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    pg = pgm.PoseGraph(r1.poses)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cand, ok = pipeline.signature_loop_closures(pg, seq.scans, scanset=ss)
    stage_s = time.perf_counter() - t0
    edges, _, unverified = pipeline.verify_loop_closures(pg, pcm.PcmParams(), remove=False)   # also the warm-up
    ea = np.array([i for i, _, _ in edges])
    eb = np.array([j for _, j, _ in edges])
    Zm = np.stack([T for _, _, T in edges])
    X, Z = pcm.pose_elements(pg.poses), pcm_ref.from_mats(Zm)
    # right in the ground truth: the same place, and the measured transform the true one
    T = pcm_ref.elements(seq.truth)
    Zt = pcm_ref.mul(pcm_ref.inv(T[ea]), T[eb])
    dxy = np.hypot(Z[:, 2] - Zt[:, 2], Z[:, 3] - Zt[:, 3])
    dth = np.abs(np.arctan2(Z[:, 1] * Zt[:, 0] - Z[:, 0] * Zt[:, 1], Z[:, 0] * Zt[:, 0] + Z[:, 1] * Zt[:, 1]))
    near = np.hypot(*(seq.truth[ea, :2] - seq.truth[eb, :2]).T) <= 0.5
    true = near & (dxy <= 0.1) & (dth <= 0.02)
    rep = {"config": f"C5 stand-in: synthetic.make_loop_sequence({a.scans}, seed={a.seed}), stage-1 poses, "
                     "signature closures", "scans": a.scans, "signature_stage_wall_s": round(stage_s, 3),
           "candidates": len(cand), "closures": len(edges), "unverified": unverified,
           "closures_right_in_truth": int(true.sum()), "closures_wrong_in_truth": int((~true).sum()),
           "chain_end_error_m": round(float(np.hypot(*(pg.poses[-1, :2] - seq.truth[-1, :2]))), 3)}
    rep["tolerance_basis"] = tolerance_basis(X, ea[true], eb[true], Z[true], a.sample)
    c = rep["tolerance_basis"]["chosen"]
    tol = (c["trans_tol"], c["trans_drift"], c["rot_tol"], c["rot_drift"])
    timing, keep, d_adj, d_deg = time_device(X, ea, eb, Z, tol, a.warmup, a.repeats)
    timing["right_kept"], timing["wrong_kept"] = int(keep[true].sum()), int(keep[~true].sum())
    t0 = time.perf_counter()
    wall = pcm.consistency(pg.poses, ea, eb, Zm, pcm.PcmParams(tol[0], tol[2], tol[1], tol[3]))
    timing["consistency_wall_s"] = round(time.perf_counter() - t0, 4)
    timing["wall_equals_timed"] = bool(np.array_equal(wall.keep, keep))
    rep["device"] = timing
    rep["tighter"] = []
    for t in TIGHTER:
        r = pcm.consistency(pg.poses, ea, eb, Zm, pcm.PcmParams(t[0], t[2], t[1], t[3]))
        rep["tighter"].append({"trans_tol": t[0], "trans_drift": t[1], "rot_tol": t[2], "rot_drift": t[3],
                               "right_kept": int(r.keep[true].sum()), "wrong_kept": int(r.keep[~true].sum()),
                               "steps": r.steps, "mean_degree": round(float(r.degree.mean()), 1)})
    m = min(a.host_size, len(ea))
    if m:
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            adj, deg = pcm_ref.adjacency(X, ea[:m], eb[:m], Z[:m], tol)
            t_adj = time.perf_counter() - t0
            t0 = time.perf_counter()
            order, hkeep, steps = pcm_ref.select(adj, deg)
            t_sel = time.perf_counter() - t0
        got = pcm.consistency(pg.poses, ea[:m], eb[:m], Zm[:m], pcm.PcmParams(tol[0], tol[2], tol[1], tol[3]),
                              return_adjacency=True)
        rep["host"] = {"closures": m, "host_threads": 1, "pcm_ref_adjacency_s": round(t_adj, 3),
                       "pcm_ref_select_s": round(t_sel, 3), "steps": int(steps),
                       "device_equals_pcm_ref": bool(np.array_equal(got.adjacency, adj) and
                                                     np.array_equal(got.order, order) and
                                                     np.array_equal(got.keep, hkeep.astype(bool)))}
    return rep


def step_synthetic(a):
    import pcm_ref
    rng = np.random.default_rng(a.seed)
    N, L = a.synthetic, a.synthetic
    truth = np.cumsum(rng.normal(0, 0.3, size=(N, 3)), axis=0)
    poses = truth + np.cumsum(rng.normal(0, 0.001, size=(N, 3)), axis=0)
    X, T = pcm_ref.elements(poses), pcm_ref.elements(truth)
    ea, eb = rng.integers(0, N, L), rng.integers(0, N, L)
    Z = pcm_ref.mul(pcm_ref.inv(T[ea]), T[eb])
    Z[3::4, 2:] += rng.uniform(-2, 2, size=(len(Z[3::4]), 2))
    tol = (0.5, 0.01, 0.2, 0.005)
    rep = time_device(X, ea, eb, Z, tol, a.warmup, a.repeats)[0]
    rep["config"] = f"{L} closures between random nodes of a random chain of {N} poses, every fourth wrong; tol {tol}"
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=["c5", "synthetic"], help="run one step in this process (used by the tool itself)")
    ap.add_argument("--scans", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--synthetic", type=int, default=50000, help="closures of the synthetic step (0: skip)")
    ap.add_argument("--sample", type=int, default=2000, help="true closures whose pairs give the tolerance basis")
    ap.add_argument("--host-size", type=int, default=2000, help="closures for tests/pcm_ref.py (0: skip)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)
    if a.step:
        print(json.dumps({"c5": step_c5, "synthetic": step_synthetic}[a.step](a)))
        return
    rep = {"tool": "pcm_time", "commit": a.commit or commit()}
    for step in ("c5", "synthetic"):
        if step == "synthetic" and not a.synthetic:
            continue
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step",
               step] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                        ("scans", "seed", "synthetic", "sample", "host_size", "warmup", "repeats")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"step {step} ended with status {r.returncode}: nothing further is started")
        rep[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rep[step]), file=sys.stderr, flush=True)
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if "host" in rep["c5"] and not rep["c5"]["host"]["device_equals_pcm_ref"]:
        raise SystemExit("device answers differ from tests/pcm_ref.py")


if __name__ == "__main__":
    main()
