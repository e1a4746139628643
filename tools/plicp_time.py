#!/usr/bin/env python3
"""Times the point-to-line refinement of ICP edges (slam_plicp_normals_f64,
slam_plicp_batch_f64) and measures what it does to the C5 stand-in.

Every GPU step runs as a child process of its own under ``timeout``, one at a
time; a step that fails ends the run.

* ``c3``: the benchmark's stream (synthetic.make_sequence(10,001, seed 2025,
  1081 beams)): the normals of its scans and the refinement of its 10,000 pairs
  from their ICP results, device time by HIP events (the median of --repeats
  after --warmup), the total of iterations and the distance evaluations per
  second; the chain's error against the truth with and without; and
  tests/plicp_ref.py on one thread on the first --host-pairs pairs, with the
  same answers asserted.
* ``c5``: the C5 stand-in (synthetic.make_loop_sequence(50,000, seed 7)): stage 1
  with and without ``refine``, its time and the chain's drift; the signature
  closures of both chains and what the pairwise-consistency check keeps of the
  right and the wrong ones at its default and at three tighter tolerances; and
  the distribution of ``inliers / n`` and ``obs`` of the refinement over the
  accepted closures, right against wrong in the ground truth (the basis of the
  --refine-min-overlap / --refine-min-observability defaults).

Needs a GPU: there is no fallback.

    python tools/plicp_time.py --out profiles/plicp_time.json
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

# (trans_tol, trans_drift, rot_tol, rot_drift): tools/pcm_time.py's tighter settings
TIGHTER = ((1.0, 0.05, 0.2, 0.01), (0.5, 0.02, 0.1, 0.005), (0.2, 0.01, 0.05, 0.002))
STEP_TIMEOUT_S = {"c3": 600, "c5": 1100}


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


def chain_error(truth, tfs):
    """(rms position, end position, end heading) error of the chain of edges from the true first pose."""
    from slamhip import se2
    X = se2.pose_to_mat(truth[0])
    c = [truth[0]]
    for T in tfs:
        X = X @ T
        c.append((X[0, 2], X[1, 2], np.arctan2(X[1, 0], X[0, 0])))
    c = np.asarray(c)
    d = c[:, :2] - truth[:, :2]
    dh = (c[-1, 2] - truth[-1, 2] + np.pi) % (2 * np.pi) - np.pi
    return {"rms_position_m": round(float(np.sqrt((d ** 2).sum(1).mean())), 5),
            "end_position_m": round(float(np.hypot(*d[-1])), 5), "end_heading_rad": round(float(abs(dh)), 6)}


def quantiles(v):
    v = np.asarray(v, dtype=np.float64)
    if len(v) == 0:
        return None
    return [round(float(x), 4) for x in (v.min(), *np.percentile(v, [1, 10, 50, 90]), v.max())]


def step_c3(a):
    import plicp_ref
    from threadpoolctl import threadpool_limits
    from slamhip import _abi, icp, plicp, se2, synthetic
    from slamhip import device as dv
    seq = synthetic.make_sequence(a.pairs + 1, seed=2025, n_beams=1081)
    B = a.pairs
    inits = np.stack([se2.pose_to_mat(seq.odometry[i] - seq.odometry[i - 1]) for i in range(1, B + 1)])
    ss = icp.ScanSet(seq.scans)
    src, dst = np.arange(1, B + 1), np.arange(0, B)
    r0 = icp.icp_batch(ss, src, dst, inits, epsilon=0.05, max_iters=100)
    prm = plicp.PlicpParams()
    lib, h = _abi.lib(), dv.stream_handle()
    P, S = len(ss.host_pts), len(ss)
    d_n = dv.empty((P, 2), np.float64)
    rho = float(prm.normal_rho)

    def normals():
        _abi.check(lib.slam_plicp_normals_f64(dv.ptr(ss.pts), dv.ptr(ss.scan_off), S, P, prm.normal_k, rho * rho,
                                              prm.corner_tol, dv.ptr(d_n), h), "slam_plicp_normals_f64")
    n_ms, n_med = events(normals, a.warmup, a.repeats)
    d_src, d_dst = dv.to_dev(src, np.int32), dv.to_dev(dst, np.int32)
    d_init = dv.to_dev(r0.tf.reshape(B, 9), np.float64)
    o_tf, o_err, o_obs = dv.empty((B, 9), np.float64), dv.empty((B,), np.float64), dv.empty((B,), np.float64)
    o_inl, o_it, o_st = (dv.empty((B,), np.int32) for _ in range(3))
    max_n1 = int(ss.lens[src].max())

    def refine():
        _abi.check(lib.slam_plicp_batch_f64(
            dv.ptr(ss.pts), dv.ptr(ss.scan_off), S, P, dv.ptr(d_n), dv.ptr(d_src), dv.ptr(d_dst), dv.ptr(d_init), B,
            prm.max_dist ** 2, prm.min_inliers, prm.max_iters, prm.eps_t, prm.eps_r, prm.pivot_tol, max_n1,
            dv.ptr(o_tf), dv.ptr(o_err), dv.ptr(o_obs), dv.ptr(o_inl), dv.ptr(o_it), dv.ptr(o_st), None, 0, h),
            "slam_plicp_batch_f64")
    r_ms, r_med = events(refine, a.warmup, a.repeats)
    plicp.status()
    it, st = o_it.cpu().numpy().astype(np.int64), o_st.cpu().numpy()
    tf = o_tf.cpu().numpy().reshape(B, 3, 3)
    lin = it + (st >= plicp.DEGENERATE)                        # linearisations: a stopped one searched too
    evals = int((lin * ss.lens[src] * ss.lens[dst]).sum())
    has = (d_n.cpu().numpy() != 0).any(axis=1)
    rep = {"config": f"C3: synthetic.make_sequence({B + 1}, seed=2025, n_beams=1081), pairs (i, i-1) refined from "
                     "their ICP results (eps 0.05, max_iters 100); default PlicpParams",
           "scans": S, "points": P, "pairs": B,
           "normals_gpu_ms": n_ms, "normals_gpu_ms_median": n_med, "points_with_normal_share": round(float(has.mean()), 4),
           "refine_gpu_ms": r_ms, "refine_gpu_ms_median": r_med, "iterations_total": int(it.sum()),
           "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
           "status_counts": np.bincount(st, minlength=4).tolist(), "linearisations": int(lin.sum()),
           "distance_evaluations": evals, "distance_evaluations_per_s": evals / (r_med * 1e-3),
           "inlier_share_quantiles_min_p1_p10_p50_p90_max": quantiles(o_inl.cpu().numpy() / ss.lens[src]),
           "obs_quantiles_min_p1_p10_p50_p90_max": quantiles(o_obs.cpu().numpy()),
           "icp_mean_iters": float(r0.iters.mean()),
           "chain_point_to_point": chain_error(seq.truth, r0.tf), "chain_refined": chain_error(seq.truth, tf)}
    m = min(a.host_pairs, B)
    if m:
        N = d_n.cpu().numpy()
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            want = plicp_ref.refine_packed(ss.host_pts, ss.off, src[:m], dst[:m], r0.tf[:m], normals=N)
            t_host = time.perf_counter() - t0
        got = plicp.refine_batch(ss, src[:m], dst[:m], r0.tf[:m], prm, normals=d_n, return_match=True)
        same = all(np.array_equal(got.match[b], w["match"]) and got.iters[b] == w["iters"] and
                   got.status[b] == w["status"] and got.inliers[b] == w["inliers"] and
                   np.abs(got.tf[b] - w["tf"]).max() <= 1e-9 for b, w in enumerate(want))
        rep["host"] = {"pairs": m, "host_threads": 1, "plicp_ref_s": round(t_host, 3),
                       "plicp_ref_ms_per_pair": round(1e3 * t_host / m, 2), "device_equals_plicp_ref": bool(same),
                       "batch_bits_equal_timed_run": bool(got.tf.tobytes() == tf[:m].tobytes())}
    return rep


def classify(truth, edges):
    """Right in the ground truth (tools/pcm_time.py's rule): the same place, and the measured transform the
    true one.  Edges (i, j, T) in the "relative" convention X_j = X_i T.  Returns (right, dxy, dth)."""
    import pcm_ref
    ea = np.array([i for i, _, _ in edges])
    eb = np.array([j for _, j, _ in edges])
    Z = pcm_ref.from_mats(np.stack([T for _, _, T in edges]))
    T = pcm_ref.elements(truth)
    Zt = pcm_ref.mul(pcm_ref.inv(T[ea]), T[eb])
    dxy = np.hypot(Z[:, 2] - Zt[:, 2], Z[:, 3] - Zt[:, 3])
    dth = np.abs(np.arctan2(Z[:, 1] * Zt[:, 0] - Z[:, 0] * Zt[:, 1], Z[:, 0] * Zt[:, 0] + Z[:, 1] * Zt[:, 1]))
    near = np.hypot(*(truth[ea, :2] - truth[eb, :2]).T) <= 0.5
    return near & (dxy <= 0.1) & (dth <= 0.02), dxy, dth


def closures_report(seq, ss, poses, refine):
    """The signature closures over ``poses`` and what the consistency check keeps of them."""
    import torch
    import src.pose_graph as pgm
    from slamhip import pcm, pipeline
    pg = pgm.PoseGraph(poses.copy())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cand, ok = pipeline.signature_loop_closures(pg, seq.scans, scanset=ss, refine=refine)
    stage_s = time.perf_counter() - t0
    edges, _, _ = pipeline.verify_loop_closures(pg, pcm.PcmParams(), remove=False)
    right, dxy, dth = classify(seq.truth, edges)
    ea = np.array([i for i, _, _ in edges])
    eb = np.array([j for _, j, _ in edges])
    Zm = np.stack([T for _, _, T in edges])
    rep = {"signature_stage_wall_s": round(stage_s, 3), "candidates": len(cand), "closures": len(edges),
           "right_in_truth": int(right.sum()), "wrong_in_truth": int((~right).sum()),
           "right_translation_error_m_p50_p90": [round(float(v), 5) for v in np.percentile(dxy[right], [50, 90])],
           "right_rotation_error_rad_p50_p90": [round(float(v), 6) for v in np.percentile(dth[right], [50, 90])],
           "consistency": []}
    for t in ((pcm.PcmParams().trans_tol, pcm.PcmParams().trans_drift, pcm.PcmParams().rot_tol,
               pcm.PcmParams().rot_drift),) + TIGHTER:
        t0 = time.perf_counter()
        r = pcm.consistency(pg.poses, ea, eb, Zm, pcm.PcmParams(t[0], t[2], t[1], t[3]))
        rep["consistency"].append({"trans_tol": t[0], "trans_drift": t[1], "rot_tol": t[2], "rot_drift": t[3],
                                   "right_kept": int(r.keep[right].sum()), "wrong_kept": int(r.keep[~right].sum()),
                                   "steps": r.steps, "wall_s": round(time.perf_counter() - t0, 3)})
    return rep, edges, right


def step_c5(a):
    import torch
    from slamhip import icp, pipeline, plicp, synthetic
    t0 = time.perf_counter()
    seq = synthetic.make_loop_sequence(a.scans, seed=a.seed)
    print(f"generated {a.scans} scans in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
    ss = icp.ScanSet(seq.scans)
    prm = plicp.PlicpParams()
    pipeline.scan_matching(seq.odometry[:3], seq.scans[:3], refine=prm)   # warm-up
    torch.cuda.synchronize()
    rep = {"config": f"C5 stand-in: synthetic.make_loop_sequence({a.scans}, seed={a.seed}); default PlicpParams, "
                     "gates (0.5, 0)", "scans": a.scans}
    runs = {}
    for name, refine in (("point_to_point", None), ("refined", prm)):
        t0 = time.perf_counter()
        r1 = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, refine=refine)
        wall = time.perf_counter() - t0
        d = r1.poses[:, :2] - seq.truth[:, :2]
        run = {"stage1_wall_s": round(wall, 3), "chain_end_error_m": round(float(np.hypot(*d[-1])), 3),
               "chain_max_error_m": round(float(np.hypot(d[:, 0], d[:, 1]).max()), 3),
               "chain_end_heading_error_rad": round(float(abs((r1.poses[-1, 2] - seq.truth[-1, 2] + np.pi)
                                                              % (2 * np.pi) - np.pi)), 4)}
        if refine is not None:
            run["refine_status_counts"] = np.bincount(r1.refine_status, minlength=4).tolist()
            run["refine_taken"] = int(r1.refine_taken.sum())
            run["inlier_share_quantiles_min_p1_p10_p50_p90_max"] = quantiles(r1.refine_inliers / ss.lens[1:])
            run["obs_quantiles_min_p1_p10_p50_p90_max"] = quantiles(r1.refine_obs)
        run["closures"], edges, right = closures_report(seq, ss, r1.poses, refine)
        runs[name] = (run, edges, right)
        rep[name] = run
        print(json.dumps({name: run}), file=sys.stderr, flush=True)
    # the gates' basis: the refinement of the point-to-point chain's accepted closures, right against wrong
    _, edges, right = runs["point_to_point"]
    src = np.array([j for _, j, _ in edges])      # icp(pc_j, pc_i): X_j = X_i T
    dst = np.array([i for i, _, _ in edges])
    Zm = np.stack([T for _, _, T in edges])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = plicp.refine_batch(ss, src, dst, Zm, prm)
    wall = time.perf_counter() - t0
    share = res.inliers / ss.lens[src]
    fine = (res.status == plicp.CONVERGED) | (res.status == plicp.MAX_ITERS)
    new_right, dxy, _ = classify(seq.truth, [(i, j, T) for (i, j, _), T in zip(edges, res.tf)])
    _, dxy0, _ = classify(seq.truth, edges)
    basis = {"closures": len(edges), "refine_wall_s": round(wall, 3)}
    for name, m in (("right", right), ("wrong", ~right)):
        basis[name] = {"closures": int(m.sum()), "status_counts": np.bincount(res.status[m], minlength=4).tolist(),
                       "inlier_share_quantiles_min_p1_p10_p50_p90_max": quantiles(share[m & fine]),
                       "obs_quantiles_min_p1_p10_p50_p90_max": quantiles(res.obs[m & fine]),
                       "translation_error_m_p50_p90_before": quantiles(dxy0[m])[3:5] if m.any() else None,
                       "translation_error_m_p50_p90_after": quantiles(dxy[m & fine])[3:5] if (m & fine).any() else None,
                       "right_after_refinement": int(new_right[m & fine].sum())}
    grid = []
    for mo in (0.3, 0.5, 0.6, 0.7, 0.8, 0.9):
        for ob in (0.0, 0.05, 0.1, 0.2):
            take = fine & (share >= mo) & (res.obs >= ob)
            grid.append([mo, ob, int(take[right].sum()), int(take[~right].sum())])
    basis["gate_grid_min_overlap_min_obs_right_taken_wrong_taken"] = grid
    rep["closure_gates_basis"] = basis
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=["c3", "c5"], help="run one step in this process (used by the tool itself)")
    ap.add_argument("--steps", default="c3,c5", help="the steps to run, comma-separated")
    ap.add_argument("--pairs", type=int, default=10000, help="c3: pairs of the stream")
    ap.add_argument("--host-pairs", type=int, default=64, help="c3: pairs for tests/plicp_ref.py (0: skip)")
    ap.add_argument("--scans", type=int, default=50000, help="c5: scans")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)
    if a.step:
        print(json.dumps({"c3": step_c3, "c5": step_c5}[a.step](a)))
        return
    rep = {"tool": "plicp_time", "commit": a.commit or commit()}
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step",
               step] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                        ("pairs", "host_pairs", "scans", "seed", "warmup", "repeats")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"step {step} ended with status {r.returncode}: nothing further is started")
        rep[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rep[step]), file=sys.stderr, flush=True)
        if a.out:   # after every step: a later step that fails leaves the earlier ones on record
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(rep) + "\n")
    print(json.dumps(rep))
    if "c3" in rep and "host" in rep["c3"] and not rep["c3"]["host"]["device_equals_plicp_ref"]:
        raise SystemExit("device answers differ from tests/plicp_ref.py")


if __name__ == "__main__":
    main()
