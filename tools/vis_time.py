#!/usr/bin/env python3
"""Times the visibility check of pose-graph edges (slam_vis_tables_f64,
slam_vis_check_f64) and measures what checking and repairing does to the C5
stand-in and to the benchmark's stream.

Every GPU step runs as a child process of its own under ``timeout``, one at a
time; a step that fails ends the run.

* ``c5``: the C5 stand-in (synthetic.make_loop_sequence(50,000, seed 7)): the
  time of the 50,000 range tables and of the check of the 49,999 chain edges and
  of the accepted signature closures (HIP events, the median of --repeats after
  --warmup); the shares of agreeing and conflicting points of the chain edges
  and closures that are right and wrong in the ground truth (the basis of the
  VisParams defaults); the chain's end, max and rms error and end heading for
  ICP, ICP + repair, ICP + ``refine`` and ICP + repair + ``refine``; and what
  the pairwise-consistency check keeps of the checked closures on the repaired
  chain at its defaults and at DESIGN.md section 3.9's tighter settings.
* ``c3``: the benchmark's stream (synthetic.make_sequence(10,001, seed 2025)):
  the same four chains.
* ``bench``: ``bench.py --gpus 1`` with this tree's library and, alternated,
  with the parent commit's (``--parent-lib``, a libslamhip.so built from it):
  the benchmark runs unchanged code, so the new median must lie within the
  parent's own min-max.

Needs a GPU: there is no fallback.

    python tools/vis_time.py --out profiles/vis_time.json [--parent-lib PATH]
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

from plicp_time import TIGHTER, classify, commit, events, quantiles  # noqa: E402

STEP_TIMEOUT_S = {"c3": 600, "c5": 1100, "bench": 900}
EDGE_RIGHT = (0.1, 0.02)   # m, rad: a chain edge this near its true transform is right (the closures' rule)


def chain_report(truth, first, tfs):
    """End, max and rms position error and end heading error of the chain of edges ``tfs`` from ``first``."""
    from slamhip import se2
    poses = se2.compose_chain(first, tfs)
    d = poses[:, :2] - truth[:, :2]
    e = np.hypot(d[:, 0], d[:, 1])
    dh = (poses[-1, 2] - truth[-1, 2] + np.pi) % (2 * np.pi) - np.pi
    return {"end_error_m": round(float(e[-1]), 3), "max_error_m": round(float(e.max()), 3),
            "rms_error_m": round(float(np.sqrt((e ** 2).mean())), 3), "end_heading_error_rad": round(float(abs(dh)), 4)}


def edge_errors(truth, tfs):
    """(translation, rotation) error of the chain edges icp(scan i, scan i - 1) against the truth."""
    import pcm_ref
    T = pcm_ref.elements(truth)
    Zt = pcm_ref.mul(pcm_ref.inv(T[:-1]), T[1:])
    Z = pcm_ref.from_mats(np.asarray(tfs))
    dxy = np.hypot(Z[:, 2] - Zt[:, 2], Z[:, 3] - Zt[:, 3])
    dth = np.abs(np.arctan2(Z[:, 1] * Zt[:, 0] - Z[:, 0] * Zt[:, 1], Z[:, 0] * Zt[:, 0] + Z[:, 1] * Zt[:, 1]))
    return dxy, dth


def share_basis(res, right):
    """The smaller agree share and the larger conflict share of the two directions, right against wrong."""
    lo, hi = res.agree.min(axis=1), res.conflict.max(axis=1)
    out = {}
    for name, m in (("right", right), ("wrong", ~right)):
        out[name] = {"edges": int(m.sum()), "pass": int(res.ok[m].sum()),
                     "agree_share_min_p1_p10_p50_p90_max": quantiles(lo[m]),
                     "conflict_share_min_p1_p10_p50_p90_max": quantiles(hi[m])}
    return out


def four_chains(seq, ss, verify, prm, rep):
    """ICP, ICP + repair, ICP + refine, ICP + repair + refine: the transforms of each, and their reports."""
    import torch
    from slamhip import pipeline, se2
    S = len(seq.scans)
    src, dst = np.arange(1, S), np.arange(0, S - 1)
    pipeline.scan_matching(seq.odometry[:3], seq.scans[:3], verify=verify, refine=prm)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    rep["stage1_wall_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    rv = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss, verify=verify)
    rep["stage1_with_verify_wall_s"] = round(time.perf_counter() - t0, 3)
    assert rv.tf[rv.verify_ok].tobytes() == r.tf[rv.verify_ok].tobytes()
    tf_a, _, _ = pipeline.refine_edges(ss, src, dst, r.tf, prm)
    tf_b, _, _ = pipeline.refine_edges(ss, src, dst, rv.tf, prm)
    chains = {"icp": r.tf, "icp_repair": rv.tf, "icp_refine": tf_a, "icp_repair_refine": tf_b}
    rep["chains"] = {k: chain_report(seq.truth, seq.odometry[0], v) for k, v in chains.items()}
    dxy, dth = edge_errors(seq.truth, r.tf)
    right = (dxy <= EDGE_RIGHT[0]) & (dth <= EDGE_RIGHT[1])
    first = pipeline.check_edges(ss, src, dst, r.tf, verify)
    assert np.array_equal(first.ok, rv.verify_ok)
    dxy2, dth2 = edge_errors(seq.truth, rv.tf)
    flagged = ~rv.verify_ok
    turn = np.abs((np.diff(seq.truth[:, 2]) + np.pi) % (2 * np.pi) - np.pi)
    rep["edges"] = {"edges": int(S - 1), "right_in_truth": int(right.sum()), "wrong_in_truth": int((~right).sum()),
                    "flagged": int(flagged.sum()), "flagged_wrong": int((flagged & ~right).sum()),
                    "flagged_right": int((flagged & right).sum()), "unflagged_wrong": int((~flagged & ~right).sum()),
                    "flagged_at_turns_above_0.5_rad": int((flagged & (turn > 0.5)).sum()),
                    "turns_above_0.5_rad": int((turn > 0.5).sum()),
                    "repair_source_counts_icp_refined_init": np.bincount(rv.repair_source, minlength=3).tolist(),
                    "flagged_right_after_repair": int(((dxy2 <= EDGE_RIGHT[0]) & (dth2 <= EDGE_RIGHT[1]))[flagged].sum()),
                    "flagged_translation_error_m_before_p50_max": quantiles(dxy[flagged])[3::2] if flagged.any() else None,
                    "flagged_translation_error_m_after_p50_max": quantiles(dxy2[flagged])[3::2] if flagged.any() else None,
                    "basis": share_basis(first, right)}
    return r, rv, chains


def closures(seq, ss, poses, verify):
    """The signature closures over ``poses`` (with the check when ``verify``): (edges, right, stage wall s, report)."""
    import torch
    import src.pose_graph as pgm
    from slamhip import pcm, pipeline
    pg = pgm.PoseGraph(poses.copy())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pipeline.signature_loop_closures(pg, seq.scans, scanset=ss, verify=verify)
    wall = time.perf_counter() - t0
    edges, _, _ = pipeline.verify_loop_closures(pg, pcm.PcmParams(), remove=False)
    right = classify(seq.truth, edges)[0] if edges else np.zeros(0, dtype=bool)
    return pg, edges, right, wall, (out[2] if verify is not None else None)


def consistency(pg, edges, right):
    from slamhip import pcm
    ea = np.array([i for i, _, _ in edges])
    eb = np.array([j for _, j, _ in edges])
    Zm = np.stack([T for _, _, T in edges])
    d = pcm.PcmParams()
    out = []
    for t in ((d.trans_tol, d.trans_drift, d.rot_tol, d.rot_drift),) + TIGHTER:
        r = pcm.consistency(pg.poses, ea, eb, Zm, pcm.PcmParams(t[0], t[2], t[1], t[3]))
        out.append({"trans_tol": t[0], "trans_drift": t[1], "rot_tol": t[2], "rot_drift": t[3],
                    "right_kept": int(r.keep[right].sum()), "wrong_kept": int(r.keep[~right].sum())})
    return out


def step_c5(a):
    from slamhip import _abi, icp, plicp, se2, synthetic, vis
    from slamhip import device as dv
    t0 = time.perf_counter()
    seq = synthetic.make_loop_sequence(a.scans, seed=a.seed)
    print(f"generated {a.scans} scans in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
    ss = icp.ScanSet(seq.scans)
    verify, prm = vis.VisParams(), plicp.PlicpParams()
    rep = {"config": f"C5 stand-in: synthetic.make_loop_sequence({a.scans}, seed={a.seed}); default VisParams "
                     f"{verify}, default PlicpParams", "scans": a.scans}
    r, rv, chains = four_chains(seq, ss, verify, prm, rep)
    print(json.dumps({"chains": rep["chains"], "edges": rep["edges"]}), file=sys.stderr, flush=True)
    # the kernels' device time
    lib, h = _abi.lib(), dv.stream_handle()
    n, P, S = len(ss), len(ss.host_pts), verify.sectors
    d_dirs = dv.to_dev(vis.sector_dirs(S), np.float64)
    d_tab = dv.empty((n, S), np.float64)

    def tables():
        _abi.check(lib.slam_vis_tables_f64(dv.ptr(ss.pts), dv.ptr(ss.scan_off), n, P, dv.ptr(d_dirs), S, dv.ptr(d_tab),
                                           h), "slam_vis_tables_f64")
    rep["tables_gpu_ms"], rep["tables_gpu_ms_median"] = events(tables, a.warmup, a.repeats)

    def timed_check(src, dst, tf):
        B = len(src)
        d_src, d_dst = dv.to_dev(src, np.int32), dv.to_dev(dst, np.int32)
        d_tf = dv.to_dev(np.asarray(tf, dtype=np.float64).reshape(B, 9), np.float64)
        out = dv.empty((B, 6), np.int32)

        def check():
            _abi.check(lib.slam_vis_check_f64(dv.ptr(ss.pts), dv.ptr(ss.scan_off), n, P, dv.ptr(d_dirs), S,
                                              dv.ptr(d_tab), dv.ptr(d_src), dv.ptr(d_dst), dv.ptr(d_tf), B,
                                              verify.margin, verify.window, dv.ptr(out), h), "slam_vis_check_f64")
        ms, med = events(check, a.warmup, a.repeats)
        vis.status()
        return ms, med, out.cpu().numpy().astype(np.int64)
    ms, med, counts = timed_check(np.arange(1, n), np.arange(0, n - 1), r.tf)
    assert np.array_equal(counts, rv.verify_counts)
    rep["check_chain_edges"] = {"edges": n - 1, "gpu_ms": ms, "gpu_ms_median": med,
                                "sector_evaluations": int(2 * P * S), "share_of_stage1": round(med * 1e-3 /
                                                                                              rep["stage1_wall_s"], 4)}
    # the signature closures of the ICP chain: right and wrong against the check
    pg0, edges0, right0, wall0, _ = closures(seq, ss, r.poses, None)
    src = np.array([j for _, j, _ in edges0])      # icp(pc_j, pc_i): X_j = X_i T
    dst = np.array([i for i, _, _ in edges0])
    Zm = np.stack([T for _, _, T in edges0])
    ms, med, counts = timed_check(src, dst, Zm)
    res = vis.check_batch(ss, src, dst, Zm, verify)
    assert np.array_equal(res.counts, counts)
    rep["check_signature_closures"] = {"closures": len(edges0), "gpu_ms": ms, "gpu_ms_median": med,
                                       "signature_stage_wall_s": round(wall0, 3),
                                       "share_of_stage": round(med * 1e-3 / wall0, 4),
                                       "right_in_truth": int(right0.sum()), "wrong_in_truth": int((~right0).sum()),
                                       "right_pass": int(res.ok[right0].sum()), "wrong_pass": int(res.ok[~right0].sum()),
                                       "basis": share_basis(res, right0)}
    print(json.dumps({"check_signature_closures": rep["check_signature_closures"]}), file=sys.stderr, flush=True)
    # the stage with the check, on the ICP chain and on the repaired one, and the consistency check after it
    rep["closures"] = {}
    for name, tfs in (("icp", chains["icp"]), ("icp_repair", chains["icp_repair"])):
        poses = se2.compose_chain(seq.odometry[0], tfs)
        row = {}
        for label, v in (("unchecked", None), ("checked", verify)):
            pg, edges, right, wall, check = closures(seq, ss, poses, v)
            row[label] = {"signature_stage_wall_s": round(wall, 3), "closures": len(edges),
                          "right_in_truth": int(right.sum()), "wrong_in_truth": int((~right).sum()),
                          "consistency": consistency(pg, edges, right)}
            if check is not None:
                row[label]["rejected_by_check"] = check.rejected
        rep["closures"][name] = row
    return rep


def step_c3(a):
    from slamhip import icp, plicp, synthetic, vis
    seq = synthetic.make_sequence(a.pairs + 1, seed=2025, n_beams=1081)
    ss = icp.ScanSet(seq.scans)
    rep = {"config": f"C3: synthetic.make_sequence({a.pairs + 1}, seed=2025, n_beams=1081); default VisParams, "
                     "default PlicpParams", "scans": a.pairs + 1}
    four_chains(seq, ss, vis.VisParams(), plicp.PlicpParams(), rep)
    return rep


def step_bench(a):
    """bench.py with the parent's library and with this tree's, alternated."""
    runs = {"parent": [], "this": []}
    for _ in range(a.bench_rounds):
        for name in ("parent", "this"):
            env = dict(os.environ)
            if name == "parent":
                env["SLAMHIP_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("SLAMHIP_LIB", None)
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                                "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)], env=env,
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit(f"bench.py ({name}) ended with status {r.returncode}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            runs[name].append(out["value"])
            print(name, out["value"], file=sys.stderr, flush=True)
    rep = {"command": f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}", "rounds": a.bench_rounds,
           "unit": "scan-pairs/s"}
    for name, v in runs.items():
        rep[name] = {"values": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
    rep["this_median_within_parent_min_max"] = bool(rep["parent"]["min"] <= rep["this"]["median"] <= rep["parent"]["max"])
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=["c3", "c5", "bench"], help="run one step in this process (used by the tool itself)")
    ap.add_argument("--steps", default="c5,c3", help="the steps to run, comma-separated (bench needs --parent-lib)")
    ap.add_argument("--pairs", type=int, default=10000, help="c3: pairs of the stream")
    ap.add_argument("--scans", type=int, default=50000, help="c5: scans")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib", default="", help="bench: a libslamhip.so built from the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    ap.add_argument("--append", action="store_true", help="keep the steps that --out already holds and add these")
    a = ap.parse_args(argv)
    if a.step:
        print(json.dumps({"c3": step_c3, "c5": step_c5, "bench": step_bench}[a.step](a)))
        return
    steps = a.steps.split(",")
    if "bench" in steps and not a.parent_lib:
        ap.error("the bench step needs --parent-lib")
    rep = {"tool": "vis_time", "commit": a.commit or commit()}
    if a.append and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rep = json.load(f)
    for step in steps:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step",
               step] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                        ("pairs", "scans", "seed", "warmup", "repeats", "parent_lib", "bench_rounds", "bench_steps",
                         "bench_warmup")]
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


if __name__ == "__main__":
    main()
