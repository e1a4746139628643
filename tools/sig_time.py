#!/usr/bin/env python3
"""Times the scan-signature loop-closure search (slam_sig_build,
slam_sig_match) and the stage built on it.

* Device time of the signature build and of the match at --sizes scans of
  synthetic.make_loop_sequence(N, seed 7) (default 8,000 and 50,000; the scans,
  the signatures, the starts, the outputs and the workspace resident on the
  device): HIP events around each call after --warmup calls, the median of
  --repeats.  The match is timed with the ring-count screen on and off,
  alternating in one process, and both answers are compared.
* The share of pairs that survive the screen, counted on the host from the
  ring counts on --sample rows, and the pairs per second of the match.  An
  evaluated pair costs 64 lanes x 2 S instructions (xor + accumulating
  popcount per mask), a screened pair 8 (the four-byte sums of absolute
  differences); their sum per second is set against the vector issue rate
  DESIGN.md section 3.1 uses (3.92e13 lane-instructions/s).
* tests/sig_ref.py (NumPy, --host-threads BLAS threads) on the first
  --host-size scans: its time, and that the device answers equal it.
* With --stage N (default 50,000; 0 skips it): the C5 stand-in through stage
  1, then slamhip.pipeline.signature_loop_closures on the stage-1 poses and the
  resident ScanSet: wall time of the whole stage, the candidates it finds and
  the closures it accepts (and how many of the candidates lie within 0.5 m in
  the ground truth).

Needs a GPU: there is no fallback.

    python tools/sig_time.py --out profiles/sig_time.json
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

LANE_INSTR_PER_S = 8 * 4.9e12   # 1,024 SIMDs x 16 lanes per cycle x 2.4 GHz


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


def time_search(seq, ss, a):
    from slamhip import _abi, lcd, sig as gsig
    from slamhip import device as dv
    L = _abi.lib()
    params = gsig.SigParams(sectors=a.sectors)
    N, S = len(ss), a.sectors
    dirs, edges2 = params.tables()
    d_dirs, d_edges = dv.to_dev(dirs, np.float64), dv.to_dev(edges2, np.float64)
    sg = gsig.SignatureSet(params, N, ss.device)
    h = dv.stream_handle()

    def build():
        _abi.check(L.slam_sig_build(dv.ptr(ss.pts), dv.ptr(ss.scan_off), N, int(ss.off[-1]), dv.ptr(d_dirs),
                                    dv.ptr(d_edges), S, dv.ptr(sg.d_sig), dv.ptr(sg.d_ring), dv.ptr(sg.d_n), h),
                   "slam_sig_build")
    build_ms, build_med = events(build, a.warmup, a.repeats)

    start, n_rows = lcd.path_starts(seq.odometry, a.min_dist_along_path)
    num, den = a.max_frac
    n_work = int(L.slam_sig_work_size(N, S, 1))
    d_start = dv.to_dev(start[:n_rows], np.int32)
    work = dv.empty((n_work,), np.uint8)
    outs = {s: [dv.empty((n_rows, 1), np.int32) for _ in range(3)] + [dv.empty((n_rows,), np.int32)] for s in (0, 1)}

    def match(screen):
        o = outs[screen]
        _abi.check(L.slam_sig_set_screen(screen), "slam_sig_set_screen")
        _abi.check(L.slam_sig_match(dv.ptr(sg.d_sig), dv.ptr(sg.d_ring), dv.ptr(sg.d_n), N, S, dv.ptr(d_start), n_rows,
                                    num, den, 1, dv.ptr(o[0]), dv.ptr(o[1]), dv.ptr(o[2]), dv.ptr(o[3]), dv.ptr(work),
                                    h), "slam_sig_match")
    try:
        for _ in range(a.warmup):
            match(1)
            match(0)
        on, off = [], []
        for _ in range(a.repeats):   # alternating
            on.append(events(lambda: match(1), 0, 1)[1])
            off.append(events(lambda: match(0), 0, 1)[1])
    finally:
        L.slam_sig_set_screen(1)
    _abi.check(L.slam_sig_status(h), "slam_sig_match")
    same = all(bool((x == y).all()) for x, y in zip(outs[0], outs[1]))

    pairs = int((N - start[:n_rows].astype(np.int64)).sum())
    ring, n = sg.d_ring[:N].cpu().numpy().astype(np.int64), sg.d_n[:N].cpu().numpy().astype(np.int64)
    rows = np.unique(np.random.default_rng(0).integers(0, n_rows, size=min(a.sample, n_rows)))
    kept = seen = 0
    for i in rows:
        lb = np.abs(ring[i][None, :] - ring[start[i]:]).sum(1)
        kept += int((lb * den <= num * (n[i] + n[start[i]:])).sum())
        seen += N - int(start[i])
    share = kept / max(seen, 1)
    med_on, med_off = float(np.median(on)), float(np.median(off))
    lane_instr = pairs * (8 + share * 64 * 2 * S)
    count = outs[1][3].cpu().numpy()
    return sg, {
        "scans": N, "points": int(ss.off[-1]), "sectors": S, "rows": n_rows, "pairs": pairs,
        "workspace_MiB": round(n_work / 2**20, 2),
        "build_gpu_ms": build_ms, "build_gpu_ms_median": build_med,
        "match_screen_on_gpu_ms": on, "match_screen_on_gpu_ms_median": round(med_on, 4),
        "match_screen_on_range_ms": round(max(on) - min(on), 4),
        "match_screen_off_gpu_ms": off, "match_screen_off_gpu_ms_median": round(med_off, 4),
        "screen_on_equals_off": same,
        "share_of_pairs_surviving_screen": round(share, 4), "screen_share_sampled_rows": int(len(rows)),
        "pairs_per_s_screen_on": pairs / (med_on * 1e-3), "pairs_per_s_screen_off": pairs / (med_off * 1e-3),
        "share_of_vector_issue_rate_screen_on": round(lane_instr / (med_on * 1e-3) / LANE_INSTR_PER_S, 4),
        "share_of_vector_issue_rate_screen_off": round(pairs * (8 + 128 * S) / (med_off * 1e-3) / LANE_INSTR_PER_S, 4),
        "rows_with_a_candidate": int((count > 0).sum()), "mean_candidates_per_row": round(float(count.mean()), 2)}


def host_check(seq, a):
    """sig_ref on the first --host-size scans against the device."""
    import sig_ref
    from threadpoolctl import threadpool_limits
    from slamhip import icp, lcd, sig as gsig
    m = min(a.host_size, len(seq.scans))
    num, den = a.max_frac
    start, n_rows = lcd.path_starts(seq.odometry[:m], a.min_dist_along_path)
    with threadpool_limits(limits=a.host_threads):
        t0 = time.perf_counter()
        ref = sig_ref.signatures(seq.scans[:m], *sig_ref.tables(a.sectors))
        t_sig = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = sig_ref.match(ref[0], start, n_rows, num, den, 1)
        t_match = time.perf_counter() - t0
    t0 = time.perf_counter()
    sub = gsig.build_signatures(icp.ScanSet(seq.scans[:m]), gsig.SigParams(sectors=a.sectors))
    got = gsig.match_signatures(sub, start, n_rows, a.max_frac, 1)
    dev_s = time.perf_counter() - t0
    equal = all(np.array_equal(g, w) for g, w in zip(sub.host(), ref)) and \
        all(np.array_equal(g, w) for g, w in zip(got, want))
    return {"scans": m, "host_threads": a.host_threads, "sig_ref_signatures_s": round(t_sig, 3),
            "sig_ref_match_s": round(t_match, 3), "device_upload_build_match_wall_s": round(dev_s, 4),
            "device_equals_sig_ref": bool(equal)}


def time_stage(seq, ss, a):
    import torch
    import src.pose_graph as pgm
    from slamhip import pipeline, sig as gsig
    pipeline.scan_matching(seq.odometry[:3], seq.scans[:3])     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r1 = pipeline.scan_matching(seq.odometry, seq.scans, scanset=ss)
    rep = {"config": f"C5 stand-in: synthetic.make_loop_sequence({len(ss)}, seed={a.seed}), stage-1 poses",
           "scans": len(ss), "stage1_scan_matching_s": round(time.perf_counter() - t0, 3),
           "min_dist_along_path": a.min_dist_along_path, "max_frac": list(a.max_frac), "err_thresh": a.icp_error,
           "init": "signature"}
    pg = pgm.PoseGraph(r1.poses)
    t0 = time.perf_counter()
    cand, ok = pipeline.signature_loop_closures(pg, seq.scans, a.min_dist_along_path, a.max_frac, a.icp_error,
                                                scanset=ss, params=gsig.SigParams(sectors=a.sectors))
    rep["stage_wall_s"] = round(time.perf_counter() - t0, 3)
    rep["candidates"], rep["accepted"] = len(cand), int(ok.sum())
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 3)
    d = np.hypot(*(seq.truth[c[:, 0], :2] - seq.truth[c[:, 1], :2]).T)
    rep["candidates_within_0.5_m_in_truth"] = int((d <= 0.5).sum())
    rep["accepted_within_0.5_m_in_truth"] = int((d[ok] <= 0.5).sum())
    return rep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[8000, 50000])
    ap.add_argument("--host-size", type=int, default=2000, help="scans for tests/sig_ref.py (0: skip)")
    ap.add_argument("--host-threads", type=int, default=1)
    ap.add_argument("--stage", type=int, default=50000, help="scans of the C5 stand-in stage (0: skip)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sectors", type=int, default=64)
    ap.add_argument("--min-dist-along-path", type=float, default=5)
    ap.add_argument("--max-frac", type=int, nargs=2, default=(1, 4))
    ap.add_argument("--icp-error", type=float, default=110)
    ap.add_argument("--sample", type=int, default=1000, help="rows on which the screen's share is counted")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)
    a.max_frac = tuple(a.max_frac)

    from slamhip import device as dv
    from slamhip import icp, synthetic
    t = dv.require_gpu()
    rep = {"tool": "sig_time", "commit": a.commit or commit(), "device": t.cuda.get_device_name(0),
           "lane_instr_per_s": LANE_INSTR_PER_S, "search": []}
    sizes = sorted(set(a.sizes) | ({a.stage} if a.stage else set()))
    for n in sizes:
        t0 = time.perf_counter()
        seq = synthetic.make_loop_sequence(n, seed=a.seed)
        print(f"generated {n} scans in {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
        ss = icp.ScanSet(seq.scans)
        if n in a.sizes:
            r = time_search(seq, ss, a)[1]
            rep["search"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            if a.host_size and "host" not in rep:
                rep["host"] = host_check(seq, a)
        if n == a.stage:
            rep["stage"] = time_stage(seq, ss, a)
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(r["screen_on_equals_off"] for r in rep["search"]):
        raise SystemExit("the screen changed an answer")
    if a.host_size and not rep["host"]["device_equals_sig_ref"]:
        raise SystemExit("device answers differ from tests/sig_ref.py")


if __name__ == "__main__":
    main()
