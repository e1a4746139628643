#!/usr/bin/env python3
"""Times the localisation in a finished occupancy grid (slamhip.loc,
csrc/loc_kernels.hip) on resident data with HIP events after a warm-up call:

* the field (slam_loc_field) of a 2,000 x 2,000 grid, the C5 stand-in's map
  tiled to that size, at d_cap 15 and 40;
* the window search (slam_loc_search) of --scans scans (default 1,000) of
  1081 points in the C5 stand-in's map at the tracking window 41 x 21 x 21,
  step 1, with table look-ups per second (look-ups = angles x shifts x query
  points, counted from the shapes), at d_cap 20 (2-byte table) and at d_cap 15
  with the 2-byte and the 1-byte table, alternating;
* the refinement (slam_loc_refine_f64) of the same queries from the search's bins;
* one global relocalisation of a 1081-point scan in that map (step 2 cells,
  3 degree bins): its search launch, and the whole call by the wall clock;
* the NumPy restatement (tests/loc_ref.py) on --cpu-scans of the same queries,
  checking that the GPU's bins and costs are the restatement's.

The map is built on the GPU from the even scans of the first lap of
make_loop_sequence at their true poses, 0.05 m cells.  Needs a GPU: there is no
fallback.

    python tools/loc_time.py --out profiles/loc_time.json
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


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scans", type=int, default=1000)
    ap.add_argument("--beams", type=int, default=1081)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--field-cells", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-scans", type=int, default=4, help="queries the NumPy restatement runs (0: none)")
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)

    import loc_ref
    import src.produce_occupancy_grid as pog
    from slamhip import _abi, loc, synthetic
    from slamhip import device as dv
    from slamhip.icp import ScanSet
    t = dv.require_gpu()
    L = _abi.lib()

    def events(fn, width=2):
        _abi.check(L.slam_loc_set_table(width), "slam_loc_set_table")
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        _abi.check(L.slam_loc_set_table(2), "slam_loc_set_table")
        return e0.elapsed_time(e1)

    def median_ms(fn, width=2):
        for _ in range(a.warmup):
            events(fn, width)
        ms = [events(fn, width) for _ in range(a.repeats)]
        return [round(m, 3) for m in ms], round(float(np.median(ms)), 3)

    probe = synthetic.make_loop_sequence(1, seed=a.seed, n_beams=8)
    seq = synthetic.make_loop_sequence(max(probe.per_lap, a.scans), seed=a.seed, n_beams=a.beams)
    lap = np.arange(probe.per_lap)
    map_idx = lap[lap % 2 == 0]
    cw = 0.05
    grid, origin = pog.produce_occupancy_grid(seq.truth[map_idx], [seq.scans[i] for i in map_idx], cw)
    rep = {"tool": "loc_time", "commit": a.commit or commit(), "device": t.cuda.get_device_name(0),
           "map_cells": list(grid.shape), "cell_width": cw, "beams": a.beams}

    # ---- the field of a large grid
    n = a.field_cells
    big = np.ascontiguousarray(np.tile(grid, (-(-n // grid.shape[0]), -(-n // grid.shape[1])))[:n, :n])
    d_big = dv.to_dev(big, np.int8)
    out = t.empty((n, n), dtype=t.int16, device=d_big.device)
    work = dv.empty((int(L.slam_loc_field_work_size(n, n)),), np.uint8, d_big.device)
    rep["field"] = {"cells": [n, n], "occupied_share": float((big > 0).mean())}
    for d_cap in (15, 40):
        def field_call():
            _abi.check(L.slam_loc_field(dv.ptr(d_big), n, n, 0, d_cap, dv.ptr(out), dv.ptr(work), dv.stream_handle()),
                       "slam_loc_field")
        ms, med = median_ms(field_call)
        rep["field"]["d_cap_%d" % d_cap] = {"ms": ms, "ms_median": med,
                                            "cell_ops_per_s": n * n * (2 * d_cap + 1) / (med * 1e-3),
                                            "equals_restatement": bool(np.array_equal(
                                                out.cpu().numpy().view(np.uint16), loc_ref.field(big, d_cap)))}
    del d_big, out, work

    # ---- the tracking search and the refinement
    B = a.scans
    ss = ScanSet(seq.scans[:B])
    idx = np.arange(B)
    rng = np.random.default_rng(11)
    guess = seq.truth[:B].copy()
    guess[:, :2] += rng.uniform(-0.4, 0.4, size=(B, 2))
    guess[:, 2] += rng.uniform(-0.2, 0.2, size=B)
    p = loc.LocParams(n_theta=41, d_theta=0.0125, nx=21, ny=21, step=1)
    centre = guess[:, [2, 0, 1]]
    dev = ss.device
    d_idx = dv.to_dev(idx, np.int32, dev)
    d_centre = dv.to_dev(centre, np.float64, dev)
    d_rot = dv.to_dev(loc.rotations(centre, p), np.float64, dev)
    best = dv.empty((B, 4), np.int32, dev)
    swork = dv.empty((int(L.slam_loc_search_work_size(B, grid.shape[0], grid.shape[1], p.n_theta, p.ny, p.nx, p.step)),),
                     np.uint8, dev)
    max_n = int(ss.lens.max())
    lookups = p.n_theta * p.ny * p.nx * int(ss.lens[idx].sum())
    rep["search"] = {"scans": B, "query_points": int(ss.lens[idx].sum()), "window": [p.n_theta, p.ny, p.nx, p.step],
                     "lookups": lookups, "csm_lookups_per_s_for_comparison": 1.07e13}
    fields = {}
    for d_cap in (20, 15):
        f = fields[d_cap] = loc.LikelihoodField(grid, origin, cw, d_cap=d_cap)

        def search_call():
            _abi.check(L.slam_loc_search(*loc._map_args(f), dv.ptr(ss.pts), dv.ptr(ss.scan_off), len(ss),
                                         len(ss.host_pts), dv.ptr(d_idx), dv.ptr(d_centre), dv.ptr(d_rot), B, max_n,
                                         p.n_theta, p.nx, p.ny, p.step, dv.ptr(best), None, dv.ptr(swork),
                                         dv.stream_handle()), "slam_loc_search")
        for width in ((2,) if d_cap > 15 else (2, 1)):
            ms, med = median_ms(search_call, width)
            rep["search"]["d_cap_%d_table_%dB" % (d_cap, width)] = {
                "ms": ms, "ms_median": med, "ms_per_scan": round(med / B, 4), "lookups_per_s": lookups / (med * 1e-3)}
            if d_cap == 20:
                got = best.cpu().numpy()
    f = fields[20]
    start = loc.assemble(centre, got[:, 1:], p, cw)
    ep, et = loc_ref.pose_error(start, seq.truth[:B])
    rep["search"]["bin_error_max"] = [float(ep.max()), float(et.max())]
    d_init = dv.to_dev(start[:, [2, 0, 1]], np.float64, dev)
    o_pose, o_rms = dv.empty((B, 3), np.float64, dev), dv.empty((B,), np.float64, dev)
    o_inl, o_it, o_st = (dv.empty((B,), np.int32, dev) for _ in range(3))

    def refine_call():
        _abi.check(L.slam_loc_refine_f64(*loc._map_args(f), dv.ptr(ss.pts), dv.ptr(ss.scan_off), len(ss),
                                         len(ss.host_pts), dv.ptr(d_idx), dv.ptr(d_init), B, max_n, p.max_iters,
                                         p.eps_t, p.eps_r, p.min_inlier_frac, p.pivot_tol, dv.ptr(o_pose),
                                         dv.ptr(o_rms), dv.ptr(o_inl), dv.ptr(o_it), dv.ptr(o_st), dv.stream_handle()),
                   "slam_loc_refine_f64")
    ms, med = median_ms(refine_call)
    pose = o_pose.cpu().numpy()[:, [1, 2, 0]]
    ep, et = loc_ref.pose_error(pose, seq.truth[:B])
    # scans of the first lap's even positions built the map; the others are held out
    rep["refine"] = {"ms": ms, "ms_median": med, "ms_per_scan": round(med / B, 4),
                     "mean_iters": float(o_it.cpu().numpy().mean()),
                     "status": np.bincount(o_st.cpu().numpy(), minlength=4).tolist(),
                     "error_max": [float(ep.max()), float(et.max())], "error_median": [float(np.median(ep)),
                                                                                       float(np.median(et))]}

    # ---- one global relocalisation
    q = loc.reloc_params(loc.LocParams(nx=21, ny=21, step=2, d_theta=np.deg2rad(3.0)))
    centres = loc.reloc_centres(f.H, f.W, f.origin, cw, q)
    T = len(centres)
    scan = 151
    r_idx = dv.to_dev(np.full(T, scan), np.int32, dev)
    r_centre = dv.to_dev(centres, np.float64, dev)
    r_rot = dv.to_dev(loc.rotations(centres, q), np.float64, dev)
    r_best = dv.empty((T, 4), np.int32, dev)
    r_work = dv.empty((int(L.slam_loc_search_work_size(T, f.H, f.W, q.n_theta, q.ny, q.nx, q.step)),), np.uint8, dev)

    def reloc_call():
        _abi.check(L.slam_loc_search(*loc._map_args(f), dv.ptr(ss.pts), dv.ptr(ss.scan_off), len(ss), len(ss.host_pts),
                                     dv.ptr(r_idx), dv.ptr(r_centre), dv.ptr(r_rot), T, max_n, q.n_theta, q.nx, q.ny,
                                     q.step, dv.ptr(r_best), None, dv.ptr(r_work), dv.stream_handle()),
                   "slam_loc_search")
    ms, med = median_ms(reloc_call)
    r_lookups = T * q.n_theta * q.ny * q.nx * int(ss.lens[scan])
    t0 = time.perf_counter()
    r = loc.relocalize(f, ss, [scan], loc.LocParams(nx=21, ny=21, step=2, d_theta=np.deg2rad(3.0)))
    wall = time.perf_counter() - t0
    ep, et = loc_ref.pose_error(r.poses, seq.truth[scan])
    rep["relocalize"] = {"scan": scan, "tiles": T, "window": [q.n_theta, q.ny, q.nx, q.step], "lookups": r_lookups,
                         "search_ms": ms, "search_ms_median": med, "lookups_per_s": r_lookups / (med * 1e-3),
                         "whole_call_wall_s": round(wall, 4), "error": [float(ep[0]), float(et[0])],
                         "status": int(r.refine.status[0])}

    # ---- the restatement beside it
    if a.cpu_scans:
        m = min(a.cpu_scans, B)
        F = loc_ref.field(grid, 20)
        same = bool(np.array_equal(F, f.field))
        t0 = time.perf_counter()
        for b in range(m):
            _, bb = loc_ref.search(F, origin, cw, 20, seq.scans[b], centre[b], p.n_theta, p.d_theta, p.nx, p.ny, p.step)
            same = same and bb == tuple(int(v) for v in got[b])
        cpu_s = time.perf_counter() - t0
        gpu_s_per_scan = rep["search"]["d_cap_20_table_2B"]["ms_median"] * 1e-3 / B
        rep["restatement"] = {"scans": m, "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                              "cpu_s_per_scan": round(cpu_s / m, 3),
                              "cpu_lookups_per_s": p.n_theta * p.ny * p.nx * int(ss.lens[:m].sum()) / cpu_s,
                              "equal_answers": same, "gpu_over_cpu_per_scan": round((cpu_s / m) / gpu_s_per_scan, 1)}
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if a.cpu_scans and not rep["restatement"]["equal_answers"]:
        raise SystemExit("GPU result differs from the NumPy restatement")


if __name__ == "__main__":
    main()
