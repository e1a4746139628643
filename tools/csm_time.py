#!/usr/bin/env python3
"""Times the correlative scan matcher (slam_csm_batch) at the loop-closure
workload's own size: --pairs candidate pairs (default 1,000) of 1081-beam
scans from synthetic.make_loop_sequence, default CsmParams, every input and
the workspace resident on the device, HIP events around each call after a
warm-up call.  Reports milliseconds per call and table look-ups per second
(look-ups = pairs x n_theta x ny x nx x query points, counted from the
shapes), and runs the NumPy restatement (tests/csm_ref.py) on --cpu-pairs of
the same pairs as the "CPU beside it" figure, checking that the GPU's answer
for those pairs is the restatement's.  Needs a GPU: there is no fallback.

    python tools/csm_time.py --out profiles/csm_time.json
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
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--beams", type=int, default=1081)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=16, help="pairs the NumPy restatement runs (0: none)")
    ap.add_argument("--ab", action="store_true",
                    help="also time the byte-gather form of the score kernel (slam_csm_set_gather(1)), alternating")
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)

    import csm_ref
    from slamhip import _abi, csm, synthetic
    from slamhip import device as dv
    from slamhip.icp import ScanSet
    t = dv.require_gpu()

    # every lap position once: pair b = (scan b, scan b + per_lap), the later scan the query
    probe = synthetic.make_loop_sequence(1, seed=a.seed, n_beams=8)
    seq = synthetic.make_loop_sequence(probe.per_lap + a.pairs, seed=a.seed, n_beams=a.beams, loop_every=1)
    pairs = seq.loop_pairs[:a.pairs]
    B = len(pairs)
    assert B == a.pairs, (B, a.pairs)
    src, dst = pairs[:, 1].astype(np.int32), pairs[:, 0].astype(np.int32)
    p = csm.CsmParams()
    ss = ScanSet(seq.scans)
    centre = np.zeros((B, 3))
    rot = csm.rotations(centre, p)
    L = _abi.lib()
    dev = ss.device
    d_src, d_dst = dv.to_dev(src, np.int32, dev), dv.to_dev(dst, np.int32, dev)
    d_centre, d_rot = dv.to_dev(centre, np.float64, dev), dv.to_dev(rot, np.float64, dev)
    n_work = int(L.slam_csm_work_size(B, p.G, p.n_theta, p.ny, p.nx))
    work = dv.empty((n_work,), np.uint8, dev)
    best = dv.empty((B, 4), np.int32, dev)

    def call():
        _abi.check(L.slam_csm_batch(dv.ptr(ss.pts), dv.ptr(ss.scan_off), dv.ptr(d_src), dv.ptr(d_dst),
                                    dv.ptr(d_centre), dv.ptr(d_rot), B, p.res, p.G, p.n_theta, p.nx, p.ny,
                                    dv.ptr(best), None, dv.ptr(work), dv.stream_handle()), "slam_csm_batch")

    def timed(width):
        _abi.check(L.slam_csm_set_gather(width), "slam_csm_set_gather")
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        _abi.check(L.slam_csm_set_gather(4), "slam_csm_set_gather")
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(4)
        if a.ab:
            timed(1)
    ms, ms_byte = [], []
    for _ in range(a.repeats):   # the A/B alternates the two forms in one process
        ms.append(timed(4))
        if a.ab:
            ms_byte.append(timed(1))
    lookups = int(p.n_theta) * p.ny * p.nx * int(ss.lens[src].sum())
    med = float(np.median(ms))
    got = best.cpu().numpy()
    rep = {"tool": "csm_time", "commit": a.commit or commit(), "device": t.cuda.get_device_name(0), "pairs": B,
           "beams": a.beams, "query_points": int(ss.lens[src].sum()), "params": p.__dict__,
           "workspace_MiB": round(n_work / 2**20, 1), "lookups": lookups,
           "gpu_ms": [round(m, 3) for m in ms], "gpu_ms_median": round(med, 3),
           "gpu_ms_per_pair": round(med / B, 4), "gpu_lookups_per_s": lookups / (med * 1e-3),
           "mean_score_fraction": float(np.mean(got[:, 0] / (2.0 * ss.lens[src])))}
    if a.ab:
        rep.update({"byte_gather_ms": [round(m, 3) for m in ms_byte],
                    "byte_gather_ms_median": round(float(np.median(ms_byte)), 3),
                    "byte_over_dword": round(float(np.median(ms_byte)) / med, 3)})

    if a.cpu_pairs:
        n = min(a.cpu_pairs, B)
        t0 = time.perf_counter()
        same = True
        for b in range(n):
            _, score, index, _ = csm_ref.match(seq.scans[src[b]], seq.scans[dst[b]], **p.__dict__)
            same = same and (score, *index) == tuple(int(v) for v in got[b])
        cpu_s = time.perf_counter() - t0
        cpu_lookups = int(p.n_theta) * p.ny * p.nx * int(ss.lens[src[:n]].sum())
        rep.update({"cpu_pairs": n, "cpu_threads": os.environ.get("OMP_NUM_THREADS"),
                    "cpu_s_per_pair": round(cpu_s / n, 3), "cpu_lookups_per_s": cpu_lookups / cpu_s,
                    "cpu_matches_gpu": bool(same),
                    "gpu_over_cpu_per_pair": round((cpu_s / n) / (med * 1e-3 / B), 1)})
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.cpu_pairs and not rep["cpu_matches_gpu"]:
        raise SystemExit("GPU result differs from the NumPy restatement")


if __name__ == "__main__":
    main()
