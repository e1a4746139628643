#!/usr/bin/env python3
"""Times the batched descriptor matcher (slam_desc_match_batch).

* Workload: --images images (default 1,000) of --per-image random 32-byte
  descriptors (default 500) along laps of a circle (the pose generator of
  tests/test_lcd_gpu.py, one image per pose), every pair (i, j >= start[i])
  of the reference's start rule at --min-dist-along-path (default 5):
  slamhip.desc.image_starts, as similarity_matrix launches them (scores and
  counts only, n_matches 20).
* Device time per metric: descriptors, pair lists and outputs resident, HIP
  events around each call after --warmup calls, the median of --repeats.
  Reported with pairs/s and distance evaluations/s (hamming evaluates every
  distance twice, once per direction).
* The bwd A/B (hamming): the swapped second pass against the LDS atomicMin
  variant (slam_desc_set_bwd) on the first --ab-pairs pairs, same protocol,
  equal outputs asserted.
* Beside it the NumPy restatement (tests/desc_ref.py) on the first
  --host-pairs pairs, BLAS limited to one thread, with equal answers asserted.

Needs a GPU: there is no fallback.

    python tools/desc_time.py --out profiles/desc_time.json
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

N_MATCHES = 20


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def time_pairs(ds, qi, ti, metric, warmup, repeats, bwd=0):
    """Median device milliseconds of one slam_desc_match_batch call over the
    pairs, on resident data; also the scores and counts it wrote."""
    from slamhip import _abi, desc
    from slamhip import device as dv
    t = dv.require_gpu()
    L = _abi.lib()
    B = len(qi)
    d_qi, d_ti = dv.to_dev(qi, np.int32), dv.to_dev(ti, np.int32)
    work = dv.empty((int(L.slam_desc_work_size(B, int(ds.counts.max()), N_MATCHES)),), np.uint8)
    out_s, out_c = dv.empty((B,), np.float64), dv.empty((B,), np.int32)
    _abi.check(L.slam_desc_set_bwd(bwd), "slam_desc_set_bwd")

    def timed():
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        _abi.check(L.slam_desc_match_batch(dv.ptr(ds.d_desc), dv.ptr(ds.d_off), len(ds), dv.ptr(d_qi), dv.ptr(d_ti), B,
                                           desc.METRICS[metric], N_MATCHES, dv.ptr(out_s), dv.ptr(out_c), None,
                                           dv.ptr(work), dv.stream_handle()), "slam_desc_match_batch")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    try:
        for _ in range(warmup):
            timed()
        ms = [timed() for _ in range(repeats)]
        _abi.check(L.slam_desc_status(dv.stream_handle()), "slam_desc_match_batch")
    finally:
        L.slam_desc_set_bwd(0)
    med = float(np.median(ms))
    dirs = 2 if metric == "hamming" else 1
    dist = int((ds.counts[qi] * ds.counts[ti]).sum()) * dirs
    rep = {"metric": metric, "bwd": ("swapped pass", "LDS atomicMin")[bwd] if metric == "hamming" else None,
           "pairs": B, "distance_evaluations": dist, "gpu_ms": [round(m, 3) for m in ms],
           "gpu_ms_median": round(med, 3),
           "pairs_per_s": B / (med * 1e-3), "distances_per_s": dist / (med * 1e-3)}
    return rep, out_s.cpu().numpy(), out_c.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--per-image", type=int, default=500)
    ap.add_argument("--min-dist-along-path", type=float, default=5)
    ap.add_argument("--ab-pairs", type=int, default=50000)
    ap.add_argument("--host-pairs", type=int, default=48)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", help="commit to record when the tree is not a git checkout")
    ap.add_argument("--out", help="also write the JSON report here")
    a = ap.parse_args(argv)

    import desc_ref
    from test_lcd_gpu import lap_poses
    from threadpoolctl import threadpool_limits
    from slamhip import desc
    from slamhip import device as dv
    t = dv.require_gpu()
    rng = np.random.default_rng(a.seed)
    descs = [rng.integers(0, 256, (a.per_image, 32), dtype=np.uint8) for _ in range(a.images)]
    ds = desc.DescriptorSet(descs)
    start = np.minimum(desc.image_starts(lap_poses(a.images), a.min_dist_along_path, 1), a.images)
    qi = np.repeat(np.arange(a.images), a.images - start)
    ti = np.concatenate([np.arange(s, a.images) for s in start])
    rep = {"tool": "desc_time", "commit": a.commit or commit(), "device": t.cuda.get_device_name(0),
           "images": a.images, "descriptors_per_image": a.per_image, "n_matches": N_MATCHES,
           "min_dist_along_path": a.min_dist_along_path,
           "poses": "laps of a circle of radius 3 m, step 0.05 m (tests/test_lcd_gpu.py lap_poses, seed 11)",
           "protocol": f"HIP events, {a.warmup} warm-up calls, median of {a.repeats}, data resident, no rows",
           "match": [], "bwd_ab": []}
    results = {}
    for metric in desc_ref.METRICS:
        r, s, c = time_pairs(ds, qi, ti, metric, a.warmup, a.repeats)
        rep["match"].append(r)
        results[metric] = (s, c)
    n_ab = min(a.ab_pairs, len(qi))
    ab = [time_pairs(ds, qi[:n_ab], ti[:n_ab], "hamming", a.warmup, a.repeats, bwd) for bwd in (0, 1)]
    rep["bwd_ab"] = [r for r, _, _ in ab]
    rep["bwd_ab_equal"] = bool(np.array_equal(ab[0][1], ab[1][1]) and np.array_equal(ab[0][2], ab[1][2]))
    rep["host"] = []
    n_host = min(a.host_pairs, len(qi))
    with threadpool_limits(limits=1):
        for metric in desc_ref.METRICS:
            t0 = time.perf_counter()
            s, c, _ = desc_ref.match_pairs(descs, qi[:n_host], ti[:n_host], N_MATCHES, metric)
            host_s = time.perf_counter() - t0
            equal = bool(np.array_equal(s, results[metric][0][:n_host]) and
                         np.array_equal(c, results[metric][1][:n_host]))
            rep["host"].append({"metric": metric, "pairs": n_host, "numpy_restatement_s": round(host_s, 4),
                                "pairs_per_s": n_host / host_s, "blas_threads": 1, "device_equals_host": equal})
    line = json.dumps(rep)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not rep["bwd_ab_equal"] or not all(h["device_equals_host"] for h in rep["host"]):
        raise SystemExit("the device answers differ (bwd variants, or from the NumPy restatement)")


if __name__ == "__main__":
    main()
