"""The pruned screen's group search (csrc/icp_kernels.hip nn_window_pruned step
3: the fused bounds reduction, live masks, visit batches) at the shapes where it
can go wrong.  The search must stay invisible: mode 2 (pruned) equals mode 0 (exact
fp64 scan) bit for bit, and both equal the CPU oracle in iteration counts and
to 1e-9 in the transforms.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, homog

pytestmark = pytest.mark.gpu
TOL = 1e-9
EPS, ITERS, STOP = 1e-12, 20, 1e-14   # as test_small_and_degenerate_scans: every pair runs many iterations
# The outlier scans keep the pipeline's rule (stop when the error moves by less than 1e-4): their error is
# dominated by the outliers' ~1e2 m^2 terms, so a 1e-14 threshold would compare rounding noise of the sums
OUTLIER_PARAMS = (0.05, 100, 1e-4)


@pytest.fixture(scope="module")
def k():
    from slamhip import icp as kk
    return kk


@pytest.fixture(scope="module")
def lib():
    from slamhip import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def oracle():
    import icp_oracle
    return icp_oracle


def _instances(lib):
    out = []
    b, q = ctypes.c_int32(), ctypes.c_int32()
    for i in range(lib.slam_icp_num_instances()):
        lib.slam_icp_instance_shape(i, ctypes.byref(b), ctypes.byref(q))
        out.append((b.value, q.value))
    return out


def _smallest_instance(shapes, n1):
    fit = [(b * q, i) for i, (b, q) in enumerate(shapes) if b * q >= n1]
    return min(fit)[1]


def test_fused_reduction_against_a_serial_loop(tmp_path):
    """tools/check_wave_reduce.hip: wave_group_bounds on one 64-lane workgroup
    against a serial host loop, over the active-lane sets (none, lane 0, lane
    63, one lane per row, one full row, lanes 31 and 32, all) and value
    patterns (both signs, +-0, equal values, FLT_MAX, windows at both ends)."""
    exe = str(tmp_path / "check_wave_reduce")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "icp-slam-with-loop-closure_amd", "csrc"),
                    os.path.join(REPO, "tools", "check_wave_reduce.hip"), "-o", exe],
                   check=True, timeout=120, capture_output=True)
    r = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "check_wave_reduce: 35 cases, 0 mismatches", r.stdout + r.stderr


N1S = (1, 2, 63, 64, 65, 67, 128, 129)
N2S = (33, 97, 257, 512, 520, 1081)   # nsub 16, 32, 72, 128, 136, 136: partial first / second / third box pass


def _uniform_cases():
    """Unstructured uniform clouds (every query is active), every n1 x n2, and
    the duplicate-point cloud of test_small_and_degenerate_scans (first-index
    ties between a window and a visited sub-chunk)."""
    rng = np.random.default_rng(2718)
    cases = []
    for n1 in N1S:
        for n2 in N2S:
            pc2 = rng.uniform(-3, 3, size=(n2, 2))
            pc1 = pc2[rng.integers(0, n2, n1)] + rng.normal(0, 0.05, size=(n1, 2))
            cases.append((pc1, pc2))
    dup = rng.uniform(-2, 2, size=(40, 2))
    dup = np.concatenate([dup, dup[::3], dup[5:9]])   # exact duplicates in pc2
    cases.append((dup[:30] + 0.01, dup))
    return cases


def _outlier_cases():
    """A structured room scan (nearly every query settles in its window) with 1
    to 5 outlier queries moved far (> 1 m) from every candidate, at indices
    that land in lanes 0, 16, 63 and 32 of group 0 and lane 0 of group 1: a few
    active lanes per group in every iteration."""
    from slamhip import se2, synthetic
    seq = synthetic.make_sequence(2, seed=41)
    init = se2.pose_to_mat(seq.odometry[1] - seq.odometry[0])
    idx = [0, 16, 63, 64, 32]
    cases = []
    for n in range(1, 6):
        pc1 = seq.scans[1].copy()
        for j in idx[:n]:
            pc1[j] = [14.0 + 3.0 * j / 64.0, 12.0 - j / 16.0]   # the room is 10 m x 8 m: > 1 m past every return
        cases.append((pc1, seq.scans[0], init))
    return cases


@pytest.fixture(scope="module")
def uniform_ref(oracle):
    cases = _uniform_cases()
    ref = []
    for pc1, pc2 in cases:
        h, _ = oracle.icp(homog(pc1), homog(pc2), np.eye(3), EPS, ITERS, STOP)
        ref.append((len(h) - 1, h[-1], oracle.correspondences(homog(pc1), homog(pc2))))
    return cases, ref


@pytest.fixture(scope="module")
def outlier_ref(oracle):
    cases = _outlier_cases()
    ref = []
    for pc1, pc2, init in cases:
        h, _ = oracle.icp(homog(pc1), homog(pc2), init.copy(), *OUTLIER_PARAMS)
        ref.append((len(h) - 1, h[-1]))
    return cases, ref


def _run_modes(k, lib, inst, scans, src, dst, inits, params=(EPS, ITERS, STOP)):
    """(mode 0, mode 2) results with histories and first-step correspondences on a forced instance."""
    outs = []
    try:
        assert lib.slam_icp_force_instance(inst) == 0
        for mode in (0, 2):
            assert lib.slam_icp_set_screen(mode) == 0
            res = k.icp_batch(scans, src, dst, inits, epsilon=params[0], max_iters=params[1],
                              stopping_thresh=params[2], history=True)
            _, corr, _ = k.icp_step(scans, src, dst, inits)
            outs.append((res, corr))
    finally:
        lib.slam_icp_force_instance(-1)
        lib.slam_icp_set_screen(2)
    return outs


def _assert_identical(a, b, tag):
    (ra, ca), (rb, cb) = a, b
    assert np.array_equal(ra.iters, rb.iters), tag
    assert np.array_equal(ra.tf, rb.tf) and np.array_equal(ra.err, rb.err), tag
    for j, (h0, h1) in enumerate(zip(ra.hist, rb.hist)):
        assert np.array_equal(h0, h1), (tag, j)
    for j, (c0, c1) in enumerate(zip(ca, cb)):
        assert np.array_equal(c0, c1), (tag, j)


@pytest.mark.parametrize("which", ["smallest", "256x5"])
def test_uniform_clouds_modes_identical(k, lib, uniform_ref, which):
    cases, ref = uniform_ref
    shapes = _instances(lib)
    groups = {}
    for c, (pc1, _) in enumerate(cases):
        inst = shapes.index((256, 5)) if which == "256x5" else _smallest_instance(shapes, len(pc1))
        groups.setdefault(inst, []).append(c)
    if which == "smallest":
        assert len(groups) >= 3   # 64x1, 64x2 and the instance of 129 queries
    for inst, members in groups.items():
        scans = [a for c in members for a in cases[c]]
        B = len(members)
        src, dst = np.arange(0, 2 * B, 2), np.arange(1, 2 * B, 2)
        exact, pruned = _run_modes(k, lib, inst, scans, src, dst, np.stack([np.eye(3)] * B))
        _assert_identical(exact, pruned, shapes[inst])
        res, corr = pruned
        for j, c in enumerate(members):
            its, tf, cr = ref[c]
            tag = (shapes[inst], len(cases[c][0]), len(cases[c][1]))
            assert res.iters[j] == its, tag
            assert np.allclose(res.tf[j], tf, rtol=0, atol=TOL), tag
            assert np.array_equal(corr[j], cr), tag


@pytest.mark.parametrize("which", ["smallest", "256x5"])
def test_few_active_queries_modes_identical(k, lib, outlier_ref, which):
    cases, ref = outlier_ref
    shapes = _instances(lib)
    inst = shapes.index((256, 5)) if which == "256x5" else _smallest_instance(shapes, 1081)
    scans = [a for pc1, pc2, _ in cases for a in (pc1, pc2)]
    B = len(cases)
    src, dst = np.arange(0, 2 * B, 2), np.arange(1, 2 * B, 2)
    exact, pruned = _run_modes(k, lib, inst, scans, src, dst, np.stack([c[2] for c in cases]), OUTLIER_PARAMS)
    _assert_identical(exact, pruned, shapes[inst])
    res, _ = pruned
    assert res.iters.min() > 3
    for j, (its, tf) in enumerate(ref):
        assert res.iters[j] == its, (shapes[inst], j)
        assert np.allclose(res.tf[j], tf, rtol=0, atol=TOL), (shapes[inst], j)


def test_c3_slice_schedule_identity_and_oracle(k, lib, oracle):
    """64 consecutive pairs of the C3 stream (seed 2025, 1081 beams; a slice of
    the 10,001-scan sequence itself: a shorter sequence is not its prefix): the
    default two-phase schedule (its pair threshold lowered to 1, or 64 pairs
    would take the single launch anyway) and one launch are bit-identical; 8
    sampled pairs equal the oracle."""
    from slamhip import se2, synthetic
    n, first = 64, 2000
    full = synthetic.make_sequence(10001, seed=2025, n_beams=1081)
    scans = full.scans[first:first + n + 1]
    odo = full.odometry[first:first + n + 1]
    inits = np.stack([se2.pose_to_mat(odo[i] - odo[i - 1]) for i in range(1, n + 1)])
    src, dst = np.arange(1, n + 1), np.arange(0, n)
    try:
        assert lib.slam_icp_set_schedule(-1, 1) == 0   # the default probe length, phased from one pair on
        a = k.icp_batch(scans, src, dst, inits, epsilon=0.05, max_iters=100, history=True)
        assert lib.slam_icp_set_schedule(0, 1024) == 0
        b = k.icp_batch(scans, src, dst, inits, epsilon=0.05, max_iters=100, history=True)
    finally:
        lib.slam_icp_set_schedule(-1, 1024)
        lib.slam_icp_set_schedule_auto(1)
    assert a.iters.max() > 3   # some pairs outlive the probe phase and are resumed
    assert np.array_equal(a.iters, b.iters)
    assert np.array_equal(a.tf, b.tf) and np.array_equal(a.err, b.err)
    for h0, h1 in zip(a.hist, b.hist):
        assert np.array_equal(h0, h1)
    for p in range(0, n, 8):
        h, _ = oracle.icp(homog(scans[p + 1]), homog(scans[p]), inits[p].copy(), 0.05, 100)
        assert a.iters[p] == len(h) - 1, p
        assert np.abs(a.tf[p] - h[-1]).max() <= TOL, p
