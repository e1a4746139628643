"""CPU self-checks of the one-step Gauss-Newton accuracy harness (gn_step.py):
every case has the block shape it names, the bound leaves plain SuperLU a
factor of ten to spare, and a 1e-6 .. 1e-4 defect of one edge's information
moves a step by five bounds or more (so the GPU tests of test_gn_step_gpu.py
would notice it).  No GPU."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import gn_step as gs

IDS = [c.name for c in gs.CASES]


@pytest.mark.parametrize("case", gs.CASES, ids=IDS)
def test_case_plan_shape(case):
    """(a) planned in natural order the span graph has W = 3 dmax + 2 and the
    block rows, block count, remainder and border size of the case table."""
    p = gs.case_plan(case)
    assert p.ordering == "given" and p.nv == 3 * (case.N - 1) <= 900
    assert p.W == case.W == 3 * case.dmax + 2
    assert p.nv - p.nv_band == case.nbd == 3 * len(case.border)
    assert gs.block_shape(p) == (case.wb, case.nb, case.rem)
    assert all(p.node_col[list(case.border)] >= p.nv_band)
    _, ea, eb, _ = gs.case_graph(case)
    d = (eb - ea)[case.N - 1:]
    assert len(d) == case.n_loops and d[0] == case.dmax and d.min() >= 2 and d.max() == case.dmax
    assert ea[case.N - 1:].min() >= 1


def test_block_shape_follows_the_library():
    """gs.block_shape restates slam_gn_bcr_block_rows (a host-only call)."""
    from slamhip import _abi
    lib = _abi.lib()
    for case in gs.CASES:
        p = gs.case_plan(case)
        assert lib.slam_gn_bcr_block_rows(p.nv_band, p.W) == case.wb, case.name


def test_cases_cover_the_block_shapes():
    """Every register tile 1..6 with at least 4 blocks, the smallest block
    counts (4, 5, 2^k + 1), a band that is a whole number of blocks, and
    borders of one and two RHS column tiles."""
    shapes = {(c.wb, c.nb) for c in gs.CASES}
    assert {c.wb for c in gs.CASES if c.nb >= 4} >= {16, 32, 48, 64, 80, 96}
    assert {4, 5, 17} <= {nb for _, nb in shapes} and (0, 3) in shapes
    assert any(c.rem == 0 and c.wb for c in gs.UNBORDERED) and any(c.rem == 1 for c in gs.CASES)
    assert sorted(c.nbd for c in gs.BORDERED) == [3, 6, 15, 30]


@pytest.mark.parametrize("case", gs.CASES, ids=IDS)
def test_bound_holds_for_superlu_and_sees_a_defect(case):
    """(b) plain SuperLU lies at least 10x inside the bound; (c) the first
    loop edge's information times (1 + defect) moves the step by at least 5x
    the bound (defect 1e-6, or the case table's larger power of ten <= 1e-4
    where 1e-6 moves it by less)."""
    guess, ea, eb, tf = gs.case_graph(case)
    ref = gs.reference_step(guess, ea, eb, tf)
    bound = gs.step_bound(ref, guess)
    e_lu = float(np.abs(ref.x_lu - ref.x).max())
    move = float(np.abs(gs.defect_step(case, case.defect) - ref.x).max())
    print(f"{case.name}: cond {ref.cond:.2e} |x| {ref.xnorm:.2e} bound {bound:.2e} superlu {e_lu:.2e} "
          f"({bound / max(e_lu, 1e-300):.0f}x inside) defect {case.defect:g} moves {move / bound:.1f} bounds")
    assert 1e-13 <= bound <= 3e-9
    assert 10 * e_lu <= bound
    assert case.defect in (1e-6, 1e-5, 1e-4)
    assert move >= 5 * bound
    if case.defect > 1e-6:   # the larger factor is needed: the next smaller one is not enough
        assert np.abs(gs.defect_step(case, case.defect / 10) - ref.x).max() < 5 * bound


def test_reference_step_is_a_solution():
    """The refined reference solves the oracle's system to a residual far
    below plain SuperLU's, and agrees with the oracle's own iteration."""
    import gn_oracle as go
    case = gs.BY_NAME["N49_d10"]
    guess, ea, eb, tf = gs.case_graph(case)
    ref = gs.reference_step(guess, ea, eb, tf)
    H, b, _, chi2 = go.build_system(np.array(guess), ea.astype(np.int64), eb.astype(np.int64),
                                    go.edge_measurements(tf), go.information(ea, eb))
    Hl, bl = H.toarray().astype(np.longdouble), b.astype(np.longdouble)
    r_ref = float(np.abs(-bl - Hl @ ref.x.astype(np.longdouble)).max())
    r_lu = float(np.abs(-bl - Hl @ ref.x_lu.astype(np.longdouble)).max())
    assert r_ref <= 4 * gs.EPS * float(np.abs(Hl).sum(1).max()) * ref.xnorm and r_ref <= r_lu
    assert chi2 == ref.chi2
    out, _, _ = go.gn_iteration(np.array(guess), ea, eb, tf)
    d = out - guess
    d[:, 2] = go.wrap(d[:, 2])
    assert np.abs(d[1:].ravel() - ref.x).max() <= gs.step_bound(ref, guess)


def test_variant_table():
    """Every switch of the table is one the library or the planner reads."""
    for name, (env, mask, schur_ok, _) in gs.VARIANTS.items():
        assert set(env) <= set(gs.SWITCHES)
        assert schur_ok == (0 if mask & (gs.CHOL | gs.LEGACY) else 1)
    env = gs.variant_env("split3")
    assert env["SLAMHIP_GN_SPLIT_MIN"] == "3" and "SLAMHIP_BCR_CHOL" not in env
    assert gs.expected_path(gs.BY_NAME["N70_d4_b2"], "chol") == "bordered"
    assert gs.expected_path(gs.BY_NAME["N70_d4_b2"], "split1") == "schur"
    assert gs.expected_path(gs.BY_NAME["N70_d4"], "no_schur") == "plain"


_MASK_PROBE = """
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
print(lib.slam_gn_bcr_variant(), lib.slam_gn_schur_supported())
"""


@pytest.mark.parametrize("name", [n for n in gs.VARIANTS if n != "no_schur"])
def test_variant_mask_is_latched_from_the_environment(name):
    """slam_gn_bcr_variant (host only) in a fresh process per environment."""
    from slamhip import _abi
    ctypes.CDLL(_abi.LIB_PATH)   # loads here: a failure below is the child's own
    r = subprocess.run([sys.executable, "-c", _MASK_PROBE, _abi.LIB_PATH], env=gs.variant_env(name),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _, mask, schur_ok, _ = gs.VARIANTS[name]
    assert r.stdout.split() == [str(mask), str(schur_ok)]
