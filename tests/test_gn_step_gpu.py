"""Every Gauss-Newton solver path, one step at a time, to rounding.

gn_step.py has the harness, the bound and the cases.  The paths a process can
switch between run here in process (the default, slam_gn_set_solver(1) and
(2), slam_gn_set_fused_back(0)); the ones the library latches from the
environment at first use (the Cholesky, legacy and odd-MFMA cyclic reductions,
the pre-inverting split, the per-level back-substitution as a default, the
bordered entry point without the Schur accumulation) each run in a fresh child
process, one at a time, which checks through slam_gn_bcr_variant() that it
really latched its switches.  profiles/gn_step_accuracy.md keeps the ratios."""
import json
import os
import subprocess
import sys

import pytest

import gn_step as gs
from conftest import REPO

pytestmark = pytest.mark.gpu

STEPS = 3


@pytest.fixture
def lib():
    """The library in its default state (no latched A/B switch), restored after the test."""
    from slamhip import _abi
    h = _abi.lib()
    assert h.slam_gn_bcr_variant() == gs.FUSED and "SLAMHIP_GN_SCHUR" not in os.environ, \
        "this process latched a solver switch from its environment: the in-process paths need a default one"
    assert h.slam_gn_get_solver() == 0 and h.slam_gn_get_fused_back() == 1
    yield h
    h.slam_gn_set_solver(0)
    h.slam_gn_set_fused_back(1)


def _run(lib, case, schur):
    """gpu_steps of one case in this process; the plan must name the case's
    block rows (so no case silently runs another solver) and, bordered, take
    the Schur entry point (schur) or slam_gn_iteration_bordered_f64."""
    plan = gs.case_plan(case)
    assert lib.slam_gn_bcr_block_rows(plan.nv_band, plan.W) == case.wb
    assert plan.nv - plan.nv_band == case.nbd
    if case.border:
        assert (plan.pslot is not None) == schur
    _, steps = gs.gpu_steps(case, STEPS, plan)
    gs.check_steps(case, steps)
    return steps


@pytest.mark.parametrize("case", gs.CASES, ids=[c.name for c in gs.CASES])
def test_step_default(lib, case):
    """The default solver: explicit-inverse cyclic reduction (band Cholesky
    below 4 blocks), borders by the Schur accumulation and the fused
    back-substitution."""
    _run(lib, case, True)


@pytest.mark.parametrize("case", gs.UNBORDERED, ids=[c.name for c in gs.UNBORDERED])
def test_step_band_cholesky(lib, case):
    """slam_gn_set_solver(1): the band Cholesky at every band width (it takes no border)."""
    assert lib.slam_gn_set_solver(1) == 0 and lib.slam_gn_get_solver() == 1
    _run(lib, case, False)


@pytest.mark.parametrize("case", gs.CASES, ids=[c.name for c in gs.CASES])
def test_step_forced_reduction(lib, case):
    """slam_gn_set_solver(2): the cyclic reduction wherever the band allows it."""
    assert lib.slam_gn_set_solver(2) == 0
    _run(lib, case, True)


@pytest.mark.parametrize("case", gs.BORDERED, ids=[c.name for c in gs.BORDERED])
def test_step_per_level_back_substitution(lib, case):
    """slam_gn_set_fused_back(0): the Schur path with one back-substitution launch per level."""
    assert lib.slam_gn_set_fused_back(0) == 0 and lib.slam_gn_get_fused_back() == 0
    _run(lib, case, True)


# ---- one child process per latched variant ----------------------------------
# One clean child run of all 18 cases x 3 steps was measured at 2.8 - 2.9 s on
# an MI355X host (0.9 s of it the cases, the rest Python and torch start-up);
# the limit is about 5x that.
CHILD_TIMEOUT_S = 15
_ABNORMAL = []   # the first variant whose child ended abnormally: no later child is started


def _child(name):
    if _ABNORMAL:
        pytest.fail(f"not started: the child of variant {_ABNORMAL[0]!r} ended abnormally")
    cmd = [sys.executable, os.path.join("tests", "gn_step.py"), name, str(STEPS)]
    try:
        r = subprocess.run(cmd, cwd=REPO, env=gs.variant_env(name), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _ABNORMAL.append(name)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"variant {name}: killed at its {CHILD_TIMEOUT_S} s limit\n{err[-4000:]}")
    if r.returncode != 0:
        # a signal, an abort (134), a segmentation fault (139), a time limit
        # (124, 137) or any other unexpected end: nothing more goes to the GPU
        _ABNORMAL.append(name)
        pytest.fail(f"variant {name}: child exit status {r.returncode}\n{r.stderr[-4000:]}")
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert recs and recs[-1].get("done") == name, r.stderr[-4000:]
    assert recs[-1]["mask"] == gs.VARIANTS[name][1]
    return recs[:-1]


def _check(name, recs):
    for rec in recs:
        print(f"{name} {rec['case']} step {rec['step']} [{rec['path']}, {rec['wb']} rows]: err {rec['err']:.3e} "
              f"bound {rec['bound']:.3e} ratio {rec['ratio']:.3f}")
    cases = gs.variant_cases(name)
    assert [(rec["case"], rec["step"]) for rec in recs] == [(c.name, i) for c in cases for i in range(STEPS)]
    for rec in recs:
        case = gs.BY_NAME[rec["case"]]
        assert rec["wb"] == case.wb and rec["path"] == gs.expected_path(case, name), rec
        assert not rec["fixed_moved"], rec
        assert abs(rec["chi2"] - rec["chi2_ref"]) <= rec["chi2_rtol"] * rec["chi2_ref"], rec
        assert rec["err"] <= rec["bound"], rec
        assert rec.get("bordered_ratio", 0.0) <= 1.0, rec


_DEFAULT = []


def _default_child():
    """The default child's records, run once (the split's identity checks compare with them)."""
    if not _DEFAULT:
        _DEFAULT.append(None)   # a failed run is not repeated
        _DEFAULT[0] = _child("default")
    if _DEFAULT[0] is None:
        pytest.fail("the default child failed in an earlier test")
    return _DEFAULT[0]


def test_step_default_child():
    """No switch set: the child harness itself, and the records the split variants are compared with."""
    _check("default", _default_child())


@pytest.mark.parametrize("name", ["chol", "chol_odd_mfma", "legacy", "unfused_back", "no_schur"])
def test_step_latched_variant(name):
    """SLAMHIP_BCR_CHOL=1 (MFMA even / top kernels), with SLAMHIP_BCR_ODD_MFMA=1
    (bcr_odd_mfma_kernel), SLAMHIP_BCR_LEGACY=1 (register elimination) — under
    these three a bordered case takes slam_gn_iteration_bordered_f64 through
    bcr_load_kernel's multi-column form —, SLAMHIP_GN_FUSED_BACK=0 and
    SLAMHIP_GN_SCHUR=0 (bordered cases; the latter with border_solve_kernel on
    the assembly's direct block layout)."""
    _check(name, _child(name))


@pytest.mark.parametrize("name", ["split1", "split3"])
def test_step_split_inversion(name):
    """SLAMHIP_GN_SPLIT_MIN=1 pre-inverts every level (inv_kernel overwrites
    D_i with its inverse in place); =3 mixes: on the 13-block cases the levels
    of 6 and 3 odd blocks pre-invert and those of 2 and 1 do not.

    The split does the same operations in the same order, so beside the bound
    its poses and chi2 are the unsplit default's bit for bit, step by step,
    for the plain, the Schur and (the children's second run of every bordered
    case with SLAMHIP_GN_SCHUR=0 at plan time) the bordered entry point.
    The identity ADVICE.md round 6 item 4 words as "the bordered and the Schur
    plan" giving EACH OTHER's bits does not hold: on the default path already
    (measured, every bordered case and step) the two entry points differ in
    the last bits, as include/slamhip.h says ("to rounding"); between them
    the bound is the check."""
    recs = _child(name)
    _check(name, recs)
    base = _default_child()
    _check("default", base)
    key = [(r["case"], r["step"]) for r in recs]
    assert key == [(r["case"], r["step"]) for r in base]
    assert [r["digest"] for r in recs] == [r["digest"] for r in base]
    twin = [r.get("bordered_digest") for r in recs]
    assert twin == [r.get("bordered_digest") for r in base]
    assert sum(t is not None for t in twin) == STEPS * len(gs.BORDERED)
