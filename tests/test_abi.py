"""CPU-side checks of the C-ABI boundary: the library loads (no GPU needed to
dlopen it) and exports every entry point include/slamhip.h declares, with the
ctypes table in slamhip/_abi.py covering all of them."""
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "slamhip.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", txt)))


def test_header_parses():
    names = declared()
    assert "slam_icp_batch_f64" in names and "slam_pgo_sgd_step_f64" in names
    assert "slam_gn_iteration_f64" in names


def test_library_exports_every_declared_symbol():
    from slamhip import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.fail(f"{_abi.LIB_PATH} not built (run __graft_entry__.build())")
    lib = _abi.lib()
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_ctypes_table_covers_header():
    from slamhip import _abi
    assert set(declared()) <= set(_abi.SIGNATURES), set(declared()) - set(_abi.SIGNATURES)


def test_host_only_calls():
    """Entry points that only validate arguments run without a GPU."""
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 100
    assert lib.slam_icp_max_query_points() >= 4096
    # shape validation fails loudly before any launch
    rc = lib.slam_icp_batch_f64(None, None, None, None, None, 4, 0.01, 100, 1e-4, 0, 10, 10, 0,
                                None, None, None, None, None)
    assert rc == -1 and b"null" in lib.slam_last_error()
    rc = lib.slam_kabsch2d_f64(None, None, 0, None, None, None)
    assert rc == -1
    assert lib.slam_pgo_sgd_work_size(10, 4) >= 3 * 10 + 3 * 4
    # the relaxation's launch plan: (in LDS, BR, shift, threads) per N, and the
    # forced plans; a force that cannot hold the graph is an error, not another launch
    from slamhip import pgo
    one = lambda br: {"in_lds": True, "rounds": br, "shift": 6, "threads": 64}      # noqa: E731
    wg = lambda sh: {"in_lds": False, "rounds": 1, "shift": sh, "threads": 256}     # noqa: E731
    for N, want in [(1, one(1)), (3, one(1)), (4096, one(1)), (4097, one(2)), (6144, one(2)), (6145, wg(6)),
                    (131072, wg(6)), (131073, wg(7)), (262144, wg(7)), (262145, wg(8)), (524288, wg(8)),
                    (524289, wg(9))]:
        assert pgo.sgd_plan(N) == want, N
    assert lib.slam_pgo_sgd_plan(0, None, None, None, None) == -1
    assert lib.slam_pgo_sgd_plan(100, None, None, None, None) == 0      # NULL outputs are allowed
    try:
        for bad in [(3, -1), (-2, -1), (0, 6), (1, 6), (-1, 6), (2, 5), (2, 13)]:
            assert lib.slam_pgo_sgd_force(*bad) == -1 and lib.slam_last_error(), bad
            assert pgo.sgd_plan(200) == one(1), bad      # a refused force changes nothing
        pgo.force_sgd_path(0)
        assert pgo.sgd_plan(4096) == one(1)
        for N in (4097, 6145):
            with pytest.raises(_abi.SlamHipError):
                pgo.sgd_plan(N)
        pgo.force_sgd_path(1)
        assert pgo.sgd_plan(200) == one(2) and pgo.sgd_plan(6144) == one(2)
        with pytest.raises(_abi.SlamHipError):
            pgo.sgd_plan(6145)
        pgo.force_sgd_path(2)
        assert pgo.sgd_plan(200) == wg(6) and pgo.sgd_plan(131073) == wg(7)
        pgo.force_sgd_path(2, 9)
        assert pgo.sgd_plan(2200) == wg(9) and pgo.sgd_plan(2048 * 512) == wg(9)
        with pytest.raises(_abi.SlamHipError):
            pgo.sgd_plan(2048 * 512 + 1)
    finally:
        pgo.force_sgd_path()
    assert pgo.sgd_plan(6145) == wg(6)
    # the occupancy-grid update refuses bad arguments before any launch (all arrays NULL here,
    # and the NULL check comes last): S, H, W, P, the odds, the cell width, the event-key range
    def grid_update(S=1, P=10, cw=0.25, H=5, W=7, kh=3, km=1):
        return lib.slam_grid_update_i8(None, None, S, None, P, 0.0, 0.0, cw, H, W, kh, km, None, None, None)
    EINVAL, ETOOBIG = -1, -3
    for kw, rc, word in [({"S": 0}, EINVAL, b"S=0"), ({"P": -1}, EINVAL, b"P=-1"), ({"H": 0}, EINVAL, b"H=0"),
                         ({"W": 0}, EINVAL, b"W=0"), ({"kh": 0}, EINVAL, b"odds"), ({"kh": 128}, EINVAL, b"odds"),
                         ({"km": 0}, EINVAL, b"odds"), ({"km": 128}, EINVAL, b"odds"),
                         ({"cw": 0.0}, EINVAL, b"cell_width"), ({"cw": float("nan")}, EINVAL, b"cell_width"),
                         ({"cw": -0.25}, EINVAL, b"cell_width"),
                         ({"H": 1 << 21, "W": 1 << 21}, ETOOBIG, b"event-key"),
                         ({"H": 1, "W": (1 << 22) - 1}, ETOOBIG, b"event-key"),
                         ({"P": 1 << 40}, ETOOBIG, b"event-key"),
                         ({}, EINVAL, b"null"), ({"P": 0}, EINVAL, b"null"),
                         ({"H": 1, "W": (1 << 22) - 2, "P": (1 << 40) - 1, "kh": 127, "km": 127}, EINVAL, b"null")]:
        assert grid_update(**kw) == rc and word in lib.slam_last_error(), (kw, lib.slam_last_error())
    assert lib.slam_grid_global_points_f64(None, None, 0, None, None, None, None, None) == EINVAL
    assert lib.slam_grid_global_points_f64(None, None, 3, None, None, None, None, None) == EINVAL
    assert b"null" in lib.slam_last_error()
    assert lib.slam_grid_work_size(3, 5, 7) >= 32 * 3 + 16 * 35
    n = lib.slam_icp_num_instances()
    assert n >= 4
    # instance chooser: smallest capacity covering the scan
    import ctypes
    b, q = ctypes.c_int32(), ctypes.c_int32()
    i = lib.slam_icp_selected_instance(1081)
    assert lib.slam_icp_instance_shape(i, ctypes.byref(b), ctypes.byref(q)) == 0
    assert b.value * q.value >= 1081
    # the cyclic reduction's latched A/B switches: none of them set in the
    # environment leaves the fused back-substitution's default bit alone
    if not any(k.startswith(("SLAMHIP_BCR_", "SLAMHIP_GN_")) for k in os.environ):
        assert lib.slam_gn_bcr_variant() == _abi.GN_VARIANT_FUSED_BACK
        assert lib.slam_gn_schur_supported() == 1
    assert lib.slam_gn_bcr_variant() == lib.slam_gn_bcr_variant()
