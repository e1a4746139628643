"""GPU parity of the scan signatures (csrc/sig_kernels.hip) on every
``sig_scan_kernel<S>`` instance and on every edge of its gate, screen, sorted
list and launch shape, against the NumPy restatement (tests/sig_ref.py) and
hand-written numbers.

tests/test_sig_gpu.py launches four of the sixteen ``sig_scan_kernel<S>`` (S =
8, 64, 72, 128) on seeded masks; here the cases of tests/sig_cases.py reach all
sixteen, S = 8, 16, ..., 128, through ``SigParams(sectors=S)``, on the build
side (a point on every sector's centre, every sector in one ring, points 1e-9
rad either side of four sector boundaries, infinities, NaN, a denormal, -0.0)
and on the match side (an aperiodic signature against its rolls by 0, 1, S / 2,
S - 1, 63 and 64, exact and three bits off, from given masks and from a cloud
that realises them).  Further: periodic signatures whose best shift ties between
the first and the second pass; pairs exactly on the gate and on the ring-count
screen and one step outside, full against empty (d = 4,096, ring counts of 128)
at thresholds up to (2^31 - 1) / (2^31 - 1), and pairs whose products a 32-bit
multiply decides the other way, each with the screen on and off; row 0 of 520
signatures with candidates only where placed (ascending, descending, equal
across the tile and chunk edges, the best in the 8-column last chunk, exactly K
and K + 1 of them) at K = 1, 2, 15, 16; N = 1, 63, 64, 65, 255, 256, 257, 512,
513, 4,096 and 4,097 with starts on every edge and n_rows around the 4 rows of a
scan workgroup and the 16 of a merge workgroup; the device-side refusal of
descending scan offsets; and one case of each group again behind five other
rows.  tests/test_sig_cases.py shows on the CPU that the inputs are what they
claim and pins the restatement to plain loops.

Bounds: none.  Masks, ring counts, lists, shifts and counts are compared with
``np.array_equal``: only integers and individually rounded fp64 comparisons
decide an outcome.

Measured on an MI355X: the 74 tests of this file take 5.2 s together, the
restatement's lists included; the largest single ones 0.23 s (N = 4,096 and
4,097).  No case failed on the kernels as they were.

Mutation check (scratch builds, never committed; each edit of
csrc/sig_kernels.hip built and run once; the tests of this file that fail, and
of tests/test_sig_gpu.py's kernel tests):
  gate `<=` as `<`                      test_gate_and_screen_on_their_bounds[on-the-bounds, gate-on-its-bound,
                                        full-empty-* (3)], test_shapes[every N but 1],
                                        test_case_inside_a_larger_batch[on-the-bounds]; test_sig_gpu.py: 10
  screen `<=` as `<`                    test_gate_and_screen_on_their_bounds[on-the-bounds, full-empty-* (3)],
                                        test_case_inside_a_larger_batch[on-the-bounds]; test_sig_gpu.py: 6
                                        (its d = 0 lists at threshold 0/1 sit on both bounds)
  lnum, lden as int32_t                 nothing changes: d, n_i + n_j and the cast of lb keep the products 64-bit
  both products in uint32_t             test_gate_and_screen_on_their_bounds[wrap-in-screen, wrap-in-gate,
                                        wrap-out-screen, wrap-out-gate]; test_sig_gpu.py: none
  both products' low words as int32_t   the same four and full-empty-2147483647/2147483647,
                                        full-empty-2147483646/2147483647; test_sig_gpu.py: none
  rot[(t + 64 * p) % S]                 test_rolls_every_sector_count[72, 80, 88, 96, 104, 112, 120],
                                        test_case_inside_a_larger_batch[rolls-72]; test_sig_gpu.py: S = 72
  k = lane + 64 * (kPasses - 1 - p)     test_rolls_every_sector_count[72, ..., 128],
                                        test_case_inside_a_larger_batch[rolls-72]; test_sig_gpu.py: S = 72, 128
"""
import numpy as np
import pytest

import sig_cases as sc
import sig_ref

pytestmark = pytest.mark.gpu

CASES = sc.match_cases()


def _ids(cases):
    return [c.name for c in cases]


def _resident(case):
    from slamhip import sig as gsig
    return gsig.SignatureSet.from_host(case.sig, gsig.SigParams(sectors=case.S))


def _run(case, K, sg):
    from slamhip import sig as gsig
    got = gsig.match_signatures(sg, case.start, case.n_rows, case.frac, K)
    assert all(g.dtype == np.int64 for g in got) and got[0].shape == (case.n_rows, K) == got[1].shape == got[2].shape
    return got


def _equals(case, sg=None):
    """The case at each of its K against the restatement and the hand-written lists; {K: arrays}."""
    sg = sg if sg is not None else _resident(case)
    sel = slice(None) if case.rows is None else case.rows
    out = {}
    for K in case.Ks:
        got = _run(case, K, sg)
        for what, g, w in zip("jdkc", got, case.ref(K)):
            assert np.array_equal(g[sel], w), (case.name, K, what, np.argwhere(g[sel] != w)[:4])
        for r in case.expect:
            want = case.expected(r, K)
            assert all(np.array_equal(g[r], w) for g, w in zip(got, want)), (case.name, K, r, [g[r] for g in got])
        out[K] = got
    return out


def _screen_off_equals(case, on):
    """The same launches with the ring-count screen off: identical arrays."""
    from slamhip import _abi
    L = _abi.lib()
    sg = _resident(case)
    try:
        assert L.slam_sig_set_screen(0) == 0
        off = {K: _run(case, K, sg) for K in case.Ks}
    finally:
        assert L.slam_sig_set_screen(1) == 0
    for K in case.Ks:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(on[K], off[K])), (case.name, K)


def _literal_sets(cases):
    return (np.stack([c.sig for c in cases]), np.stack([c.ring for c in cases]),
            np.array([c.n for c in cases], np.int32))


@pytest.mark.parametrize("S", sc.ALL_S)
def test_build_every_sector_count(S):
    """Group A, alone and between other scans: the literal masks, ring counts (S in one uint8 for
    the one-ring cloud: 128 at S = 128) and n."""
    from slamhip import icp, sig as gsig
    cases = sc.build_cases(S)
    params = gsig.SigParams(sectors=S)
    scans = [c.points for c in cases]
    got = gsig.build_signatures(icp.ScanSet(scans), params).host()
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    with np.errstate(over="ignore", invalid="ignore"):
        ref = sig_ref.signatures(scans, *sig_ref.tables(S))
    for g, w, lit in zip(got, ref, _literal_sets(cases)):
        assert np.array_equal(g, w) and np.array_equal(g, lit), (S, g, lit)
    assert int(got[1][1][sc.one_ring(S)]) == S == int(got[2][1])
    fill = [np.random.default_rng(S + m).uniform(-12, 12, size=(50 + 100 * m, 2)) for m in range(8)]
    inside = gsig.build_signatures(icp.ScanSet(fill[:5] + scans[::-1] + fill[5:]), params).host()
    for g, i in zip(got, inside):
        assert g[::-1].tobytes() == i[5:9].tobytes()


@pytest.mark.parametrize("S", sc.ALL_S)
def test_rolls_every_sector_count(S):
    """Group B through ``SignatureSet.from_host`` and through ``build_signatures`` on the cloud
    that realises the masks: sig_scan_kernel<S> for each of the sixteen S, fed by host-made and by
    device-made ring counts."""
    from slamhip import icp, sig as gsig
    case = sc.roll_case(S)
    given = _equals(case)
    m = len(sc.roll_shifts(S))
    j, d, k, count = given[16]
    assert k[0, :2 * m].tolist() == list(sc.roll_shifts(S)) * 2 and d[0, :2 * m].tolist() == [0] * m + [3] * m
    built = gsig.build_signatures(icp.ScanSet([sc.realise(s) for s in case.sig]), gsig.SigParams(sectors=S))
    ring, n = sig_ref.ring_counts(case.sig)
    for g, w in zip(built.host(), (case.sig, ring, n)):
        assert np.array_equal(g, w)
    again = _equals(case, built)
    for K in case.Ks:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(given[K], again[K]))


@pytest.mark.parametrize("case", CASES["C"], ids=_ids(CASES["C"]))
def test_shift_ties_across_the_passes(case):
    """Shifts 6 and 70 (S = 128), 6, 14, ..., 70 (S = 72) and 6 and 14 (S = 16) tie: 6 wins."""
    got = _equals(case)
    assert got[16][2][0, :2].tolist() == [6, 6] and got[16][1][0, :2].tolist() == [0, 3]


@pytest.mark.parametrize("case", CASES["D"], ids=_ids(CASES["D"]))
def test_gate_and_screen_on_their_bounds(case):
    _screen_off_equals(case, _equals(case))


@pytest.mark.parametrize("case", CASES["E"], ids=_ids(CASES["E"]))
def test_sorted_list_placements(case):
    on = _equals(case)
    named, js = sc.PLACED[case.name[len("placed-"):]]
    assert on[16][0][0, :len(js)].tolist() == js and on[16][3][0] == len(named)
    assert on[1][0][0].tolist() == js[:1] and on[15][0][0, :len(js[:15])].tolist() == js[:15]
    _screen_off_equals(case, on)


@pytest.mark.parametrize("N", sc.SHAPE_N)
def test_shapes(N):
    """Group F: one resident set per N, every n_rows of it a launch of its own."""
    cases = [c for c in CASES["F"] if c.N == N and c.name.startswith("shape-%d-rows" % N)]
    assert [c.n_rows for c in cases] == sorted({r for r in sc.SHAPE_ROWS if r <= N} | {N})
    sg = _resident(cases[0])
    for c in cases:
        _equals(c, sg)


def test_single_signature_starts():
    for start in (0, 1):
        _equals(sc.single_start_case(start))


def test_bad_scan_offsets_leave_the_scan_empty():
    """What only the device sees (kSigBadScan): a scan whose offsets descend is left empty and
    nothing is read through them, slam_sig_status reports it once, and the other scans of the
    launch, a zero-length one among them, are done."""
    import torch
    from slamhip import _abi, device as dv
    S, N, P = 16, 4, 9
    pts = np.random.default_rng(12).uniform(-10, 10, size=(P, 2))
    dirs, edges2 = sig_ref.tables(S)
    d_pts, d_dirs, d_edges = (dv.to_dev(a, np.float64) for a in (pts, dirs, edges2))
    dev = d_pts.device
    L = _abi.lib()
    h = dv.stream_handle()
    assert L.slam_sig_status(h) == 0

    def run(off):
        d_off = dv.to_dev(off, np.int64)
        sig = torch.full((N, S), -1, dtype=torch.int32, device=dev)
        ring = torch.full((N, 32), 255, dtype=torch.uint8, device=dev)
        n = torch.full((N,), -1, dtype=torch.int32, device=dev)
        assert L.slam_sig_build(dv.ptr(d_pts), dv.ptr(d_off), N, P, dv.ptr(d_dirs), dv.ptr(d_edges), S, dv.ptr(sig),
                                dv.ptr(ring), dv.ptr(n), h) == 0
        status = (L.slam_sig_status(h), L.slam_last_error(), L.slam_sig_status(h))
        torch.cuda.synchronize()
        return status, (sig.cpu().numpy().view(np.uint32), ring.cpu().numpy(), n.cpu().numpy())

    def want(spans):
        out = [sig_ref.signature(pts[a:b], dirs, edges2) for a, b in spans]
        return (np.array([o[0] for o in out], np.uint32), np.array([o[1] for o in out], np.uint8),
                np.array([o[2] for o in out], np.int32))
    status, got = run([0, 0, 5, 5, 9])                  # two zero-length scans: empty, and no flag
    assert status[0] == 0 and status[2] == 0
    for g, w in zip(got, want([(0, 0), (0, 5), (5, 5), (5, 9)])):
        assert np.array_equal(g, w)
    assert not got[0][0].any() and not got[1][0].any() and got[2][0] == 0 and got[2][1] > 0 and got[2][3] > 0
    status, got = run([0, 0, 5, 3, 9])                  # scan 2 descends: flagged once, empty
    assert status[0] == -1 and b"scan offsets" in status[1] and status[2] == 0
    for g, w in zip(got, want([(0, 0), (0, 5), (0, 0), (3, 9)])):
        assert np.array_equal(g, w)
    assert not got[0][2].any() and not got[1][2].any() and got[2][2] == 0
    status, got = run([0, 0, 5, 5, 9])                  # the flag does not outlive its report
    assert status[0] == 0 and got[2][2] == 0


INSIDE = [sc.roll_case(72), sc.tie_case(*sc.TIES[0]), sc.boundary_pairs_case(), sc.placed_case("last-chunk"),
          sc.shape_case(257, 17)]


@pytest.mark.parametrize("case", INSIDE, ids=_ids(INSIDE))
def test_case_inside_a_larger_batch(case):
    """One case of each group B to F behind five other rows (other waves of the scan workgroup,
    other tile and chunk offsets of every column): the same bytes, the indices moved up by 5."""
    alone = {K: _run(case, K, _resident(case)) for K in case.Ks}
    moved = _equals(sc.shifted(case, 5))
    for K in case.Ks:
        j, d, k, count = (a[5:] for a in moved[K])
        assert np.where(j >= 0, j - 5, -1).tobytes() == alone[K][0].tobytes()
        assert d.tobytes() == alone[K][1].tobytes() and k.tobytes() == alone[K][2].tobytes()
        assert count.tobytes() == alone[K][3].tobytes()
        assert (moved[K][3][:5] == 0).all() and (moved[K][0][:5] == -1).all()
