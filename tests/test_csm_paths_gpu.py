"""GPU parity of the correlative scan matcher (csrc/csm_kernels.hip) on every
score-kernel instance and every edge of its clamp, border, gathers and packed
sums, against the NumPy restatement (tests/csm_ref.py) and hand-written numbers.

tests/test_csm_gpu.py runs seeded scans through four of the 24
``csm_score_kernel<R, W>``; here the cases of tests/csm_cases.py put inputs on
the positions the kernels distinguish, each under both gather widths
(``slam_csm_set_gather``): a query in the last cell from which a shift reaches
the grid and in the first from which none does, on all four sides and corners,
odd and even windows, and 1e6 cells out; occupied cells exactly where the last
dword of a window row reads past the window; two reference points in adjacent
cells, 600 duplicates, points in the cells -1 and G and at 1e12; coordinates on
a cell edge, one ulp to either side and on -0.0; points whose cell an FMA
contraction of the rotation would change; up to 40,000 copies of a query point
(scores to 80,000, past the 16-bit pairs of the dword sums) beside a cell of 0;
ties between columns, rows, angles, waves and passes; empty scans between
ordinary pairs; a window for every R of both widths with no idle slot and with
one slot in the last group, windows of two and three passes, the default
61 x 61 window; 240 angles.  tests/test_csm_cases.py shows on the CPU that the
inputs are what they claim and pins the restatement to plain loops.

Bounds: none.  Volumes, best scores, best bins and the assembled transforms are
compared with ``np.array_equal``: everything is an integer once a point is
binned, and the transform is assembled from the bin on the host.

Measured on an MI355X: the 154 tests of this file take 4.8 s together, the
restatement's volumes included; the largest single one 0.22 s (the 64 x 260
window).

Mutation check (scratch builds, never committed; each edit of
csrc/csm_kernels.hip built and run once, the tests of this file that fail):
  xlo + 1, yhi - 1 (clamp one cell       test_hand_placed_case[reach-x7, reach-x8, reach-y5, reach-y6,
  short; reads stay in the table)        corner-7x5, corner-8x6], test_every_instantiation[1x1, 5x1]
  overhang cells kept in the best key    test_hand_placed_case[overhang-1, 2, 3, 5, 6, 7, reach-x7,
  (`i0 + t < nx` on the store only)      corner-7x5], test_every_instantiation[11 of the 1 x ny windows],
                                         dword gathers only
  widening after the tile loop           test_hand_placed_case[saturation], dword gathers only
"""
import numpy as np
import pytest

import csm_cases as cc

pytestmark = pytest.mark.gpu


def _batch(case, width, return_scores, scans=None, pairs=slice(None)):
    from slamhip import _abi
    from slamhip.csm import CsmParams, csm_batch
    lib = _abi.lib()
    assert lib.slam_csm_set_gather(width) == 0
    try:
        return csm_batch(case.scans if scans is None else scans, case.src[pairs], case.dst[pairs], case.centre[pairs],
                         CsmParams(**case.params), return_scores=return_scores)
    finally:
        assert lib.slam_csm_set_gather(4) == 0


def _equals(case, width, scans=None):
    """The case's batch in one launch against the restatement and the hand-written numbers,
    then once more without the volume."""
    vol, index, score, tf = case.ref
    r = _batch(case, width, True, scans)
    assert r.scores.dtype == np.int32 and r.scores.shape == case.shape
    for b in range(len(vol)):      # pair by pair: a pair that must score 0 leaves its neighbours as they are
        assert np.array_equal(r.scores[b], vol[b]), (case.name, width, case.labels[b],
                                                     np.argwhere(r.scores[b] != vol[b])[:4])
        if case.expect is not None:
            assert np.array_equal(r.scores[b], case.expect[b]), (case.name, width, case.labels[b])
    assert np.array_equal(r.index, index) and np.array_equal(r.score, score), (case.name, width, r.index, r.score)
    if case.expect_index is not None:
        assert np.array_equal(r.index, case.expect_index), (case.name, width, r.index)
    if case.expect_score is not None:
        assert np.array_equal(r.score, case.expect_score), (case.name, width, r.score)
    assert np.array_equal(r.tf, tf)
    assert np.array_equal(r.n_query, [len(case.scans[s]) for s in case.src])
    q = _batch(case, width, False, scans)
    assert q.scores is None and np.array_equal(q.index, index) and np.array_equal(q.score, score)
    assert np.array_equal(q.tf, tf)
    return r


HAND = [c for c in cc.hand_cases() if c.name != "empty"]


@pytest.mark.parametrize("width", cc.WIDTHS)
@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_placed_case(case, width):
    _equals(case, width)


@pytest.mark.parametrize("width", cc.WIDTHS)
@pytest.mark.parametrize("nx,ny", cc.sweep_windows(), ids=["%dx%d" % w for w in cc.sweep_windows()])
def test_every_instantiation(nx, ny, width):
    """The window selects ``csm_score_kernel<R, width>`` for the R that csm_cases.host_shape
    names; csm_cases asserts that the windows cover every R of both widths at both fill levels."""
    c = cc.sweep_case(nx, ny)
    r = _equals(c, width)
    for group in (0, -1):
        j0, j1 = cc.slot_rows(nx, ny, width, group)
        assert r.scores[:, :, j0:j1 + 1].any()


@pytest.mark.parametrize("width", cc.WIDTHS)
def test_empty_scans_between_ordinary_pairs(width):
    from slamhip import plicp
    c = cc.empty_case()
    ss = plicp.packed_scans(*c.packed())
    assert len(ss) == 5 and ss.lens.tolist() == [25, 0, 30, 0, 25]
    r = _equals(c, width, ss)
    for b, (kind, s, d) in enumerate(cc.EMPTY_PAIRS):
        if "empty" in kind:
            assert not r.scores[b].any() and r.score[b] == 0 and tuple(r.index[b]) == (0, 0, 0)
            assert r.n_query[b] == len(c.scans[s]) and (r.n_query[b] == 0) == (kind != "empty reference")
        else:
            one = _batch(c, width, True, ss, slice(b, b + 1))
            assert one.scores.tobytes() == r.scores[b].tobytes() and one.tf.tobytes() == r.tf[b].tobytes()
            assert one.index.tobytes() == r.index[b].tobytes() and one.score[0] == r.score[b] > 0
