"""CPU-side checks of the correlative scan matcher: the C-ABI's argument
validation (no GPU needed) and the NumPy restatement (tests/csm_ref.py) on
hand-made cases."""
import numpy as np
import pytest

import csm_ref


def test_work_size_valid_shape():
    from slamhip import _abi
    lib = _abi.lib()
    n = lib.slam_csm_work_size(6, 128, 9, 5, 7)
    assert n > 6 * 128 * 128          # at least the tables themselves
    assert lib.slam_csm_work_size(1000, 512, 240, 61, 61) > 1000 * 512 * 512
    for bad in ((0, 128, 9, 5, 7), (6, 127, 9, 5, 7), (6, 0, 9, 5, 7), (6, 128, 0, 5, 7), (6, 128, 9, 0, 7),
                (6, 128, 9, 5, 0), (1, 128, 1 << 20, 1 << 6, 1 << 6)):
        assert lib.slam_csm_work_size(*bad) == -1, bad
        assert lib.slam_last_error() != b""


def _call(lib, ptrs, B=2, res=0.05, G=128, n_theta=9, nx=7, ny=5):
    p = [1 if f else None for f in ptrs]   # never dereferenced: validation fails first
    return lib.slam_csm_batch(p[0], p[1], p[2], p[3], p[4], p[5], B, res, G, n_theta, nx, ny, p[6], None, p[7], None)


def test_batch_rejects_null_pointers():
    from slamhip import _abi
    lib = _abi.lib()
    assert _call(lib, [0] * 8) == -1 and b"null" in lib.slam_last_error()
    for missing in range(8):
        ptrs = [1] * 8
        ptrs[missing] = 0
        assert _call(lib, ptrs) == -1 and b"null" in lib.slam_last_error(), missing


@pytest.mark.parametrize("kw, word", [(dict(G=127), b"G"), (dict(G=0), b"G"), (dict(B=0), b"B"),
                                      (dict(res=0.0), b"res"), (dict(res=-1.0), b"res"),
                                      (dict(n_theta=0), b"n_theta"), (dict(nx=0), b"nx"), (dict(ny=-3), b"ny"),
                                      (dict(n_theta=1 << 20, nx=1 << 6, ny=1 << 6), b"volume")])
def test_batch_rejects_bad_shapes(kw, word):
    from slamhip import _abi
    lib = _abi.lib()
    assert _call(lib, [1] * 8, **kw) == -1
    assert word in lib.slam_last_error(), lib.slam_last_error()


def test_gather_switch_validates():
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_csm_set_gather(3) == -1 and b"gather" in lib.slam_last_error()
    assert lib.slam_csm_set_gather(1) == 0 and lib.slam_csm_set_gather(4) == 0


def test_unknown_loop_closure_init_raises():
    """An unknown ``init`` is refused before anything touches the device."""
    import src.loop_closure_detection as lcd
    from slamhip import pipeline
    with pytest.raises(ValueError, match="init"):
        pipeline.manual_loop_closures(None, [np.zeros((3, 2))] * 2, [[0, 1]], init="bogus")
    with pytest.raises(ValueError, match="init"):
        lcd.detect_proximity(None, [], init="bogus")
    with pytest.raises(ValueError, match="init"):
        lcd.detect_images_direct_similarity(None, [], [], init="bogus")


def test_restatement_one_point():
    """One reference point, one query point: one 2, eight 1s, zeros."""
    S, cs = csm_ref.score_volume([[0.02, 0.03]], [[0.02, 0.03]], n_theta=1, nx=7, ny=5, G=64, res=0.1)
    assert S.shape == (1, 5, 7) and S.dtype == np.int32
    want = np.zeros((5, 7), np.int32)
    want[1:4, 2:5] = 1
    want[2, 3] = 2
    assert np.array_equal(S[0], want)
    assert csm_ref.best(S) == (2, (0, 2, 3))
    assert np.array_equal(cs, [[1.0, 0.0]])


def test_restatement_table_clipping():
    """Each of the 9 cells is clipped on its own: a point one cell outside the
    grid still marks its neighbours inside; a far point marks nothing."""
    G, res = 8, 1.0
    L = csm_ref.lookup_table([[-4.5, 0.5], [1e12, -1e12], [3.5, 3.5]], G, res)
    want = np.zeros((G, G), np.uint8)
    want[3:6, 0] = 1          # neighbours of cell (x = -1, y = 4)
    want[6:8, 6:8] = 1        # corner cell (7, 7) and its in-grid neighbours
    want[7, 7] = 2
    assert np.array_equal(L, want)


def test_restatement_shift_and_ties():
    """A query displaced by whole cells peaks at the opposite shift; equal
    scores resolve to the smallest flat index."""
    ref = np.array([[0.05, 0.05], [1.05, 0.05], [0.05, 2.05]])
    tf, score, index, S = csm_ref.match(ref - [0.3, -0.2], ref, n_theta=3, d_theta=0.5, nx=9, ny=9, G=64, res=0.1)
    assert score == 6 and index == (1, 2, 7)
    assert np.allclose(tf, [[1, 0, 0.3], [0, 1, -0.2], [0, 0, 1]])
    _, score, index, S = csm_ref.match([[0.0, 0.0]], [[0.0, 0.0]], n_theta=5, d_theta=0.1, nx=7, ny=5, G=64, res=0.1)
    assert score == 2 and index == (0, 2, 3) and (S[:, 2, 3] == 2).all()
    _, score, index, S = csm_ref.match([[1e3, 0.0]], [[0.0, 0.0]], n_theta=5, d_theta=0.1, nx=7, ny=5, G=64, res=0.1)
    assert score == 0 and index == (0, 0, 0) and not S.any()
