"""CPU-side checks of the descriptor matcher (slamhip.desc,
csrc/desc_kernels.hip): the NumPy restatement (tests/desc_ref.py) against a
plain-Python double loop of the definition, the float32 square-root facts the
``l2`` score rests on, the synthetic descriptor generator, the C-ABI's argument
validation (no GPU needed), the host-side selection rule and the new keywords
and command-line flags."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import PKG

import desc_ref

sys.path.insert(0, os.path.join(PKG, "scripts"))


# ---- the definition, as plainly as it can be written -------------------------

def _d(x, y, metric):
    if metric == "hamming":
        return sum(bin(int(p) ^ int(q)).count("1") for p, q in zip(x, y))
    return sum((int(p) - int(q)) ** 2 for p, q in zip(x, y))


def _plain_matches(A, B, metric):
    if len(A) == 0 or len(B) == 0:
        return []
    fwd = []
    for a in range(len(A)):
        best = None
        for b in range(len(B)):
            d = _d(A[a], B[b], metric)
            if best is None or d < best[0]:   # strict: the smallest b among equals
                best = (d, b)
        fwd.append(best)
    out = []
    for a, (d, b) in enumerate(fwd):
        if metric == "hamming":
            back = None
            for a2 in range(len(A)):
                d2 = _d(A[a2], B[b], metric)
                if back is None or d2 < back[0]:
                    back = (d2, a2)
            if back[1] != a:
                continue
        out.append((a, b, d))
    return sorted(out, key=lambda m: m[2])   # stable, like the reference's sorted(matches, key=distance)


def _tie_cases():
    rng = np.random.default_rng(0)
    code = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    few = code[rng.integers(0, 4, 9)], code[rng.integers(0, 4, 7)]          # a 4-code codebook: ties everywhere
    same = np.repeat(code[:1], 5, axis=0), np.repeat(code[:1], 3, axis=0)  # all identical
    near = code[rng.integers(0, 4, 8)].copy(), code[rng.integers(0, 4, 8)].copy()
    near[0][:, 0] ^= rng.integers(0, 4, 8).astype(np.uint8)                 # small distances with repeats
    rand = rng.integers(0, 256, (11, 32), dtype=np.uint8), rng.integers(0, 256, (6, 32), dtype=np.uint8)
    empty = np.zeros((0, 32), np.uint8), code
    return [few, same, near, rand, empty, (code, np.zeros((0, 32), np.uint8)), (code[:1], code[:1])]


@pytest.mark.parametrize("metric", desc_ref.METRICS)
def test_restatement_against_the_plain_definition(metric):
    for A, B in _tie_cases():
        want = _plain_matches(A, B, metric)
        got = desc_ref.matches(A, B, metric)
        assert got.shape == (len(want), 3) and got.tolist() == [list(m) for m in want]
        for n in (1, 2, len(want), len(want) + 1):
            if n < 1:
                continue
            s, c, rows = desc_ref.score(got, n, metric)
            assert c == len(want)
            if n > len(want):
                assert s == np.inf and (rows == -1).all()
            else:
                total = 0.0
                for _, _, d in want[:n]:
                    total += float(d) if metric == "hamming" else float(np.float32(math.sqrt(d)))   # the fp64 route
                assert s == total and rows.tolist() == [list(m) for m in want[:n]]


def test_l2_extremes_and_symmetry():
    lo, hi = np.zeros((2, 32), np.uint8), np.full((3, 32), 255, np.uint8)
    assert (desc_ref.distance_matrix(lo, hi, "l2") == 2080800).all()
    assert (desc_ref.distance_matrix(lo, hi, "hamming") == 256).all()
    rng = np.random.default_rng(1)
    A, B = rng.integers(0, 256, (5, 32), dtype=np.uint8), rng.integers(0, 256, (4, 32), dtype=np.uint8)
    for metric in desc_ref.METRICS:
        assert np.array_equal(desc_ref.distance_matrix(A, B, metric), desc_ref.distance_matrix(B, A, metric).T)


def test_float32_square_roots_exhaustive():
    """For every possible l2 distance d <= 32 * 255^2: the fp64 root rounded to
    float32 IS the float32 root (a kernel may take either route), and distinct
    d have distinct float32 roots (ordering by d is ordering by the root)."""
    d = np.arange(32 * 255 * 255 + 1, dtype=np.int64)
    r32 = np.sqrt(d.astype(np.float32))
    assert r32.dtype == np.float32
    assert np.array_equal(r32, np.sqrt(d.astype(np.float64)).astype(np.float32))
    assert (np.diff(r32) > 0).all()
    # and a sum of up to 256 such roots is exact in float64 in any order: each is a multiple of 2^-23 below 2^11
    assert np.array_equal(r32.astype(np.float64) * 2.0 ** 23, np.round(r32.astype(np.float64) * 2.0 ** 23))
    assert r32.max() < 2.0 ** 11


# ---- the generator -------------------------------------------------------------

@pytest.fixture(scope="module")
def loop():
    from slamhip import synthetic
    seq = synthetic.make_loop_sequence(66, seed=2, n_beams=5, step=1.32)   # 3.3 laps of 20 positions
    assert seq.per_lap == 20
    return seq, synthetic.make_descriptors(seq, seed=2, n_per_image=100)


def test_generator_is_deterministic(loop):
    from slamhip import synthetic
    seq, descs = loop
    again = synthetic.make_descriptors(seq, seed=2, n_per_image=100)
    assert len(descs) == 66 and all(d.shape == (100, 32) and d.dtype == np.uint8 for d in descs)
    assert all(np.array_equal(a, b) for a, b in zip(descs, again))
    other = synthetic.make_descriptors(seq, seed=3, n_per_image=100)
    assert not np.array_equal(descs[0], other[0])
    half = synthetic.make_descriptors(seq, seed=2, image_rate=2, n_per_image=100)
    assert len(half) == 33 and np.array_equal(half[1], descs[2])
    with pytest.raises(ValueError, match="loop"):
        synthetic.make_descriptors(synthetic.make_sequence(4, seed=0, n_beams=5), seed=0)


@pytest.mark.parametrize("metric", desc_ref.METRICS)
def test_generator_selects_only_same_place_pairs(loop, metric):
    """The threshold is derived here, from the generator as committed: halfway
    between the worst same-place score and the best other score."""
    from slamhip import desc
    seq, descs = loop
    n = 20
    start = desc.image_starts(seq.odometry, 5, 1)
    assert len(start) == 66 and (np.diff(start) >= 0).all() and start[0] > 0
    mat = desc_ref.similarity_matrix(descs, start, n, metric)
    i, j = np.nonzero(np.isfinite(mat))
    assert len(i) > 500
    same = (j - i) % seq.per_lap == 0
    assert same.sum() >= 40
    worst_same, best_other = mat[i[same], j[same]].max(), mat[i[~same], j[~same]].min()
    print(metric, "same place <=", worst_same, "others >=", best_other)
    assert worst_same * 1.5 < best_other
    thresh = 0.5 * (worst_same + best_other)
    good = desc.select_matches(mat, thresh)
    assert len(good) >= 40
    assert all((b - a) % seq.per_lap == 0 and b >= start[a] for a, b in good)


def test_image_starts_restates_the_reference():
    from slamhip import desc, synthetic
    poses = synthetic.make_loop_sequence(200, seed=4, n_beams=3, step=0.3).odometry
    dx, dy = poses[:-1, 0] - poses[1:, 0], poses[:-1, 1] - poses[1:, 1]
    walked = np.append([0], np.cumsum(np.sqrt(dx * dx + dy * dy)))
    for mdp, rate in ((5, 1), (5, 3), (2, 7), (1000, 2)):
        # reference src/loop_closure_detection.py:87-91
        want = np.array([np.searchsorted(walked, walked[i] + mdp, side="right") for i in range(len(walked))])
        want[want == len(want)] = want[want == len(want)] * rate
        want = np.floor(want[::rate] / rate).astype(int)
        got = desc.image_starts(poses, mdp, rate)
        assert got.tolist() == want.tolist() and len(got) == -(-200 // rate)
    with pytest.raises(ValueError, match="image_rate"):
        desc.image_starts(poses, 5, 0)


# ---- selection -----------------------------------------------------------------

def test_select_matches_hand_made():
    from slamhip import desc
    inf = np.inf
    m = np.array([[inf, 5.0, 9.0, inf],
                  [inf, inf, 3.0, inf],
                  [inf, inf, inf, inf],
                  [inf, inf, inf, inf]])
    assert desc.select_matches(m, 10) == [(0, 1), (1, 2)]      # columns 0 and 3 are all-inf: argmin 0, inf < t fails
    assert desc.select_matches(m, 5) == [(1, 2)]               # strict <
    assert desc.select_matches(m, 3) == []
    assert desc.select_matches(m, inf) == [(0, 1), (1, 2)]     # inf < inf fails too
    tie = np.array([[4.0, 4.0], [4.0, 1.0]])
    assert desc.select_matches(tie, 5) == [(0, 0), (1, 1)]     # the first row among equals
    assert desc.select_matches(np.zeros((0, 0)), 5) == []
    with pytest.raises(ValueError, match="matrix"):
        desc.select_matches(np.zeros(3), 5)


# ---- C-ABI validation, no device ------------------------------------------------

def _call(lib, ptrs=(1,) * 7, M=4, B=3, metric=0, n_matches=10):
    p = [16 if f else None for f in ptrs]   # never dereferenced: validation fails first
    return lib.slam_desc_match_batch(p[0], p[1], M, p[2], p[3], B, metric, n_matches, p[4], p[5], None, p[6], None)


def test_abi_validation():
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_abi_version() >= 104
    for missing in range(7):
        ptrs = [1] * 7
        ptrs[missing] = 0
        assert _call(lib, ptrs) == -1 and b"null" in lib.slam_last_error(), missing
    for kw, word in ((dict(B=-1), b"B"), (dict(M=0), b"M"), (dict(M=-2), b"M"), (dict(metric=2), b"metric"),
                     (dict(metric=-1), b"metric"), (dict(n_matches=0), b"n_matches"),
                     (dict(n_matches=257), b"n_matches")):
        assert _call(lib, **kw) == -1
        assert word in lib.slam_last_error(), lib.slam_last_error()
    assert lib.slam_desc_match_batch(8, 16, 4, 16, 16, 3, 0, 10, 16, 16, None, 16, None) == -1
    assert b"aligned" in lib.slam_last_error()
    # no pairs: success without a launch (nothing is dereferenced, no device needed)
    assert _call(lib, B=0) == 0 and lib.slam_last_error() == b""
    for metric in (0, 1):
        for n in (1, 256):
            assert _call(lib, B=0, metric=metric, n_matches=n) == 0


def test_work_size():
    from slamhip import _abi
    lib = _abi.lib()
    assert lib.slam_desc_work_size(-1, 10, 10) == -1
    assert lib.slam_desc_work_size(5, -1, 10) == -1
    assert lib.slam_desc_work_size(5, 10, 0) == -1 and lib.slam_desc_work_size(5, 10, 257) == -1
    assert lib.slam_desc_work_size(5, 4097, 10) == -3 and b"4096" in lib.slam_last_error()
    last = 0
    for B, n, k in ((0, 0, 1), (1, 1, 1), (300, 500, 10), (300, 4096, 256), (500000, 4096, 256),
                    ((1 << 31) - 1, 4096, 256)):
        w = lib.slam_desc_work_size(B, n, k)
        assert 0 < w < 1 << 40 and w >= last, (B, n, k, w)
        last = w
    assert lib.slam_last_error() == b""


# ---- Python surface -------------------------------------------------------------

def test_python_argument_checks_stay_on_the_host():
    from slamhip import desc
    assert desc.METRICS == {"hamming": 0, "l2": 1}
    with pytest.raises(ValueError, match="metric"):
        desc.match_pairs(None, [0], [0], 10, metric="cosine")
    with pytest.raises(ValueError, match="n_matches"):
        desc.match_pairs(None, [0], [0], 0)
    with pytest.raises(ValueError, match="n_matches"):
        desc.match_pairs(None, [0], [0], 257)
    with pytest.raises(ValueError, match="train"):
        desc.match_pairs(None, [0, 1], [0], 10)
    s, c, m = desc.match_pairs(None, [], [], 7, return_matches=True)   # no pairs: nothing touches the device
    assert s.shape == c.shape == (0,) and m.shape == (0, 7, 3)
    for bad in (np.zeros((3, 31), np.uint8), np.zeros((3, 32), np.int8), np.zeros((3, 32)), np.zeros(32, np.uint8),
                np.zeros((2, 3, 32), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            desc.DescriptorSet([np.zeros((1, 32), np.uint8), bad])
    with pytest.raises(ValueError, match="no images"):
        desc.DescriptorSet([])


def test_matcher_keyword():
    import src.loop_closure_detection as host
    with pytest.raises(ValueError, match="matcher"):
        host.detect_images_direct_similarity(None, [], [], matcher="bogus")
    assert "cv2" not in sys.modules
    with pytest.raises(ValueError, match="save_matches"):
        host.detect_images_direct_similarity(None, [], None, save_matches=True, matcher="device",
                                             descriptors=[np.zeros((1, 32), np.uint8)])
    assert "cv2" not in sys.modules
    with pytest.raises(ValueError, match="init"):
        host.detect_images_direct_similarity(None, [], None, matcher="device", descriptors=[], init="bogus")


def test_cli_flags():
    import main_batched as mb
    a = mb.parse(["synthetic:loop:100"])
    assert a.loop_closure_detection == "none" and a.descriptors is None and a.descriptor_metric == "hamming"
    assert mb.image_params(a) == dict(image_match_error=2500, keypoint_n_matches=20, image_downsample=1,
                                      min_dist_along_path=5)
    a = mb.parse(["synthetic:loop:100", "--loop-closure-detection", "descriptors", "--descriptors", "auto",
                  "--descriptor-metric", "l2", "--image-match-error", "5500", "--keypoint-n-matches", "12",
                  "--image-downsample", "2", "--min-dist-along-path", "3", "--loop-closure-icp-error", "25"])
    assert (a.loop_closure_detection, a.descriptors, a.descriptor_metric) == ("descriptors", "auto", "l2")
    assert mb.image_params(a) == dict(image_match_error=5500, keypoint_n_matches=12, image_downsample=2,
                                      min_dist_along_path=3)
    assert a.loop_closure_icp_error == 25
    for bad in (["--loop-closure-detection", "descriptors"],                 # no --descriptors
                ["--loop-closure-detection", "images"],
                ["--descriptor-metric", "cosine"]):
        with pytest.raises(SystemExit):
            mb.parse(["synthetic:loop:100"] + bad)


def test_cli_descriptor_sources(tmp_path):
    import main_batched as mb
    from slamhip import synthetic
    a = mb.parse(["synthetic:loop:40:7", "--loop-closure-detection", "descriptors", "--descriptors", "auto",
                  "--dataset-start", "4"])
    got = mb.load_descriptors(a, 30, 3)
    seq = synthetic.make_loop_sequence(40, seed=7, n_beams=3)
    want = synthetic.make_descriptors(seq, 7)[4:34:3]
    assert len(got) == 10 and all(np.array_equal(x, y) for x, y in zip(got, want))
    desc = np.concatenate(want[:3])
    off = np.array([0, 500, 500, 1500])
    np.savez(tmp_path / "d.npz", desc=desc, off=off)
    a = mb.parse(["x.npz", "--loop-closure-detection", "descriptors", "--descriptors", str(tmp_path / "d.npz")])
    got = mb.load_descriptors(a, 3, 1)
    assert [len(g) for g in got] == [500, 0, 1000] and np.array_equal(got[2], desc[500:])
    a = mb.parse(["synthetic:walk:40", "--loop-closure-detection", "descriptors", "--descriptors", "auto"])
    with pytest.raises(SystemExit):
        mb.load_descriptors(a, 40, 1)
