"""GPU tests of the descriptor matcher (csrc/desc_kernels.hip, slamhip.desc) and
of the stage, the drop-in keyword and the command-line switch that use it.

The yardstick is the NumPy restatement tests/desc_ref.py (which
tests/test_desc.py pins to a plain loop over the definition).  Only integers
decide anything, so every comparison is ``np.array_equal``: score, count and
the (a, b, d) rows, for both metrics."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG

import desc_ref

sys.path.insert(0, os.path.join(PKG, "scripts"))

pytestmark = pytest.mark.gpu

METRICS = desc_ref.METRICS
# wave (64), workgroup (256), two queries per lane (512) and LDS tile (256) boundaries, several passes (1100)
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 500, 513, 1100)


def _equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g, w, equal_nan=False)


@pytest.fixture(scope="module")
def images():
    from slamhip import desc
    rng = np.random.default_rng(11)
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in COUNTS]
    return descs, desc.DescriptorSet(descs)


@pytest.fixture(scope="module")
def all_pairs(images):
    """Every ordered pair of the boundary images and the restatement's answers
    at n_matches = 10, computed once."""
    descs, _ = images
    qi, ti = [a.ravel() for a in np.meshgrid(np.arange(len(COUNTS)), np.arange(len(COUNTS)), indexing="ij")]
    return qi, ti, {m: desc_ref.match_pairs(descs, qi, ti, 10, m) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_boundary_counts_all_ordered_pairs(images, all_pairs, metric):
    from slamhip import desc
    _, ds = images
    qi, ti, want = all_pairs
    got = desc.match_pairs(ds, qi, ti, 10, metric, return_matches=True)
    _equal(got, want[metric])
    assert np.isinf(got[0]).sum() >= 2 * len(COUNTS) - 1 and np.isfinite(got[0]).sum() > 50
    # without the rows: the same score and count (hamming takes its histogram path)
    _equal(desc.match_pairs(ds, qi, ti, 10, metric), want[metric][:2])


@pytest.mark.parametrize("metric", METRICS)
def test_batch_position_second_call_and_stream(images, all_pairs, metric):
    import torch
    from slamhip import desc
    _, ds = images
    qi, ti, want = all_pairs
    k = int(np.nonzero((qi == 9) & (ti == 10))[0][0])           # 500 x 513
    alone = desc.match_pairs(ds, [9], [10], 10, metric, return_matches=True)
    _equal(alone, [w[k:k + 1] for w in want[metric]])
    rng = np.random.default_rng(5)
    for pos in (0, 150, 299):
        q, t = rng.integers(0, len(COUNTS), 300), rng.integers(0, len(COUNTS), 300)
        q[pos], t[pos] = 9, 10
        batch = desc.match_pairs(ds, q, t, 10, metric, return_matches=True)
        _equal([b[pos:pos + 1] for b in batch], alone)
        idx = q * len(COUNTS) + t                                  # the whole batch, too
        _equal(batch, [w[idx] for w in want[metric]])
    _equal(desc.match_pairs(ds, qi, ti, 10, metric, return_matches=True), want[metric])   # a second call
    _equal(desc.match_pairs(ds, qi, ti, 10, metric, return_matches=True, stream=torch.cuda.Stream()), want[metric])


@pytest.mark.parametrize("metric", METRICS)
def test_n_matches_up_to_count_and_beyond(images, metric):
    from slamhip import desc
    descs, ds = images
    q, t = 6, 9                                                    # 255 x 500: count <= 255
    rows = desc_ref.matches(descs[q], descs[t], metric)
    count = len(rows)
    assert 20 < count <= 255 and (metric == "hamming" or count == 255)
    for n in (1, 10, 20, count, count + 1):
        want = desc_ref.score(rows, n, metric)
        s, c, m = desc.match_pairs(ds, [q], [t], n, metric, return_matches=True)
        assert s[0] == want[0] and c[0] == want[1] == count and np.array_equal(m[0], want[2])
        s2, c2 = desc.match_pairs(ds, [q], [t], n, metric)
        assert s2[0] == s[0] and c2[0] == count
        if n > count:
            assert s[0] == np.inf and (m == -1).all()
    # 256 matches, the most the entry point takes
    rows = desc_ref.matches(descs[9], descs[11], "l2")
    s, c, m = desc.match_pairs(ds, [9], [11], 256, "l2", return_matches=True)
    want = desc_ref.score(rows, 256, "l2")
    assert s[0] == want[0] and c[0] == 500 and np.array_equal(m[0], want[2])


@pytest.mark.parametrize("metric", METRICS)
def test_ties_take_the_first_index(metric):
    """A 4-code codebook and all-identical descriptors: ties in both directions
    and in the (d, a) order inside the cut bin."""
    from slamhip import desc
    rng = np.random.default_rng(3)
    code = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    near = code[rng.integers(0, 4, 600)].copy()
    near[:, 5] ^= rng.integers(0, 8, 600).astype(np.uint8)        # many equal small distances
    descs = [code[rng.integers(0, 4, 300)], code[rng.integers(0, 4, 700)], np.repeat(code[:1], 130, axis=0),
             np.repeat(code[:1], 70, axis=0), near, code[rng.integers(0, 4, 520)], code[[2, 2, 1]]]
    ds = desc.DescriptorSet(descs)
    qi, ti = [a.ravel() for a in np.meshgrid(np.arange(len(descs)), np.arange(len(descs)), indexing="ij")]
    for n in (1, 3, 20):
        want = desc_ref.match_pairs(descs, qi, ti, n, metric)
        _equal(desc.match_pairs(ds, qi, ti, n, metric, return_matches=True), want)
        _equal(desc.match_pairs(ds, qi, ti, n, metric), want[:2])
    assert np.isfinite(want[0]).any()


def test_l2_largest_distance_does_not_overflow():
    from slamhip import desc
    descs = [np.zeros((5, 32), np.uint8), np.full((3, 32), 255, np.uint8)]
    ds = desc.DescriptorSet(descs)
    for q, t in ((0, 1), (1, 0)):
        n = len(descs[q])
        s, c, m = desc.match_pairs(ds, [q], [t], n, "l2", return_matches=True)
        assert c[0] == n and (m[0, :, 2] == 2080800).all() and m[0, :, 0].tolist() == list(range(n))
        assert (m[0, :, 1] == 0).all()
        assert s[0] == desc_ref.score(desc_ref.matches(descs[q], descs[t], "l2"), n, "l2")[0]
        assert s[0] == n * float(np.sqrt(np.float32(2080800)))
    s, c, m = desc.match_pairs(ds, [0], [1], 5, "hamming", return_matches=True)
    assert c[0] == 1 and s[0] == np.inf                          # one cross-checked match: (0, 0)


@pytest.mark.parametrize("metric", METRICS)
def test_largest_image(metric):
    """4,096 descriptors an image is the capacity; 4,097 is SLAM_ETOOBIG."""
    from slamhip import _abi, desc
    rng = np.random.default_rng(8)
    code = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    big = code[rng.integers(0, 64, 4096)].copy()
    big[:, 9] ^= rng.integers(0, 4, 4096).astype(np.uint8)
    other = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    descs = [big, other, other[:300]]
    ds = desc.DescriptorSet(descs)
    qi, ti = [0, 1, 2, 0, 0], [1, 0, 0, 2, 0]
    _equal(desc.match_pairs(ds, qi, ti, 20, metric, return_matches=True),
           desc_ref.match_pairs(descs, qi, ti, 20, metric))
    too_big = desc.DescriptorSet([other, np.concatenate([other, other[:1]])])
    with pytest.raises(_abi.SlamHipError, match="status -3"):
        desc.match_pairs(too_big, [0], [1], 20, metric)


def test_device_side_checks():
    """What only the device can see: the kernel leaves such a pair undone and
    slam_desc_status reports it once; the other pairs of the launch are done."""
    import torch
    from slamhip import _abi, desc, device as dv
    rng = np.random.default_rng(9)
    descs = [rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.integers(0, 256, (4097, 32), dtype=np.uint8),
             rng.integers(0, 256, (30, 32), dtype=np.uint8)]
    ds = desc.DescriptorSet(descs)
    L = _abi.lib()
    work = dv.empty((256,), np.uint8)

    def run(qi, ti):
        B = len(qi)
        d_q, d_t = dv.to_dev(qi, np.int32), dv.to_dev(ti, np.int32)
        s, c, m = dv.empty((B,), np.float64), dv.empty((B,), np.int32), dv.empty((B, 5, 3), np.int32)
        rc = L.slam_desc_match_batch(dv.ptr(ds.d_desc), dv.ptr(ds.d_off), 3, dv.ptr(d_q), dv.ptr(d_t), B, 0, 5,
                                     dv.ptr(s), dv.ptr(c), dv.ptr(m), dv.ptr(work), dv.stream_handle())
        assert rc == 0
        status = L.slam_desc_status(dv.stream_handle())
        torch.cuda.synchronize()
        return status, s.cpu().numpy(), c.cpu().numpy(), m.cpu().numpy()

    want = desc_ref.match_pairs(descs, [0], [2], 5, "hamming")
    for qi, ti, code in (([0, 0, 1], [2, 1, 0], -3), ([0, 3, 0, 0], [2, 0, -1, 3], -1), ([0], [2], 0)):
        status, s, c, m = run(qi, ti)
        assert status == code and (code == 0 or L.slam_last_error() != b"")
        assert s[0] == want[0][0] and c[0] == want[1][0] and np.array_equal(m[0], want[2][0])
        assert np.isnan(s[1:]).all() and (c[1:] == -1).all() and (m[1:] == -1).all()
        assert L.slam_desc_status(dv.stream_handle()) == 0        # reported once, then cleared
    small = desc.DescriptorSet([descs[0], descs[2]])              # the Python surface, on a set within capacity
    with pytest.raises(_abi.SlamHipError, match="status -1"):
        desc.match_pairs(small, [0, 5], [1, 0], 5)
    with pytest.raises(_abi.SlamHipError, match="status -1"):
        desc.match_pairs(small, [0], [1 << 40], 5)
    _equal(desc.match_pairs(small, [0], [1], 5, return_matches=True), want)


@pytest.mark.parametrize("metric", METRICS)
def test_similarity_matrix(metric):
    from slamhip import desc
    rng = np.random.default_rng(21)
    counts = rng.integers(0, 40, 48)
    counts[[3, 17]] = 0
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in counts]
    descs[5] = None
    start = np.minimum(np.arange(48) + rng.integers(0, 9, 48), 48)
    start[-3:] = 48
    ds = desc.DescriptorSet(descs)
    got = desc.similarity_matrix(ds, start, 5, metric)
    want = desc_ref.similarity_matrix(descs, start, 5, metric)
    assert got.shape == (48, 48) and np.array_equal(got, want)
    assert np.isfinite(got).sum() > 300 and np.isinf(got[:, 0]).sum() >= 47
    assert np.isinf(desc.similarity_matrix(ds, np.full(48, 48), 5, metric)).all()   # no pair at all: no launch
    with pytest.raises(ValueError, match="starts"):
        desc.similarity_matrix(ds, start[:-1], 5, metric)


# ---- end to end -----------------------------------------------------------------

class _Graph:
    def __init__(self, poses):
        self.poses = poses
        self.added = []

    def add_constraint(self, i, j, tf):
        self.added.append((i, j, np.array(tf)))


N_MATCHES, ICP_ERR = 20, 30


@pytest.fixture(scope="module")
def loop():
    """3 laps of 53 scans with descriptors, and per metric the host replay: the
    restatement's matrix, a threshold halfway between its worst same-place and
    best other score, select_matches, and the existing batched ICP."""
    from slamhip import desc, icp, synthetic
    seq = synthetic.make_loop_sequence(160, 3, n_beams=181, step=0.5)
    assert seq.per_lap == 53
    descs = synthetic.make_descriptors(seq, seed=3, n_per_image=64)
    start = desc.image_starts(seq.odometry, 5, 1)
    replay = {}
    for metric in METRICS:
        mat = desc_ref.similarity_matrix(descs, start, N_MATCHES, metric)
        i, j = np.nonzero(np.isfinite(mat))
        same = (j - i) % seq.per_lap == 0
        thresh = 0.5 * (mat[i[same], j[same]].max() + mat[i[~same], j[~same]].min())
        good = desc.select_matches(mat, thresh)
        assert len(good) > 50 and all((b - a) % seq.per_lap == 0 for a, b in good)
        pairs = np.asarray(good)
        r = icp.icp_batch(seq.scans, pairs[:, 0], pairs[:, 1], np.broadcast_to(np.eye(3), (len(good), 3, 3)),
                          epsilon=0.05, max_iters=100)
        added = [(int(a), int(b), r.tf[k]) for k, (a, b) in enumerate(good) if r.err[k] < ICP_ERR]
        assert len(added) >= 1
        replay[metric] = (mat, thresh, good, added)
    return seq, descs, replay


def _same_constraints(got, want):
    assert [(i, j) for i, j, _ in got] == [(i, j) for i, j, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("metric", METRICS)
def test_stage_adds_the_host_replays_constraints(loop, metric):
    from slamhip import desc, icp, pipeline
    seq, descs, replay = loop
    mat, thresh, good, added = replay[metric]
    g = _Graph(seq.odometry.copy())
    ds = desc.DescriptorSet(descs)
    got_good, accepted = pipeline.image_loop_closures(g, seq.scans, ds, 1, 5, thresh, N_MATCHES, ICP_ERR, metric,
                                                      scanset=icp.ScanSet(seq.scans))
    assert got_good == good and accepted.dtype == bool and accepted.shape == (len(good),)
    assert [p for p, ok in zip(good, accepted) if ok] == [(i, j) for i, j, _ in added]
    _same_constraints(g.added, added)
    assert np.array_equal(desc.similarity_matrix(ds, desc.image_starts(seq.odometry, 5, 1), N_MATCHES, metric), mat)
    with pytest.raises(ValueError, match="images"):
        pipeline.image_loop_closures(g, seq.scans, descs[:-1], 1, 5, thresh, N_MATCHES, ICP_ERR, metric)


@pytest.mark.parametrize("approximate", [False, True])
def test_drop_in_device_matcher(loop, approximate, capsys):
    import src.loop_closure_detection as host
    seq, descs, replay = loop
    _, thresh, _, added = replay["l2" if approximate else "hamming"]
    g = _Graph(seq.odometry.copy())
    host.detect_images_direct_similarity(g, seq.scans, None, 1, 5, thresh, N_MATCHES, ICP_ERR, False, False, -1,
                                         approximate, matcher="device", descriptors=descs)
    _same_constraints(g.added, added)
    assert "Closest images keypoint match error" in capsys.readouterr().out
    assert "cv2" not in sys.modules


def test_image_rate(loop):
    """Every second scan carries an image: the stage's pairs are image indices,
    its constraints scan indices."""
    from slamhip import desc, pipeline
    seq, descs, replay = loop
    half = descs[::2]
    start = desc.image_starts(seq.odometry, 5, 2)
    mat = desc_ref.similarity_matrix(half, start, N_MATCHES, "hamming")
    good = desc.select_matches(mat, replay["hamming"][1])
    g = _Graph(seq.odometry.copy())
    got_good, accepted = pipeline.image_loop_closures(g, seq.scans, half, 2, 5, replay["hamming"][1], N_MATCHES,
                                                      ICP_ERR, "hamming")
    assert got_good == good and len(good) > 10
    assert [(i, j) for i, j, _ in g.added] == [(2 * i, 2 * j) for (i, j), ok in zip(good, accepted) if ok]


def test_cli_descriptors(loop, tmp_path):
    import main_batched as mb
    from slamhip import dataset
    seq, descs, replay = loop
    _, thresh, good, added = replay["hamming"]
    dataset.save(tmp_path / "seq.npz", seq.odometry, seq.scans)
    off = np.zeros(len(descs) + 1, np.int64)
    off[1:] = np.cumsum([len(d) for d in descs])
    np.savez(tmp_path / "desc.npz", desc=np.concatenate(descs), off=off)
    rep = mb.run(mb.parse([str(tmp_path / "seq.npz"), "--skip-icp", "--program-end", "loop_closure",
                           "--loop-closure-detection", "descriptors", "--descriptors", str(tmp_path / "desc.npz"),
                           "--image-match-error", repr(float(thresh)), "--keypoint-n-matches", str(N_MATCHES),
                           "--loop-closure-icp-error", str(ICP_ERR), "--results-dir", str(tmp_path),
                           "--skip-occupancy-grid"]))
    det = rep["loop_closure_detection"]
    assert det["method"] == "descriptors" and det["metric"] == "hamming"
    assert det["selected"] == len(good) and det["accepted"] == len(added) >= 1
    edges = [line.split()[1:3] for line in open(tmp_path / "loop_closure_pose_graph.g2o")
             if line.startswith("EDGE_SE2")]
    loops = sorted(tuple(sorted((int(a), int(b)))) for a, b in edges if abs(int(a) - int(b)) > 1)
    assert loops == sorted((i, j) for i, j, _ in added)


def test_bwd_variants_agree(images, all_pairs):
    """The A/B alternative for hamming's backward nearest neighbour (LDS
    atomicMin per distance) gives the bits of the default swapped pass."""
    from slamhip import _abi, desc
    _, ds = images
    qi, ti, want = all_pairs
    L = _abi.lib()
    assert L.slam_desc_set_bwd(2) == -1 and L.slam_desc_set_bwd(-1) == -1
    assert L.slam_desc_set_bwd(1) == 0
    try:
        _equal(desc.match_pairs(ds, qi, ti, 10, "hamming", return_matches=True), want["hamming"])
        _equal(desc.match_pairs(ds, qi, ti, 10, "l2"), want["l2"][:2])
    finally:
        assert L.slam_desc_set_bwd(0) == 0
    _equal(desc.match_pairs(ds, qi, ti, 10, "hamming"), want["hamming"][:2])
