"""bench.py's command line: ``--dump-outputs DIR`` writes the last timed
step's results as float64 ``.npy`` files, a plain run prints the lean result
line, and ``--full`` adds the secondary blocks after the timed steps."""
import importlib.util
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus",
             "config"}
FULL_ONLY_KEYS = {"roofline", "cpu_baseline", "parity", "pgo", "c1"}


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_options(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _parse(bench, monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"
    with pytest.raises(SystemExit):
        _parse(bench, monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float64(bench, tmp_path):
    Res = namedtuple("Res", "tf err iters")
    rng = np.random.default_rng(3)
    res = Res(rng.normal(size=(5, 3, 3)), rng.normal(size=5), np.arange(5, dtype=np.int64))
    out = tmp_path / "a" / "b"
    bench.dump_outputs(str(out), res)
    assert sorted(os.listdir(out)) == ["err.npy", "iters.npy", "tf.npy"]
    for name, want in (("tf", res.tf), ("err", res.err), ("iters", res.iters)):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)


def test_dump_outputs_samples_above_the_limit(bench, tmp_path, monkeypatch):
    """Above the size limit every array is cut to the same seeded rows, in order."""
    Res = namedtuple("Res", "tf err iters")
    n = 1000
    res = Res(np.arange(n * 9, dtype=np.float64).reshape(n, 3, 3), np.arange(n, dtype=np.float64),
              np.arange(n, dtype=np.int64))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 72 * 120)   # a share is 120 rows of tf, 1080 of err
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), res)
    tf = np.load(tmp_path / "x" / "tf.npy")
    assert tf.shape == (120, 3, 3) and np.all(np.diff(tf[:, 0, 0]) > 0)
    assert np.array_equal(tf, res.tf[(tf[:, 0, 0] / 9).astype(int)])
    assert np.array_equal(tf, np.load(tmp_path / "y" / "tf.npy"))
    assert np.array_equal(np.load(tmp_path / "x" / "err.npy"), res.err)   # 8 kB: under its share
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert total <= 3 * 72 * 120 + 3 * 128   # the limit and three .npy headers


def _run_bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--pairs", "96", "--beams", "181",
           "--steps", "3", "--warmup", "1", *extra]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_batch_returns(tmp_path):
    from slamhip import icp as k
    from slamhip import se2, synthetic
    out = _run_bench("--dump-outputs", str(tmp_path))
    assert LEAN_KEYS <= set(out) and not (FULL_ONLY_KEYS & set(out))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["config"]["pairs_total"] == 96 and out["ms_per_step"] > 0
    # value is pairs per second of the timed steps
    assert out["value"] == pytest.approx(96 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    # the dumped arrays are the workload's results: the same stream through icp_batch
    seq = synthetic.make_sequence(97, seed=2025, n_beams=181)
    inits = np.stack([se2.pose_to_mat(seq.odometry[i] - seq.odometry[i - 1]) for i in range(1, 97)])
    want = k.icp_batch(seq.scans, np.arange(1, 97), np.arange(96), inits, epsilon=0.05, max_iters=100)
    for name, w in (("tf", want.tf), ("err", want.err), ("iters", want.iters)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, w.astype(np.float64)), name


@pytest.mark.gpu
def test_full_run_adds_the_secondary_blocks():
    out = _run_bench("--full", "--cpu-sample", "8", "--cpu-workers", "2")
    assert LEAN_KEYS <= set(out) and FULL_ONLY_KEYS <= set(out)
    assert out["parity"]["ok"] and out["parity"]["pairs"] == 8
    assert out["roofline"]["kernel_ms"] > 0 and "error" not in out["pgo"] and "error" not in out["c1"]
