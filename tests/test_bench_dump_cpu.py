"""bench.py --dump-outputs without a GPU: dump_scores on a host tensor (what it writes, which rows, how much), and the
arguments bench.py refuses before it touches a device."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _scores(N, K):
    return torch.arange(N * K, dtype=torch.float32).reshape(N, K) / 7.0


def test_a_large_matrix_is_sampled_by_a_fixed_seed(tmp_path):
    N, K = 50_000, 8
    out = _scores(N, K)
    d1 = bench.dump_scores(torch, out, str(tmp_path / "a"))
    d2 = bench.dump_scores(torch, out, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ROWS, K) and np.array_equal(a, b)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(N, bench.DUMP_ROWS, replace=False))
    assert np.array_equal(a, out.numpy()[rows])
    assert d1 == dict(d2, dir=d1["dir"]) and d1["arrays"]["scores"]["shape"] == [bench.DUMP_ROWS, K]
    assert d1["arrays"]["scores"]["of_shape"] == [N, K] and d1["arrays"]["scores"]["rows"] != "all"


def test_a_small_matrix_is_written_whole(tmp_path):
    out = _scores(100, 5)
    d = bench.dump_scores(torch, out, str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "scores.npy"), out.numpy()) and d["arrays"]["scores"]["rows"] == "all"


def test_the_dump_stays_under_its_byte_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    N, K = 30_000, 64
    bench.dump_scores(torch, _scores(N, K), str(tmp_path))
    f = tmp_path / "scores.npy"
    assert os.path.getsize(f) <= 200_000 and np.load(f).shape == ((200_000 - 4096) // (4 * K), K)


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_steps_below_one_are_refused():
    p = _bench("--steps", "0")
    assert p.returncode == 2 and b"--steps must be at least 1" in p.stderr and not p.stdout


def test_dump_outputs_is_refused_where_there_is_no_c2_pass(tmp_path):
    p = _bench("--gpus", "2", "--dump-outputs", str(tmp_path / "d"))
    assert p.returncode == 2 and b"--dump-outputs" in p.stderr and not p.stdout and not (tmp_path / "d").exists()
