"""bench.py as the driver runs it: the N = 1 line carries every object without an "error" key, `--gpus N` launches its
own N ranks (rehearsed on the one-GPU box over gloo) and proves it in the line, and refuses when it cannot."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_single_gpu_line_has_every_object_and_no_error(gpu_ctx):
    rc, out, err = _run(["--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--c5-rows", "1000000"])
    assert rc == 0, err[-2000:]
    r = _line(out)
    assert r["metric"] == "score_value evals/sec" and r["n_gpus"] == 1
    for name in ("sweep", "c3", "c4", "c5_shard"):
        assert name in r and "error" not in r[name], (name, r.get(name))
    # `value` is the region that was asked for -- exactly --steps after exactly --warmup; a region long enough for an
    # outside sampler is measured beside it, and the clock-conditioning passes before both are named
    assert r["steps"] == 20 and r["warmup"] == 5
    assert r["config"]["preconditioning_passes"] >= 100
    lr = r["config"]["long_region"]
    assert lr["steps"] >= 200 and 0.5 < lr["ms_per_step"] / r["ms_per_step"] < 1.5
    assert r["roofline"]["timed_region_launches"][1] - r["roofline"]["timed_region_launches"][0] == 20
    roof = r["roofline"]
    assert roof["bound"] == "hbm" and 0.4 < roof["frac"] < 1.0 and 0.4 < roof["frac_caller_alloc"] < 1.0
    sm = r["config"]["score_matrix"]
    assert sm["allocator"].startswith("msc_device_alloc") and sm["candidates_fill_GBps"]
    # a box without a fast stretch is recognised after a few candidates (abi.cpp alloc_placed): never the whole cap
    assert len(sm["candidates_fill_GBps"]) <= 12


def test_steps_are_the_timed_steps_and_the_last_ones_scores_are_dumped(gpu_ctx, tmp_path):
    import numpy as np
    rc, out, err = _run(["--steps", "7", "--warmup", "2", "--no-cpu-baseline", "--no-extra", "--no-sweep",
                         "--dump-outputs", str(tmp_path)])
    assert rc == 0, err[-2000:]
    r = _line(out)
    assert r["steps"] == 7 and r["warmup"] == 2 and r["ms_per_step"] > 0
    a, b = r["roofline"]["timed_region_launches"]
    assert b - a == 7
    s = np.load(tmp_path / "scores.npy")
    assert s.dtype == np.float32 and s.shape == (16384, 256) and np.isfinite(s).all()
    assert os.path.getsize(tmp_path / "scores.npy") <= 64_000_000
    assert r["dump_outputs"]["arrays"]["scores"]["of_shape"] == [1_000_000, 256]


@pytest.mark.parametrize("ranks", [2, 4])      # (four ranks + this process on the one card: the box allows six)
def test_gpus_n_launches_its_ranks_by_itself(gpu_ctx, ranks):
    rc, out, err = _run(["--gpus", str(ranks), "--steps", "2", "--warmup", "1", "--c5-rows", "20000"], MSC_BENCH_BACKEND="gloo")
    assert rc == 0, err[-2000:]
    r = _line(out)
    assert r["n_gpus"] == ranks and r["ranks_seen"] == ranks and len(r["rank_devices"]) == ranks
    assert r["steps"] == 2 and r["warmup"] == 1
    assert r["metric"] == "Gibbs-sweep rows/sec" and r["scaling"] == "weak" and r["config"]["backend"] == "gloo"
    assert r["one_rank_reference"]["value"] > 0 and r["weak_scaling_eff"] > 0


def test_gpus_2_over_rccl_on_a_one_gpu_box_fails_loudly(gpu_ctx):
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU here")
    rc, out, err = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--c5-rows", "20000"])
    assert rc != 0 and "GPU(s) visible" in err and not [ln for ln in out.splitlines() if ln.startswith("{")]
