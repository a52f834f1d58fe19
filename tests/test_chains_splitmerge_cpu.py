"""The ensemble's split-merge call, without a GPU: the ABI declares and exports msc_chains_split_merge and the binding
carries its argument types; ChainEnsemble has split_merge and run takes split_merge=; the argument errors that need no
device; and the float64 numpy yardstick (sm_helpers.Yardstick) behind the bars of tests/test_gpu_chains_splitmerge.py, at a
reduced size."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "msc_chains_split_merge"
SIG = ("int msc_chains_split_merge(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t nrows, "
       "uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, uint32_t nproposals, uint32_t launch_iters, "
       "const uint64_t *host_seeds, uint64_t sweep, double *log_dev, int32_t *trace_dev, int32_t *proposed_dev, "
       "uint64_t *counters_dev);")


def test_header_declares_and_library_exports_the_call():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    import common_amd
    assert SIG in flat
    assert hasattr(C.CDLL(common_amd.LIB_PATH), NAME)
    assert NAME in common_amd.EXPORTS
    assert "#define MSC_ABI_VERSION 1" in flat
    # the header says what the call needs of the members' tables
    assert "EVERY TABLE OF EVERY MEMBER MUST BE THAT OF ITS z ROW" in flat


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    lib = L.load()          # dlopen only; no device call
    res, args = L._SIGS[NAME]
    params = re.search(NAME + r"\((.*?)\);", SIG).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 15
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(C.c_uint64)), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    assert args[9] == C.POINTER(C.c_uint64)         # host_seeds: 64-bit keys
    assert getattr(lib, NAME).argtypes == args


def test_python_surface():
    import common_amd
    from common_amd import chains
    assert callable(common_amd.ChainEnsemble.split_merge)
    sm = inspect.signature(common_amd.ChainEnsemble.split_merge).parameters
    assert [(k, v.default) for k, v in sm.items()][2:] == [
        ("seed", inspect.Parameter.empty), ("sweep", 0), ("nproposals", 1), ("launch_iters", 2), ("want_log", False),
        ("want_trace", False), ("want_proposed", False), ("row_id0", 0)]
    run = inspect.signature(common_amd.ChainEnsemble.run).parameters
    assert "split_merge" in run and run["split_merge"].default is None
    assert chains.RunResult._fields == ("trace", "values")
    assert chains.SplitMergeResult._fields == ("counters", "log", "trace", "proposed")
    assert "split_merge" in common_amd.ChainEnsemble.run.__doc__


def test_argument_errors_that_need_no_device():
    from common_amd.chains import split_merge_args
    assert split_merge_args(7, 3, 4, 2) == ([7, 8, 9], 4, 2)
    assert split_merge_args([5, 1, 9], 3, 0, 1024) == ([5, 1, 9], 0, 1024)
    with pytest.raises(ValueError):
        split_merge_args([1, 2], 3, 1, 2)            # seeds of the wrong length
    with pytest.raises(ValueError):
        split_merge_args(1, 3, -1, 2)                # negative nproposals
    with pytest.raises(ValueError):
        split_merge_args(1, 3, 1, 1025)              # launch_iters beyond 1024
    with pytest.raises(ValueError):
        split_merge_args(1, 3, 1, -1)


def test_yardstick_behind_the_gpu_bars_at_a_reduced_size():
    """The GPU tests quote sm_helpers.Yardstick at 64 generators x 800 proposals (six rows: TV 0.021 - 0.034) and on 32
    seeds (two clusters: 31 of 32).  Here the same yardstick at an eighth of the six-row size -- 16 generators x 400
    proposals, pooled as the GPU test pools its chains -- whose Monte Carlo error is sqrt(8) times the full size's: TV
    below 0.034 sqrt(8) = 0.097; and on four seeds of the two-cluster data, of which at least three must reach 0.99."""
    from oracle import oracle as orc
    from tests import seq_helpers as sh
    from tests import sm_helpers as smh
    feats = smh.six_row_datasets()["bb3"]
    Fs = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"]) for f in feats]
    parts, p = sh.exact_posterior(Fs, 1.0)
    trace = []
    for g in range(16):
        y = smh.Yardstick(feats, 1.0, 32, 100 + g)
        z = np.zeros(6, dtype=np.int64)
        for _ in range(400):
            y.propose(z, 0)
            trace.append(z.copy())
        assert y.counts[4] == 0 and y.counts[0] + y.counts[2] == 400
    tv, kl = sh.tv_kl(sh.partition_frequencies(np.stack(trace), parts), p)
    print("yardstick bb3, 16 x 400 proposals: TV %.4f KL %.5f" % (tv, kl))
    assert tv <= 0.097, tv
    feats, truth = smh.two_cluster_data()
    good = 0
    for seed in range(4):
        y = smh.Yardstick(feats, 1.0, 8, seed)
        z = np.zeros(len(truth), dtype=np.int64)
        for _ in range(20):
            y.propose(z, 3)
        share, agree = smh.two_largest_agree(z, truth)
        good += share >= 0.99 and agree >= 0.99
    assert good >= 3, good
