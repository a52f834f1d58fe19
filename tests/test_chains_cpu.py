"""Many sequential chains in one launch, without a GPU: the ABI declares and exports the four msc_chains_* calls, the
binding carries their argument types, the ensemble's pure helpers (trace shape, per-chain keys) are right, and the
yardstick of the pooled-chains GPU test (many short chains of the double replay against the exact posterior) holds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import seq_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = (
    "int msc_chains_create(msc_state *const *states, uint32_t nchains, msc_chains **out);",
    "int msc_chains_destroy(msc_chains *ch);",
    "int msc_chains_size(const msc_chains *ch, uint32_t *nchains);",
    "int msc_chains_sweep(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows, "
    "uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order, uint32_t nsweeps, "
    "const uint64_t *host_seeds, uint64_t sweep, uint32_t trace_every, int32_t *trace_dev, uint32_t *occupied_dev);",
)
NAMES = ("msc_chains_create", "msc_chains_destroy", "msc_chains_size", "msc_chains_sweep")


def test_header_declares_and_library_exports_the_chains_calls():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    for sig in SIGS:
        assert sig in flat, sig
    assert "typedef struct msc_chains msc_chains;" in flat
    import common_amd
    lib = C.CDLL(common_amd.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in common_amd.EXPORTS


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    assert L._SIGS["msc_chains_create"] == (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)])
    assert L._SIGS["msc_chains_destroy"] == (C.c_int, [C.c_void_p])
    assert L._SIGS["msc_chains_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)])
    res, args = L._SIGS["msc_chains_sweep"]
    # one ctypes argument per parameter of the declaration, 64-bit where it says uint64_t, 32-bit where uint32_t
    params = re.search(r"msc_chains_sweep\((.*?)\);", re.sub(r"\s+", " ", SIGS[3])).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 16
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(C.c_uint64)), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    lib = L.load()          # dlopen only; no device call
    assert lib.msc_chains_sweep.argtypes == args


def test_trace_shape():
    from common_amd.chains import trace_shape
    assert trace_shape(6, 1, 4, 10) == (4, 6, 10)
    assert trace_shape(6, 3, 4, 10) == (4, 2, 10)
    assert trace_shape(7, 2, 5, 37) == (5, 3, 37)        # nsweeps not a multiple: the last sweep leaves no sample
    assert trace_shape(3, 4, 2, 9) == (2, 0, 9)          # trace_every > nsweeps: no sample
    assert trace_shape(0, 1, 2, 9) == (2, 0, 9)
    with pytest.raises(ValueError):
        trace_shape(5, 0, 1, 1)
    with pytest.raises(ValueError):
        trace_shape(-1, 1, 1, 1)


def test_chain_seeds():
    from common_amd.chains import chain_seeds
    assert chain_seeds(77, 4) == [77, 78, 79, 80]                         # an int: chain c takes seed + c
    assert chain_seeds(np.int64(5), 2) == [5, 6]
    assert chain_seeds((1 << 64) - 1, 3) == [(1 << 64) - 1, 0, 1]         # ... as a 64-bit key
    assert chain_seeds([9, 3, 9], 3) == [9, 3, 9]                         # a sequence: as given
    with pytest.raises(ValueError):
        chain_seeds([1, 2], 3)
    with pytest.raises(ValueError):
        chain_seeds([1, -2], 2)


def test_ensemble_is_exported():
    import common_amd
    assert common_amd.ChainEnsemble is common_amd.chains.ChainEnsemble and "ChainEnsemble" in common_amd.__all__


def test_pooled_short_chains_of_the_replay_stay_inside_the_gate():
    """The GPU test pools 250 chains x 800 sweeps, each seated from all-unassigned, and gates TV <= 0.05 against the exact
    posterior.  Two terms: sampling noise, TV ~ 0.013 at 2e5 samples over 203 partitions and growing as 1 / sqrt(samples),
    and the seating transient every chain carries, a share <= burn / sweeps of its samples.  The replay is the same chain
    in double; here it runs 25 chains x 80 sweeps (1 / 100 of the samples, the transient's share ten times the GPU
    test's), so the gate's noise term scales by 10: 0.05 + 9 * 0.013 = 0.167 -- pooling short seated chains reaches the
    posterior, it does not stall at the seating distribution."""
    from tests.gpu_helpers import make_feature
    rng = np.random.default_rng(2024)
    N, K, alpha, chains, sweeps = 6, 7, 1.0, 25, 80
    feats = [make_feature(orc.BB, N, 2, rng) for _ in range(3)]
    Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
    rfeats = [(F, f["values"]) for F, f in zip(Fs, feats)]
    parts, p = sh.exact_posterior(rfeats, alpha)
    traces = np.empty((chains, sweeps, N), np.int32)
    rows = np.arange(N)
    for c in range(chains):
        rp = sh.Replay(rfeats, K, alpha, np.full(N, -1, np.int32))
        for s in range(sweeps):
            rp.sweep(rows, 77 + c, s, rows)
            traces[c, s] = rp.z
    tv, kl = sh.tv_kl(sh.partition_frequencies(traces.reshape(-1, N), parts), p)
    print("pooled replay, %d chains x %d sweeps: TV %.4f KL %.5f" % (chains, sweeps, tv, kl))
    assert tv <= 0.05 + 9 * 0.013, (tv, kl)
