"""The posterior-averaged row predictive density of an ensemble, host side: the entry point in the header, the binding and
the built library, and the reductions of common_amd/csrc/chains_merge.hpp built with the host compiler -- the weights'
normalisation, the weighted merge over chains and slices, and a chain's sum over its groups -- against scipy's
logsumexp in float64.  No device needed.

Bounds.  mix is (float)(M + log S) with M, S and the terms in double: the sums of at most 300 terms carry some 300 x
1.1e-16 of relative error in S, i.e. < 1e-13 absolute in the logarithm; the one rounding to float is half an ulp,
6e-8 |want|.  So |mix - want| <= 1e-7 max(1, |want|).  A chain's L keeps its maximum in float and takes exp2 / log2 in
float (1 ulp each on the device): the plain gate of the project, 1e-6 max(1, |want|)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import logsumexp

import common_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "msc_chains_score_marginal"
SIG = ("int msc_chains_score_marginal(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, "
       "uint64_t nrows, const uint32_t *features, uint32_t nfeatures, const double *logw_dev, uint32_t flags, "
       "float *mix_dev, float *chain_logp_dev, uint64_t ld_logp);")


def test_header_declares_and_library_exports_the_call():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert SIG in flat
    assert "#define MSC_ABI_VERSION 1" in flat
    assert NAME in common_amd.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    assert re.search(r" T %s$" % NAME, out, re.M)
    assert callable(getattr(common_amd.ChainEnsemble, "predictive_logp"))


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    res, args = L._SIGS[NAME]
    # one ctypes argument per parameter of the declaration, 64-bit where it says uint64_t, 32-bit where uint32_t
    params = re.search(NAME + r"\((.*?)\);", SIG).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 12
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(C.c_uint32)), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    lib = L.load()          # dlopen only; no device call
    assert getattr(lib, NAME).argtypes == args
    assert lib.msc_abi_version() == 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cmerge") / "chains_merge_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "chains_merge_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.cm_weights.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.cm_mix.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.cm_mix.restype = C.c_float
    lib.cm_merge_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.cm_merge_parts.restype = C.c_float
    lib.cm_row.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    lib.cm_row.restype = C.c_double
    return lib


def weights(lib, logw):
    logw = np.ascontiguousarray(logw, dtype=np.float64)
    lw = np.empty_like(logw)
    lib.cm_weights(logw.ctypes.data, logw.size, lw.ctypes.data)
    return lw


def mix(lib, lw, L, nslices):
    lw, L = np.ascontiguousarray(lw, dtype=np.float64), np.ascontiguousarray(L, dtype=np.float64)
    return float(lib.cm_mix(lw.ctypes.data, L.ctypes.data, L.size, nslices))


def test_weights_are_normalised_in_double(host):
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 256, 257, 700):
        logw = rng.uniform(-800.0, 300.0, n)
        logw[rng.random(n) < 0.3] = -np.inf
        if np.isinf(logw).all():
            logw[0] = 3.0
        lw = weights(host, logw)
        want = logw - logsumexp(logw)
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(lw), np.isneginf(want))
        assert np.all(np.abs(lw[fin] - want[fin]) <= 1e-12 * np.maximum(1.0, np.abs(want[fin])))
        assert abs(logsumexp(lw)) <= 1e-12
    # one-hot: exactly zero for the chain, -inf for the others, whatever the finite value
    for v in (0.0, -3.25, 1e3):
        lw = weights(host, [-np.inf, v, -np.inf])
        assert lw[1] == 0.0 and np.isneginf(lw[0]) and np.isneginf(lw[2])
    # nothing to normalise by: NaN for every chain
    for bad in ([-np.inf, -np.inf], [0.0, np.nan], [np.inf, 1.0]):
        assert np.isnan(weights(host, bad)).all()


@pytest.mark.parametrize("nslices", [1, 2, 3, 4, 5, 6, 7])
def test_the_weighted_merge_against_scipy(host, nslices):
    rng = np.random.default_rng(10 + nslices)
    for n in (1, 2, 7, 52, 70, 300):
        for trial in range(20):
            logw = rng.uniform(-30.0, 5.0, n)
            L = rng.uniform(-3000.0, 50.0, n) if trial % 2 else rng.uniform(-40.0, -20.0, n)
            if n > 1:
                logw[rng.random(n) < 0.2] = -np.inf                       # chains left out
                L[rng.random(n) < 0.2] = -np.inf                          # rows a chain cannot hold
            if np.isinf(logw).all():
                logw[rng.integers(n)] = 0.5
            lw = weights(host, logw)
            got = mix(host, lw, L, min(nslices, n))
            with np.errstate(invalid="ignore"):
                terms = np.where(np.isneginf(logw) | np.isneginf(L), -np.inf, logw - logsumexp(logw) + L)
            want = logsumexp(terms) if np.isfinite(terms).any() else -np.inf
            if np.isneginf(want):
                assert np.isneginf(got)
            else:
                assert abs(got - want) <= 1e-7 * max(1.0, abs(want)), (n, nslices, trial, got, want)


def test_a_single_chain_and_one_hot_weights_reproduce_the_chains_row_bit_for_bit(host):
    rng = np.random.default_rng(3)
    for n, nslices in ((1, 1), (5, 1), (5, 3), (70, 7), (70, 35)):
        for _ in range(50):
            L = rng.uniform(-500.0, 20.0, n)
            c = int(rng.integers(n))
            logw = np.full(n, -np.inf)
            logw[c] = rng.uniform(-10.0, 10.0)
            got = mix(host, weights(host, logw), L, nslices)
            assert np.float32(got).tobytes() == np.float32(L[c]).tobytes()


def test_no_finite_weight_is_nan_and_no_finite_term_is_minus_infinity(host):
    L = np.array([-3.0, -4.0, -5.0])
    for nslices in (1, 2, 3):
        assert np.isnan(mix(host, weights(host, [-np.inf] * 3), L, nslices))
        assert np.isneginf(mix(host, weights(host, [0.0, 0.0, -np.inf]), [-np.inf, -np.inf, -1.0], nslices))


def test_slices_are_merged_in_ascending_order(host):
    """cm_mix over s slices IS: each slice's (M, S) over its consecutive chains pushed in ascending order, then the
    parts merged first to last -- rebuilt here from explicit parts, bit for bit"""
    rng = np.random.default_rng(4)
    for n, nslices in ((7, 2), (70, 7), (70, 35), (300, 5)):
        lw = weights(host, rng.uniform(-5.0, 5.0, n))
        L = rng.uniform(-60.0, -10.0, n)
        per = -(-n // nslices)
        M, S = [], []
        for s in range(nslices):
            u = (lw + L)[s * per:(s + 1) * per]
            m, acc = -np.inf, 0.0
            for x in u:                                                   # w_push, with the C library's exp
                if x > m:
                    acc = acc * math.exp(m - x) + 1.0
                    m = x
                else:
                    acc += math.exp(x - m)
            M.append(m)
            S.append(acc)
        M, S = np.array(M), np.array(S)
        parts = float(host.cm_merge_parts(M.ctypes.data, S.ctypes.data, nslices))
        got = mix(host, lw, L, nslices)
        want = logsumexp(lw + L)
        assert abs(parts - want) <= 1e-7 * max(1.0, abs(want))
        # the C library's exp on both sides: the same bits
        assert np.float32(got).tobytes() == np.float32(parts).tobytes()


@pytest.mark.parametrize("K", [1, 7, 8, 9, 40, 64, 1000, 8192])
def test_a_chains_row_against_scipy(host, K):
    rng = np.random.default_rng(K)
    for trial in range(30):
        t = rng.uniform(-3000.0, 10.0, K).astype(np.float32) if trial % 2 else (rng.uniform(-2.0, 0.0, K) - 77.0).astype(np.float32)
        if K > 1:
            t[rng.random(K) < 0.3] = -np.inf
        if np.isinf(t).all():
            t[rng.integers(K)] = -7.0
        norm = float(rng.uniform(0.0, 15.0))
        got = host.cm_row(t.ctypes.data, K, norm)
        want = logsumexp(t.astype(np.float64)) - norm
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (K, trial, got, want)
    t = np.full(K, -np.inf, dtype=np.float32)
    assert np.isneginf(host.cm_row(t.ctypes.data, K, 1.0))


# ---- the yardstick of the GPU suite's end-to-end test, on the oracle alone -------------------------------------------
@pytest.mark.parametrize("name", ["bb", "nich"])
def test_the_partition_ensemble_identity_holds_in_double(name):
    """one chain per set partition of five rows, weighted by the partitions' exact posterior: the average of the chains'
    predictive densities of a sixth row IS p(x_6 | x_1..5) = p(x_1..6) / p(x_1..5).  Both sides from the float64 oracle,
    by routes that share only its score functions: 1e-10.  (With the suff-stats rounded to the float fields the device
    holds, as the GPU test's twin has them, the nich answer moves by 1.3e-8: far inside that test's gate.)"""
    from tests import chains_marginal_helpers as M
    from tests import smc_helpers as H
    twin, logw, exact = M.partition_twin(H.six_row_datasets()[name][0], 1.0, narrow=False)
    assert twin.nchains == 52 and abs(logsumexp(logw)) < 1e-12
    want, gate = twin.all_chains(np.arange(1))
    mixed, _ = twin.mix(want, gate, logw)
    assert abs(mixed[0] - exact) <= 1e-10, (mixed[0], exact)


def test_the_float_suff_stats_the_device_holds_move_that_answer_by_less_than_2e_8():
    """the GPU test's twin rounds every chain's suff-stats to the float fields the device holds; its bound carries 2e-8
    for what that does to the identity (nich: 1.3e-8, bb: counts are exact).  Held here, on the oracle alone."""
    from tests import chains_marginal_helpers as M
    from tests import smc_helpers as H
    for name in ("bb", "nich"):
        twin, logw, exact = M.partition_twin(H.six_row_datasets()[name][0], 1.0, narrow=True)
        want, gate = twin.all_chains(np.arange(1))
        mixed, _ = twin.mix(want, gate, logw)
        assert abs(mixed[0] - exact) <= 2e-8, (name, mixed[0], exact)
