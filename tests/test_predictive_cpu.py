"""Posterior predictive sampling, host side: the generators of common_amd/csrc/pred_samplers.hpp built with the host
compiler -- the Philox words against the oracle's, bit for bit, under the counter layout the header documents, and 10^6
draws of every generator against scipy -- and the new entry point in the header and the binding.  No device needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

import common_amd
from oracle import oracle as orc
from tests.gpu_helpers import audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
P_GATE = 1e-4          # a fixed-seed goodness-of-fit test of a correct generator passes this with room to spare


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pred") / "pred_samplers_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "pred_samplers_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.pred_philox.argtypes = [C.c_void_p] * 3
    lib.pred_stream_words.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pred_draw.argtypes = [C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_void_p]
    return lib


def draw(lib, kind, a, b=0.0, n=N, seed=20261015):
    out = np.empty(n, dtype=np.float64)
    lib.pred_draw(kind, a, b, n, seed, out.ctypes.data)
    return out


def test_philox_matches_the_oracle(host):
    rng = np.random.default_rng(5)
    for _ in range(64):
        key = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        ctr = rng.integers(0, 2 ** 32, 4, dtype=np.uint64).astype(np.uint32)
        got = np.zeros(4, dtype=np.uint32)
        host.pred_philox(key.ctypes.data, ctr.ctypes.data, got.ctypes.data)
        assert np.array_equal(got, orc.philox(key, ctr))


@pytest.mark.parametrize("seed,row,sweep,feature", [(0, 0, 0, 0), (73, 5, 2, 3), (2 ** 40 + 9, 2 ** 33 + 1, 2 ** 32 + 7, 31),
                                                    (123456789, 999999, 17, 0x7fff)])
def test_stream_follows_the_documented_counter_layout(host, seed, row, sweep, feature):
    n = 4 * 5
    got = np.zeros(n, dtype=np.uint32)
    host.pred_stream_words(seed, row, sweep, feature, n, got.ctypes.data)
    key = [seed & 0xffffffff, seed >> 32]
    want = np.concatenate([orc.philox(key, [row & 0xffffffff, row >> 32, sweep & 0xffffffff,
                                            0x80000000 | (feature & 0x7fff) << 16 | b]) for b in range(5)])
    assert np.array_equal(got, want)
    # no counter of the stream is a sweep's: the sweep's dart has last word sweep >> 32 < 2^31
    assert all(0x80000000 | (feature & 0x7fff) << 16 | b >= 2 ** 31 for b in range(5))


def test_uniforms_lie_strictly_inside_the_unit_interval(host):
    u = draw(host, 6, 0.0)
    assert u.min() > 0.0 and u.max() < 1.0
    audit("pred_cpu_ks_p", -stats.kstest(u, "uniform").pvalue, -P_GATE)


def test_normal(host):
    audit("pred_cpu_ks_p", -stats.kstest(draw(host, 5, 0.0), "norm").pvalue, -P_GATE)


@pytest.mark.parametrize("shape", [0.3, 1.0, 7.5, 1e4])
def test_gamma(host, shape):
    x = draw(host, 0, shape)
    audit("pred_cpu_ks_p", -stats.kstest(x, stats.gamma(shape).cdf).pvalue, -P_GATE)


@pytest.mark.parametrize("a,b", [(0.5, 0.5), (2.0, 5.0), (40.0, 3.0)])
def test_beta(host, a, b):
    audit("pred_cpu_ks_p", -stats.kstest(draw(host, 1, a, b), stats.beta(a, b).cdf).pvalue, -P_GATE)


@pytest.mark.parametrize("dof", [1.0, 3.5, 60.0])
def test_chi2(host, dof):
    audit("pred_cpu_ks_p", -stats.kstest(draw(host, 2, dof), stats.chi2(dof).cdf).pvalue, -P_GATE)


@pytest.mark.parametrize("nu", [1.0, 4.0, 250.0])
def test_student_t(host, nu):
    audit("pred_cpu_ks_p", -stats.kstest(draw(host, 3, nu), stats.t(nu).cdf).pvalue, -P_GATE)


def chi2_discrete_p(x, pmf, min_expected=20.0):
    """chi-square goodness of fit of integer draws x against pmf(k), the tails pooled until every cell expects enough"""
    n = x.size
    lo, hi = int(x.min()), int(x.max())
    ks = np.arange(lo, hi + 1)
    obs = np.bincount((x - lo).astype(np.int64), minlength=ks.size).astype(np.float64)
    exp = pmf(ks) * n
    exp[0] += pmf_tail_lo(pmf, lo) * n
    exp[-1] += max(0.0, n - exp.sum())
    cells_o, cells_e, acc_o, acc_e = [], [], 0.0, 0.0
    for o, e in zip(obs, exp):
        acc_o, acc_e = acc_o + o, acc_e + e
        if acc_e >= min_expected:
            cells_o.append(acc_o); cells_e.append(acc_e); acc_o = acc_e = 0.0
    if acc_e > 0:
        cells_o[-1] += acc_o; cells_e[-1] += acc_e
    cells_o, cells_e = np.array(cells_o), np.array(cells_e)
    cells_e *= cells_o.sum() / cells_e.sum()
    return stats.chisquare(cells_o, cells_e).pvalue


def pmf_tail_lo(pmf, lo):
    return float(np.sum(pmf(np.arange(0, lo)))) if lo > 0 else 0.0


@pytest.mark.parametrize("lam", [0.1, 3.0, 9.9, 10.1, 500.0, 1e5])
def test_poisson_across_the_inversion_ptrs_switch(host, lam):
    x = draw(host, 4, lam)
    assert np.all(x == np.floor(x)) and x.min() >= 0
    audit("pred_cpu_chi2_p", -chi2_discrete_p(x, stats.poisson(lam).pmf), -P_GATE)


def test_header_and_binding_declare_the_entry_point():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        hdr = fh.read()
    assert re.search(r"int msc_sample_predictive\(", hdr) and "MSC_PRED_MASKED_ONLY 0x1u" in hdr
    assert "msc_sample_predictive" in common_amd.EXPORTS
    assert common_amd.PRED_MASKED_ONLY == 1
    assert hasattr(common_amd.State, "sample_predictive") and hasattr(common_amd.State, "impute")
