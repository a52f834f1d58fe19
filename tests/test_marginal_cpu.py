"""Row predictive log-density, host side: the entry point in the header, the binding and the built library, and the
reduction of common_amd/csrc/lse_merge.hpp built with the host compiler -- log-sum-exp and arg-max of rows in the two
chunkings the kernels use, against scipy in float64.  No device needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import logsumexp

import common_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 63, 64, 65, 256, 1000, 8192]


def test_header_binding_and_library_declare_the_entry_point():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        hdr = fh.read()
    assert re.search(r"int msc_score_marginal\(", hdr) and re.search(r"int msc_state_get_alpha\(", hdr)
    assert "msc_score_marginal" in common_amd.EXPORTS and "msc_state_get_alpha" in common_amd.EXPORTS
    assert hasattr(common_amd.State, "get_alpha")
    assert hasattr(common_amd.State, "predictive_logp") and hasattr(common_amd.State, "subset")
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    assert re.search(r" T msc_score_marginal$", out, re.M) and re.search(r" T msc_state_get_alpha$", out, re.M)
    assert common_amd.load().msc_abi_version() == 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lse") / "lse_merge_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "lse_merge_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.lse_row.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def reduce_row(lib, mode, v, log_norm=0.0):
    v = np.ascontiguousarray(v, dtype=np.float32)
    logp, lr, k = C.c_float(), C.c_float(), C.c_int32()
    lib.lse_row(mode, v.ctypes.data, v.size, log_norm, C.byref(logp), C.byref(k), C.byref(lr))
    return logp.value, k.value, lr.value


def check(lib, mode, v, log_norm=0.0):
    v = np.asarray(v, dtype=np.float32)
    logp, k, lr = reduce_row(lib, mode, v, log_norm)
    lse = logsumexp(v.astype(np.float64))
    want = lse - log_norm
    assert abs(logp - want) <= 1e-6 * max(1.0, abs(want)), (mode, v.size, logp, want)
    assert k == int(np.argmax(v)), (mode, v.size)                       # (numpy: the first index of the maximum)
    want_lr = float(v.max()) - lse
    assert abs(lr - want_lr) <= 1e-6 * max(1.0, abs(want_lr)) and lr <= 0.0


# (mode 1 is the fused kernels' chunking, which holds at most 16 entries a lane: K <= 1024)
@pytest.mark.parametrize("mode,K", [(0, K) for K in KS] + [(1, K) for K in KS if K <= 1024])
def test_rows_against_scipy(host, mode, K):
    rng = np.random.default_rng(1000 * mode + K)
    for trial in range(40):
        v = rng.uniform(-3000.0, 10.0, K)                                # most terms underflow against the maximum
        check(host, mode, v, log_norm=float(rng.uniform(0.0, 15.0)))
        w = v.copy()
        w[rng.random(K) < 0.3] = -np.inf                                 # empty entries
        if np.isinf(w).all():
            w[rng.integers(K)] = -7.0
        check(host, mode, w)
        near = rng.uniform(-2.0, 0.0, K) + rng.uniform(-500, 500)        # many terms of the same size
        check(host, mode, near)
        tie = near.astype(np.float32)
        tie[rng.integers(0, K, 3)] = tie.max()                           # exact ties: the lowest index
        check(host, mode, tie)
    check(host, mode, np.full(K, -12.25))                                # all equal: log K above the value, index 0
    check(host, mode, np.zeros(K))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1, 64, 65, 1000])
def test_a_row_of_minus_infinity_is_minus_infinity_at_index_zero(host, mode, K):
    logp, k, lr = reduce_row(host, mode, np.full(K, -np.inf))
    assert logp == -np.inf and k == 0 and not np.isnan(lr)
