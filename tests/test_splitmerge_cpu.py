"""The split-merge move, host side: common_amd/csrc/splitmerge_math.hpp built with the host compiler -- the log
acceptance ratio against the f64 oracle, the two-way log-probabilities at extreme gaps, the key and the streams -- and the
entry points in the header and the binding.  No device needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import common_amd
from oracle import oracle as orc
from tests import sm_helpers as smh
from tests.gpu_helpers import make_feature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("splitmerge") / "splitmerge_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "splitmerge_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    u64, u32, d, vp = C.c_uint64, C.c_uint32, C.c_double, C.c_void_p
    lib.sm_key.restype = u64
    lib.sm_stream_stride.restype = u64
    lib.sm_stream_key.restype = u64
    lib.sm_stream_key.argtypes = [u64, u32]
    lib.sm_stream_tags.argtypes = [vp]
    lib.sm_uniform01.restype = C.c_float
    lib.sm_uniform01.argtypes = [u64, u64, u64]
    lib.sm_anchors.argtypes = [u64, u64, u64, vp, vp]
    lib.sm_two_way.argtypes = [C.c_float, C.c_float, vp]
    lib.sm_log_crp_split.restype = d
    lib.sm_log_crp_split.argtypes = [d, d, d]
    lib.sm_log_accept.restype = d
    lib.sm_log_accept.argtypes = [u32, d, d, d, d, d, d, d]
    return lib


CASES = {
    "bb": [(orc.BB, 0)],
    "gp": [(orc.GP, 0)],
    "bnb": [(orc.BNB, 0)],
    "dd5": [(orc.DD, 5)],
    "nich": [(orc.NICH, 0)],
    "mix": [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 5), (orc.NICH, 0)],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_log_accept_against_the_oracle(host, case):
    """random two-block divisions of 12 rows: the CRP term as the difference of the oracle's score_assignment, the
    likelihood terms from Family.score_data_all, both sides double: 1e-9 relative"""
    rng = np.random.default_rng(sum(map(ord, case)))
    N, alpha = 12, 0.75                                       # (exact as a float: score_assignment takes a float)
    feats = [make_feature(f, N, 2, rng, d) for f, d in CASES[case]]
    Fs = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"]) for f in feats]
    for trial in range(20):
        lab = rng.integers(0, 2, N)
        lab[rng.integers(N)] = 0
        lab[(np.nonzero(lab == 0)[0][0] + 1 + rng.integers(N - 1)) % N] = 1      # both blocks hold a row
        if (lab == 0).sum() == 0 or (lab == 1).sum() == 0:
            continue
        rows0, rows1 = np.nonzero(lab == 0)[0], np.nonzero(lab == 1)[0]
        logq = float(-rng.gamma(2.0, 3.0))
        sd0, sd1, sdS = (smh.block_score(Fs, r)[0] for r in (rows0, rows1, np.arange(N)))
        for kind in (smh.SPLIT, smh.MERGE):
            want, _ = smh.log_accept(Fs, alpha, rows0, rows1, kind, logq)
            got = host.sm_log_accept(kind, math.log(alpha), float(len(rows0)), float(len(rows1)), sd0, sd1, sdS, logq)
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (case, trial, kind, got, want)
        # a split's ratio is the inverse of the merge that undoes it
        assert host.sm_log_accept(smh.SPLIT, 0.3, 5.0, 7.0, sd0, sd1, sdS, logq) == \
            -host.sm_log_accept(smh.MERGE, 0.3, 5.0, 7.0, sd0, sd1, sdS, logq)


def test_crp_term_is_the_difference_of_score_assignment(host):
    for n0, n1, alpha in ((1, 1, 1.0), (3, 9, 0.5), (700, 2, 2.0), (40000, 60000, 1.0)):
        za = np.concatenate([np.zeros(n0), np.ones(n1)]).astype(np.int32)
        want = orc.score_assignment(za, alpha) - orc.score_assignment(np.zeros(n0 + n1, dtype=np.int32), alpha)
        got = host.sm_log_crp_split(math.log(alpha), float(n0), float(n1))
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (n0, n1, got, want)


@pytest.mark.parametrize("gap", [-200.0, -88.0, -20.0, -1e-3, 0.0, 1e-3, 20.0, 88.0, 200.0])
def test_two_way_log_probabilities_at_extreme_gaps(host, gap):
    out = np.zeros(3, dtype=np.float32)
    for base in (0.0, -1234.5, 1e6):
        host.sm_two_way(base, base + gap, out.ctypes.data_as(C.c_void_p))
        lp0, lp1, p0 = (float(v) for v in out)
        assert math.isfinite(lp0) and math.isfinite(lp1) and lp0 <= 0.0 and lp1 <= 0.0
        assert abs(math.exp(lp0) + math.exp(lp1) - 1.0) <= 1e-6      # float32 logs: 2^-24 each
        assert abs(p0 - math.exp(lp0)) <= 1e-6
        assert (lp1 >= lp0) == (gap >= 0 or lp1 == lp0)
    if abs(gap) == 200.0:
        # the gap is beyond float32's exp: the smaller side is exactly -|gap|, the larger exactly 0 -- the sum of the
        # probabilities is one within 1e-12
        host.sm_two_way(0.0, gap, out.ctypes.data_as(C.c_void_p))
        lp0, lp1 = float(out[0]), float(out[1])
        assert {lp0, lp1} == {0.0, -200.0}
        assert abs(math.exp(lp0) + math.exp(lp1) - 1.0) <= 1e-12


def test_key_differs_from_the_other_draws(host):
    key = host.sm_key()
    assert key == smh.KEY == common_amd._lib.SPLIT_MERGE_KEY == 0xA0761D6478BD642F
    assert key not in (0, 0x9FB21C651E98DF25, 0x2545F4914F6CDD1D, 0xD1B54A32D192ED03)
    assert host.sm_stream_stride() == smh.STRIDE == common_amd._lib.SPLIT_MERGE_STREAM_STRIDE
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        assert "0xA0761D6478BD642F" in fh.read()
    tags = np.zeros(4, dtype=np.uint32)
    host.sm_stream_tags(tags.ctypes.data_as(C.c_void_p))
    assert list(tags) == [smh.STREAM_PROPOSAL, smh.STREAM_COIN, smh.STREAM_PASS0, smh.DART_ACCEPT]
    # no stream's key of a seed is the plain seed or one of the other draws' keys of that seed
    for seed in (0, 1, 77, 2 ** 63 + 5):
        keys = [host.sm_stream_key(seed, s) for s in range(8)]
        assert len(set(keys)) == 8
        assert keys == [smh.stream_key(seed, s) for s in range(8)]
        for other in (0, 0x9FB21C651E98DF25, 0x2545F4914F6CDD1D, 0xD1B54A32D192ED03):
            assert (seed ^ other) not in keys


def test_darts_and_anchors_are_the_oracles(host):
    rng = np.random.default_rng(4)
    for _ in range(50):
        key, sweep, row = (int(v) for v in rng.integers(0, 2 ** 63, 3))
        assert host.sm_uniform01(key, sweep, row) == orc.uniform01(key, sweep, row)
    seen = set()
    for sweep in range(400):
        for n in (2, 3, 700, 10 ** 6):
            i, j = C.c_uint64(), C.c_uint64()
            host.sm_anchors(9, sweep, n, C.byref(i), C.byref(j))
            assert (i.value, j.value) == smh.anchors(9, sweep, n)
            assert i.value != j.value and i.value < n and j.value < n
            if n == 3:
                seen.add((i.value, j.value))
    assert len(seen) == 6                                      # every ordered pair of three rows turns up


def test_header_and_binding_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        hdr = fh.read()
    for name in ("msc_split_merge", "msc_split_merge_tables"):
        assert re.search(r"int %s\(" % name, hdr)
        assert name in common_amd.EXPORTS
    for name in ("split_merge", "split_merge_tables"):
        assert hasattr(common_amd.State, name)
    with open(os.path.join(ROOT, "include", "microscopes_amd", "mixture_state.hpp")) as fh:
        assert "split_merge(" in fh.read()
