"""Posterior predictive draws from a chain ensemble, host side: the entry point in the header, the binding and the built
library; the two discrete draws of common_amd/csrc/chains_pick.hpp built with the host compiler against a numpy float64
restatement of the running-sum rule; the draw's Philox block against the oracle's; and the caps on undecided rows that
tests/test_gpu_chains_predictive.py works under, checked on the double twin alone.  No device needed.

The host build and numpy form the same sums of the same terms in the same order; they differ by the last bits of exp
alone.  A comparison is therefore made only where u S stands clear of every running sum by more than 1e-12 n S (the
rule of tests/chains_predictive_helpers.py for an undecided row); the terms and uniforms here are seeded, and at least
999 in 1000 of the random draws are compared.  The ends of u, which sit on a running sum, are held to what they must give."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common_amd
from oracle import oracle as orc
from tests import chains_predictive_helpers as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "msc_chains_sample_predictive"
SIG = ("int msc_chains_sample_predictive(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, "
       "uint64_t nrows, uint64_t row_id0, const double *logw_dev, uint32_t flags, uint64_t seed, uint64_t sweep, "
       "int32_t *chain_out_dev, int32_t *z_out_dev, void *const *out_dev);")


def test_header_declares_and_library_exports_the_call():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert SIG in flat
    assert "#define MSC_ABI_VERSION 1" in flat
    assert NAME in common_amd.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    assert re.search(r" T %s$" % NAME, out, re.M)
    assert callable(getattr(common_amd.ChainEnsemble, "sample_predictive"))
    assert callable(getattr(common_amd.ChainEnsemble, "impute"))


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    res, args = L._SIGS[NAME]
    params = re.search(NAME + r"\((.*?)\);", SIG).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 13
    for p, a in zip(params, args):
        if "*" in p:
            assert a is C.c_void_p, p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    lib = L.load()          # dlopen only; no device call
    assert getattr(lib, NAME).argtypes == args
    assert lib.msc_abi_version() == 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpick") / "chains_pick_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "chains_pick_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.cp_words.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.cp_uniforms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.cp_pick.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    lib.cp_pick.restype = C.c_int32
    lib.cp_group.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    lib.cp_group.restype = C.c_int32
    return lib


def host_pick(host, a, u):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return int(host.cp_pick(a.ctypes.data, len(a), float(u)))


def host_group(host, t, u):
    t = np.ascontiguousarray(t, dtype=np.float32)
    return int(host.cp_group(t.ctypes.data, len(t), float(u)))


SIZES = (1, 2, 7, 70, 300)
JUST_BELOW_1 = float(np.nextafter(1.0, 0.0))


def test_the_block_of_the_draw_is_the_oracles_philox(host):
    for seed, R, sweep in ((0, 0, 0), (73, 5, 2), (2 ** 64 - 1, 2 ** 40 + 17, 2 ** 32 + 9), (P.SEED, 4099, P.SWEEP)):
        key = seed ^ P.PICK_KEY
        want = orc.philox([key & 0xffffffff, key >> 32], [R & 0xffffffff, R >> 32, sweep & 0xffffffff, 0x80000000])
        got = np.zeros(4, dtype=np.uint32)
        host.cp_words(seed, R, sweep, got.ctypes.data)
        assert np.array_equal(got, want), (seed, R, sweep)
        assert np.array_equal(P.pick_words(seed, [R], sweep)[0], want)          # (the helpers' numpy form, which the GPU tests use)
        u = np.zeros(2)
        host.cp_uniforms(seed, R, sweep, u.ctypes.data)
        w = want.astype(np.uint64)
        for i in (0, 1):
            a, b = int(w[2 * i]), int(w[2 * i + 1])
            assert u[i] == ((a >> 5) * 2.0 ** 26 + (b >> 6) + 0.5) * 2.0 ** -53
            assert 0.0 < u[i] < 1.0
        u1, u2 = P.uniforms(seed, [R], sweep)
        assert (u1[0], u2[0]) == (u[0], u[1])


@pytest.mark.parametrize("n", SIZES)
def test_the_chain_draw_is_the_running_sum_rule(host, n):
    rng = np.random.default_rng(100 + n)
    compared = 0
    for trial in range(40):
        a = rng.uniform(-12.0, 3.0, n)
        if n > 1 and trial % 2:
            a[rng.random(n) < 0.3] = -np.inf                              # chains of weight -inf, rows a chain cannot hold
            a[int(rng.integers(n))] = rng.uniform(-12.0, 3.0)             # (one term stays finite)
        for u in rng.random(5):
            want, undecided = P.chain_rule(np.zeros(n), a[:, None], np.array([u]))
            if undecided[0]:
                continue
            compared += 1
            assert host_pick(host, a, u) == int(want[0]), (n, trial, u)
        # the ends of u sit ON a running sum (0, and S to within rounding), which the rule above calls undecided; what
        # they give is fixed all the same: the first and the last term that counts (by a hit or by the fallback)
        live = np.flatnonzero(np.isfinite(a))
        assert host_pick(host, a, 0.0) == live[0] and host_pick(host, a, JUST_BELOW_1) == live[-1]
    assert compared >= 0.999 * 40 * 5


@pytest.mark.parametrize("n", SIZES)
def test_one_hot_terms_choose_that_index_for_every_u(host, n):
    for hot in sorted({0, n // 2, n - 1}):
        a = np.full(n, -np.inf)
        a[hot] = -3.25
        for u in (0.0, 1e-300, 0.25, 0.5, JUST_BELOW_1):
            assert host_pick(host, a, u) == hot
            assert host_group(host, a, u) == hot
            assert int(P.chain_rule(np.zeros(n), a[:, None], np.array([u]))[0][0]) == hot


@pytest.mark.parametrize("n", SIZES)
def test_nothing_finite_or_a_nan_or_plus_inf_skips_the_row(host, n):
    assert host_pick(host, np.full(n, -np.inf), 0.5) == -1
    assert host_group(host, np.full(n, -np.inf), 0.5) == -1
    for poison in (np.nan, np.inf):
        a = np.linspace(-2.0, 1.0, n)
        a[n // 2] = poison
        assert host_pick(host, a, 0.5) == -1
        assert int(P.chain_rule(np.zeros(n), a[:, None], np.array([0.5]))[0][0]) == -1


@pytest.mark.parametrize("n", SIZES)
def test_u_at_zero_takes_the_first_live_term_and_the_fallback_the_last(host, n):
    rng = np.random.default_rng(n)
    a = rng.uniform(-4.0, 0.0, n)
    dead = np.zeros(n, dtype=bool)
    if n > 2:
        dead[0] = dead[n - 1] = True                                      # (the live terms start at 1 and end at n - 2)
    a[dead] = -np.inf
    live = np.flatnonzero(~dead)
    assert host_pick(host, a, 0.0) == live[0]
    assert host_group(host, a, 0.0) == live[0]
    # u = 1 is beyond what the uniforms reach: no running sum exceeds 1 * S, so the rule falls back to the last term
    # that counts -- what keeps a row whose u S rounds up to S from being left without an index
    assert host_pick(host, a, 1.0) == live[-1]
    assert host_group(host, a, 1.0) == live[-1]
    assert int(P.running_pick(a[:, None], np.array([1.0]))[0][0]) == live[-1]


@pytest.mark.parametrize("n", SIZES)
def test_the_group_draw_is_the_running_sum_rule_too(host, n):
    """totals as the kernel holds them (float), the sum formed online: the rule within the group draw's own margin"""
    rng = np.random.default_rng(200 + n)
    compared = 0
    for trial in range(40):
        t = rng.uniform(-40.0, 0.0, n).astype(np.float32)
        for u in rng.random(5):
            want, undecided = P.chain_rule(np.zeros(n), t.astype(np.float64)[:, None], np.array([u]))
            if undecided[0]:
                continue
            compared += 1
            assert host_group(host, t, u) == int(want[0]), (n, trial, u)
    assert compared >= 0.999 * 40 * 5


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_the_gpu_tests_cases_stay_within_the_caps_on_undecided_rows(name):
    """on the double twin and the Philox uniforms alone: the share of rows whose chain (<= 1 in 1000) or group (<= 5 %)
    the comparison cannot decide.  A case that does not fit is changed, not the cap."""
    twin = P.twin_of(name)
    n = len(twin.held[0]["values"])
    rows = np.arange(n)
    u1, u2 = P.uniforms(P.SEED, rows, P.SWEEP)
    L, _ = twin.all_chains(rows)
    for logw in (None, P.weights_of(name)):
        from tests.chains_marginal_helpers import normalised
        chains, und_c = P.chain_rule(normalised(logw, twin.nchains), L, u1)
        assert (chains >= 0).all()
        und_g = np.zeros(n, dtype=bool)
        for c in np.unique(chains):
            mine = np.flatnonzero(chains == c)
            _, und = P.group_rule(P.twin_totals(twin, int(c), mine), u2[mine])
            und_g[mine] = und
        print("%s: %d rows, undecided chain %.5f, undecided group %.4f" % (name, n, und_c.mean(), und_g.mean()))
        assert und_c.mean() <= P.CHAIN_CAP
        assert und_g.mean() <= P.GROUP_CAP
