"""The blocked Gibbs sampler, host side: common_amd/csrc/blocked_post.hpp built with the host compiler -- the map from
(hyper-parameters, suff-stats) to the conjugate posterior and 10^4 draws of every family's slices against scipy's
posterior, the stick weights, the truncation bound -- and the entry points in the header and the binding.  No device
needed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

import common_amd
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 10000
P_GATE = 1e-3
SEED = 20261018


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("blocked") / "blocked_post_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "blocked_post_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.blk_key.restype = C.c_uint64
    lib.blk_truncation_bound.restype = C.c_double
    lib.blk_truncation_bound.argtypes = [C.c_double, C.c_uint32, C.c_double]
    lib.blk_post.argtypes = [C.c_int, C.c_uint32, vp, vp, vp, vp]
    lib.blk_draw.argtypes = [C.c_int, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
    lib.blk_sticks.argtypes = [vp, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def post_and_draws(lib, family, dim, hp, su, sf, nslices, npost, n=N, seed=SEED):
    hp = np.ascontiguousarray(hp, dtype=np.float32)
    su = np.ascontiguousarray(su, dtype=np.uint32)
    sf = np.ascontiguousarray(sf if len(sf) else [0.0], dtype=np.float32)
    post = np.zeros(max(4, npost), dtype=np.float64)
    lib.blk_post(family, dim, _p(hp), _p(su), _p(sf), _p(post))
    out = np.zeros((n, nslices), dtype=np.float32)
    lib.blk_draw(family, dim, _p(hp), _p(su), _p(sf), n, seed, _p(out))
    assert np.isfinite(out).all()
    return post[:npost], out.astype(np.float64)


def ks(x, dist):
    p = stats.kstest(x, dist.cdf).pvalue
    assert p >= P_GATE, p
    return p


# suff-stat settings: an empty slot, one member, 500 members
def _values(kind, n):
    rng = np.random.default_rng(7 + n)
    if kind == "bool":
        return rng.random(n) < 0.3
    if kind == "count":
        return rng.poisson(4.0, n)
    if kind == "cat":
        return rng.integers(0, 5, n)
    return rng.normal(2.0, 1.5, n)


MEMBERS = [0, 1, 500]


def test_key_differs_from_the_other_draws(host):
    key = host.blk_key()
    assert key == 0x9FB21C651E98DF25
    assert key not in (0x2545F4914F6CDD1D, 0xD1B54A32D192ED03)
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        assert "0x9FB21C651E98DF25" in fh.read()


@pytest.mark.parametrize("n", MEMBERS)
def test_bb(host, n):
    v = _values("bool", n)
    heads, tails = int(v.sum()), int(n - v.sum())
    hp = [1.5, 0.7]
    post, d = post_and_draws(host, orc.BB, 0, hp, [heads, tails], [], 2, 2)
    assert np.allclose(post, [hp[0] + heads, hp[1] + tails], rtol=1e-7)
    ks(np.exp(d[:, 1]), stats.beta(post[0], post[1]))
    ks(np.exp(d[:, 0]), stats.beta(post[1], post[0]))          # log(1 - p) is drawn, not formed from p


@pytest.mark.parametrize("n", MEMBERS)
def test_gp(host, n):
    v = _values("count", n)
    hp = [2.0, 0.5]
    post, d = post_and_draws(host, orc.GP, 0, hp, [n, int(v.sum())], [0.0], 2, 2)
    assert np.allclose(post, [hp[0] + v.sum(), hp[1] + n], rtol=1e-7)
    ks(-d[:, 0], stats.gamma(post[0], scale=1.0 / post[1]))
    ks(np.exp(d[:, 1]), stats.gamma(post[0], scale=1.0 / post[1]))


@pytest.mark.parametrize("n", MEMBERS)
def test_bnb(host, n):
    v = _values("count", n)
    hp = [1.5, 2.0, 3.0]
    post, d = post_and_draws(host, orc.BNB, 0, hp, [n, int(v.sum())], [], 2, 2)
    assert np.allclose(post, [hp[0] + hp[2] * n, hp[1] + v.sum()], rtol=1e-7)
    ks(np.exp(d[:, 0] / hp[2]), stats.beta(post[0], post[1]))
    ks(np.exp(d[:, 1]), stats.beta(post[1], post[0]))


@pytest.mark.parametrize("n", MEMBERS)
def test_nich(host, n):
    v = _values("real", n).astype(np.float32).astype(np.float64)
    mean = float(v.mean()) if n else 0.0
    ctv = float(((v - mean) ** 2).sum()) if n else 0.0
    mu, kappa, sigmasq, nu = 0.3, 0.8, 1.7, 2.5
    post, d = post_and_draws(host, orc.NICH, 0, [mu, kappa, sigmasq, nu], [n], [mean, ctv], 3, 4)
    kn, nun = kappa + n, nu + n
    want = [(kappa * mu + n * mean) / kn, kn, (nu * sigmasq + ctv + n * kappa * (mu - mean) ** 2 / kn) / nun, nun]
    assert np.allclose(post, want, rtol=1e-5)
    mu_n, kappa_n, sigmasq_n, nu_n = post
    sig2 = -0.5 / d[:, 2]
    ks(sig2, stats.invgamma(nu_n / 2.0, scale=nu_n * sigmasq_n / 2.0))
    ks((d[:, 1] - mu_n) / np.sqrt(sig2 / kappa_n), stats.norm())
    assert np.allclose(d[:, 0], -0.5 * np.log(2.0 * math.pi * sig2), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("n", MEMBERS)
def test_dd(host, n):
    dim = 5
    v = _values("cat", n)
    counts = np.bincount(v, minlength=dim)
    hp = [0.4, 1.0, 2.5, 0.9, 1.3]
    post, d = post_and_draws(host, orc.DD, dim, hp, [n] + list(counts), [], dim, dim)
    assert np.allclose(post, np.asarray(hp, dtype=np.float32).astype(np.float64) + counts, rtol=1e-7)
    theta = np.exp(d)
    assert np.allclose(theta.sum(1), 1.0, atol=1e-5)
    for i in range(dim):
        ks(theta[:, i], stats.beta(post[i], post.sum() - post[i]))


def test_scipy_passes_the_same_gate_at_this_size():
    """the bar is one scipy's own sampler clears at this size and seed"""
    rng = np.random.default_rng(SEED)
    for dist in (stats.beta(1.5, 0.7), stats.gamma(2.0, scale=2.0), stats.invgamma(1.25, scale=2.1), stats.norm()):
        assert stats.kstest(dist.rvs(N, random_state=rng), dist.cdf).pvalue >= P_GATE


def _sticks(lib, cnt, alpha, seed, sweep):
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    lv, lw = np.zeros(len(cnt)), np.zeros(len(cnt))
    lib.blk_sticks(_p(cnt), len(cnt), alpha, seed, sweep, _p(lv), _p(lw))
    return lv, lw


@pytest.mark.parametrize("K", [1, 2, 32, 1000])
def test_stick_weights_sum_to_one(host, K):
    rng = np.random.default_rng(K)
    cnt = rng.integers(0, 50, K) * (rng.random(K) < 0.5)
    for sweep in range(5):
        lv, lw = _sticks(host, cnt, 1.3, SEED, sweep)
        assert np.isfinite(lw).all() and lv[-1] == 0.0
        assert abs(np.exp(lw).sum() - 1.0) <= 1e-6


def test_stick_fractions_follow_their_beta_posterior(host):
    """probability integral transform of V_k under Beta(1 + n_k, alpha + sum_{l > k} n_l), pooled over slots and sweeps"""
    K, alpha = 41, 0.7
    rng = np.random.default_rng(3)
    cnt = (rng.integers(0, 30, K) * (rng.random(K) < 0.6)).astype(np.uint32)
    after = np.concatenate([np.cumsum(cnt[::-1])[::-1][1:], [0]]).astype(np.float64)
    pit = []
    for sweep in range(250):
        lv, _ = _sticks(host, cnt, alpha, SEED, sweep)
        pit.append(stats.beta(1.0 + cnt[:-1], alpha + after[:-1]).cdf(np.exp(lv[:-1])))
    pit = np.concatenate(pit)
    assert pit.size == 250 * (K - 1)
    assert stats.kstest(pit, "uniform").pvalue >= P_GATE


def test_truncation_bound(host):
    assert host.blk_truncation_bound(6.0, 32, 1.0) == pytest.approx(4 * 6 * math.exp(-31.0), rel=1e-12)
    assert host.blk_truncation_bound(6.0, 32, 1.0) < 1e-11
    assert host.blk_truncation_bound(1e6, 256, 8.0) == pytest.approx(4e6 * math.exp(-255.0 / 8.0), rel=1e-12)


def test_header_and_binding_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        hdr = fh.read()
    for name in ("msc_blocked_draw", "msc_blocked_tables", "msc_blocked_assign", "msc_sweep_blocked"):
        assert re.search(r"int %s\(" % name, hdr)
        assert name in common_amd.EXPORTS
    for name in ("blocked_draw", "blocked_tables", "blocked_assign", "sweep_blocked"):
        assert hasattr(common_amd.State, name)
