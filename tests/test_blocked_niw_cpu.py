"""The blocked Gibbs sampler's niw feature, host side: common_amd/csrc/blocked_niw.hpp built with the host compiler -- the
posterior against a numpy restatement and 10^4 draws of (mean, whiten, c) against the Normal-Inverse-Wishart posterior
and scipy's own inverse-Wishart sampler -- and the new entry point in the header and the binding.  No device needed."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import common_amd
from oracle import oracle as orc
from tests import blocked_niw_helpers as bh
from tests.gpu_helpers import distinct_hp

ROOT = bh.ROOT
N = 10000
P_GATE = bh.P_GATE
DIMS = [2, 3, 17]
MEMBERS = [0, 1, 500]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bh.build_host(tmp_path_factory.mktemp("blocked_niw"))


def _slot(d, n):
    hpb = bh.hp_block(distinct_hp(orc.NIW, d), d)
    assert np.array_equal(hpb, common_amd.pack_hp(orc.NIW, distinct_hp(orc.NIW, d), d))
    _, sx, sxx = bh.members(d, n)
    return hpb, sx, sxx


@pytest.mark.parametrize("n", MEMBERS)
@pytest.mark.parametrize("d", DIMS)
def test_posterior(host, d, n):
    hpb, sx, sxx = _slot(d, n)
    kn, nun, mun, Psin = bh.host_post(host, hpb, d, n, sx, sxx)
    wkn, wnun, wmun, wPsin = bh.posterior(hpb, d, n, sx, sxx)
    assert np.allclose([kn, nun], [wkn, wnun], rtol=1e-7)
    assert np.allclose(mun, wmun, rtol=1e-7)
    assert np.allclose(Psin, wPsin, rtol=1e-7)
    assert np.array_equal(Psin, Psin.T) and np.all(np.linalg.eigvalsh(Psin) > 0)
    hp = distinct_hp(orc.NIW, d)
    assert kn == hp["kappa"] + n and nun == hp["nu"] + n and kn != nun      # (non-unit, distinct kappa and nu)


@pytest.mark.parametrize("n", MEMBERS)
@pytest.mark.parametrize("d", DIMS)
def test_draws_follow_the_posterior(host, d, n):
    hpb, sx, sxx = _slot(d, n)
    kn, nun, mun, Psin = bh.posterior(hpb, d, n, sx, sxx)
    mean, whiten, vmu, c = bh.host_draws(host, hpb, d, n, sx, sxx, N)
    bh.check_draws(mean, whiten, c, d, kn, nun, mun, Psin)
    # V mu as the assign kernel's operand holds it
    V = bh.unpack(whiten, d)
    assert np.allclose(vmu, np.einsum("nij,nj->ni", V, mean), rtol=1e-9, atol=1e-9)
    # another draw of the same slot is another matrix; the same one repeats its bits
    again = bh.host_draws(host, hpb, d, n, sx, sxx, 4)
    assert np.array_equal(again[1], whiten[:4]) and np.array_equal(again[0], mean[:4])
    other = bh.host_draws(host, hpb, d, n, sx, sxx, 4, sweep=1)
    assert not np.array_equal(other[1], whiten[:4])
    assert len(np.unique(whiten[:, 0])) == N


def test_the_usual_bartlett_order_is_told_apart():
    """the check at both ends of the diagonal rejects a triangular factor whose degrees of freedom DEcrease down the
    diagonal (numpy draws, the posterior of d = 3 with 500 members)"""
    d, n = 3, 500
    hpb = bh.hp_block(distinct_hp(orc.NIW, d), d)
    _, sx, sxx = bh.members(d, n)
    kn, nun, mun, Psin = bh.posterior(hpb, d, n, sx, sxx)
    rng = np.random.default_rng(bh.SEED)
    Li = np.linalg.inv(np.linalg.cholesky(Psin))
    T = np.tril(rng.standard_normal((N, d, d)), -1)
    for i in range(d):
        T[:, i, i] = np.sqrt(rng.chisquare(nun - i, N))
    Vinv = np.linalg.inv(T @ Li)
    Sigma = Vinv @ np.transpose(Vinv, (0, 2, 1))
    p = [stats.kstest(Psin[i, i] / Sigma[:, i, i], stats.chi2(nun - d + 1).cdf).pvalue for i in (0, d - 1)]
    assert min(p) < 1e-6, p


def test_scipy_passes_the_same_gate_at_this_size():
    """the bar is one scipy's own samplers clear at this size and seed"""
    d, n = 3, 500
    hpb = bh.hp_block(distinct_hp(orc.NIW, d), d)
    _, sx, sxx = bh.members(d, n)
    kn, nun, mun, Psin = bh.posterior(hpb, d, n, sx, sxx)
    rng = np.random.default_rng(bh.SEED + 1)
    Sigma = np.asarray(stats.invwishart(df=nun, scale=Psin).rvs(N, random_state=rng))
    a = bh.fixed_vector(d)
    prec = np.linalg.inv(Sigma)
    assert stats.kstest(np.einsum("i,nij,j->n", a, prec, a) / (a @ np.linalg.inv(Psin) @ a), stats.chi2(nun).cdf).pvalue >= P_GATE
    for i in (0, d - 1):
        assert stats.kstest(Psin[i, i] / Sigma[:, i, i], stats.chi2(nun - d + 1).cdf).pvalue >= P_GATE
    ref = bh.reference_sigmas(nun, Psin, N)
    for x, y in zip(bh.sigma_stats(Sigma), bh.sigma_stats(ref)):
        assert stats.ks_2samp(x, y).pvalue >= P_GATE
    assert stats.kstest(stats.norm().rvs(N * d, random_state=rng), stats.norm().cdf).pvalue >= P_GATE


def test_header_and_binding_declare_the_entry_point(host):
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        hdr = fh.read()
    assert re.search(r"int msc_blocked_niw_params\(", hdr)
    assert "msc_blocked_niw_params" in common_amd.EXPORTS
    assert hasattr(common_amd.State, "blocked_niw_params")
    assert "the blocked sweep takes a niw feature of dimension at most 32" in hdr
    assert host.niw_max_dim() == 32
