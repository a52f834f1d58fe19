"""common_amd.diagnostics on the host: split_rhat and ess against a restatement with direct autocovariance sums (no FFT),
the degenerate inputs, and their values on inputs whose answer is known."""
import math

import numpy as np
import pytest

from common_amd import diagnostics as D


def _split_brute(x):
    x = np.asarray(x, dtype=np.float64)
    s = x.shape[1]
    n = s // 2
    return [list(row[:n]) for row in x] + [list(row[s - n:]) for row in x]


def _rhat_brute(x):
    seqs = _split_brute(x)
    m, n = len(seqs), len(seqs[0])
    means = [sum(q) / n for q in seqs]
    var = [sum((v - mu) ** 2 for v in q) / (n - 1) for q, mu in zip(seqs, means)]
    w = sum(var) / m
    grand = sum(means) / m
    b_over_n = sum((mu - grand) ** 2 for mu in means) / (m - 1)
    return math.sqrt(((n - 1) / n * w + b_over_n) / w)


def _ess_brute(x):
    """the docstring of common_amd.diagnostics, with every autocovariance a direct sum"""
    seqs = _split_brute(x)
    m, n = len(seqs), len(seqs[0])
    means = [sum(q) / n for q in seqs]

    def acov(t):                                     # the mean over the sequences of the lag-t autocovariance
        tot = 0.0
        for q, mu in zip(seqs, means):
            tot += sum((q[i] - mu) * (q[i + t] - mu) for i in range(n - t)) / n
        return tot / m

    w = acov(0) * n / (n - 1)
    grand = sum(means) / m
    var_plus = w * (n - 1) / n + sum((mu - grand) ** 2 for mu in means) / (m - 1)

    def rho(t):
        return 1.0 - (w - acov(t)) / var_plus if t < n else 0.0

    kept = {0: 1.0, 1: rho(1)}
    even, odd = kept[0], kept[1]
    t = 1
    while t < n - 4 and even + odd > 0.0:
        even, odd = rho(t + 1), rho(t + 2)
        if even + odd >= 0.0:
            kept[t + 1], kept[t + 2] = even, odd
        t += 2
    max_t = t
    if even > 0.0:
        kept[max_t + 1] = even
    t = 1
    while t <= max_t - 3:
        if kept.get(t + 1, 0.0) + kept.get(t + 2, 0.0) > kept.get(t - 1, 0.0) + kept.get(t, 0.0):
            kept[t + 1] = 0.5 * (kept.get(t - 1, 0.0) + kept.get(t, 0.0))
            kept[t + 2] = kept[t + 1]
        t += 2
    tau = -1.0 + 2.0 * sum(kept.get(i, 0.0) for i in range(max_t)) + kept.get(max_t + 1, 0.0)
    tau = max(tau, 1.0 / math.log10(m * n))
    return m * n / tau


def _ar1(rng, chains, draws, phi):
    e = rng.standard_normal((chains, draws))
    x = np.zeros((chains, draws))
    for t in range(1, draws):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x


@pytest.mark.parametrize("chains,draws", [(1, 4), (1, 5), (2, 9), (3, 40), (4, 41), (5, 100), (2, 257)])
def test_against_the_brute_force_restatement(chains, draws):
    rng = np.random.default_rng(100 * chains + draws)
    for kind in range(3):
        x = rng.standard_normal((chains, draws)) if kind == 0 else _ar1(rng, chains, draws, 0.8 if kind == 1 else -0.6)
        x = 3.0 + 2.0 * x + (np.arange(chains)[:, None] * 0.3 if kind == 2 else 0.0)
        for got, want in ((D.split_rhat(x), _rhat_brute(x)), (D.ess(x), _ess_brute(x))):
            assert math.isfinite(want) and abs(got - want) <= 1e-9 * abs(want), (kind, got, want)


def test_autocovariance_is_the_direct_sum():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 65):
        y = rng.standard_normal((3, n))
        got = D.autocovariance(y)
        for j in range(3):
            mu = y[j].mean()
            want = [np.sum((y[j, :n - t] - mu) * (y[j, t:] - mu)) / n for t in range(n)]
            assert np.allclose(got[j], want, rtol=0, atol=1e-12)


def test_degenerate_inputs_give_nan():
    rng = np.random.default_rng(1)
    for x in (rng.standard_normal((4, 3)), rng.standard_normal((4, 0)), np.ones((3, 10)),
              np.tile(np.arange(3.0)[:, None], (1, 8))):                 # too short; no variance inside a chain
        assert math.isnan(D.split_rhat(x)) and math.isnan(D.ess(x))
    bad = rng.standard_normal((2, 10))
    bad[1, 4] = np.nan
    assert math.isnan(D.split_rhat(bad)) and math.isnan(D.ess(bad))
    bad[1, 4] = np.inf
    assert math.isnan(D.split_rhat(bad)) and math.isnan(D.ess(bad))
    assert math.isfinite(D.split_rhat(rng.standard_normal((1, 4)))) and math.isfinite(D.ess(rng.standard_normal((1, 4))))
    for wrong in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 10))):
        with pytest.raises(ValueError):
            D.split_rhat(wrong)
        with pytest.raises(ValueError):
            D.ess(wrong)


def test_known_answers():
    x = np.random.default_rng(0).standard_normal((8, 2000))
    assert 0.99 <= D.split_rhat(x) <= 1.01                               # 1.00003
    assert 0.8 <= D.ess(x) / 16000 <= 1.2                                # 0.976
    ar = _ar1(np.random.default_rng(0), 8, 2000, 0.9)
    assert 0.03 <= D.ess(ar) / 16000 <= 0.09                             # 0.046; theory (1 - phi) / (1 + phi) = 0.0526
    assert D.split_rhat(x + np.arange(8)[:, None]) > 2.0                 # 2.58
