"""The sequential Gibbs sweep without a GPU: the ABI declares and exports it, and the yardsticks its GPU tests use (the
exact posterior over set partitions, the double replay of the chain) are right."""
import ctypes as C
import math
import os
import re

import numpy as np

from oracle import oracle as orc
from tests import seq_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = ("int msc_sweep_sequential(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, "
       "uint64_t nrows, uint64_t row_id0, int32_t *z_dev, const uint32_t *order_dev, uint32_t nsweeps, uint64_t seed, "
       "uint64_t sweep, int32_t *trace_dev);")


def test_header_declares_and_library_exports_sweep_sequential():
    text = open(os.path.join(ROOT, "include", "microscopes_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert SIG in flat
    import common_amd
    lib = C.CDLL(common_amd.LIB_PATH)
    assert hasattr(lib, "msc_sweep_sequential")
    assert "msc_sweep_sequential" in common_amd.EXPORTS


def test_enumerator_covers_bell_numbers_and_normalises():
    for n, bell in [(1, 1), (2, 2), (3, 5), (4, 15), (5, 52), (6, 203)]:
        parts = sh.set_partitions(n)
        assert len(parts) == bell and len(set(parts)) == bell
        assert all(sh.canonical(a) == a for a in parts)
    F = orc.Family(orc.BB, dict(alpha=1.0, beta=1.0))
    vals = np.array([True, False, True, True], dtype=np.bool_)
    parts, p = sh.exact_posterior([(F, vals)], 1.3)
    assert len(parts) == 15 and abs(p.sum() - 1.0) < 1e-12 and (p > 0).all()


def test_two_rows_closed_form():
    # two identical bool rows over D uniform-hp bb columns: together, the block's marginal likelihood is 1/3 a column;
    # apart, (1/2)^2.  With alpha = 1: P(together) = (1/2) (1/3)^D / ((1/2) (1/3)^D + (1/2) (1/4)^D)
    D, alpha = 16, 1.0
    F = orc.Family(orc.BB, dict(alpha=1.0, beta=1.0))
    feats = [(F, np.array([True, True], dtype=np.bool_)) for _ in range(D)]
    parts, p = sh.exact_posterior(feats, alpha)
    apart = p[parts.index((0, 1))]
    assert abs(apart - 1.0 / (1.0 + (4.0 / 3.0) ** D)) < 1e-12
    # and with the CRP weights of alpha != 1 (together alpha / (1 + alpha) * 1/alpha ... : 1 : alpha)
    parts, p = sh.exact_posterior([(F, np.array([True, False], dtype=np.bool_))], 2.5)
    w_tog, w_apart = 1.0 / (1 + 2.5) * (1.0 / 6.0), 2.5 / (1 + 2.5) * 0.25
    assert abs(p[parts.index((0, 1))] - w_apart / (w_tog + w_apart)) < 1e-12


def test_replay_as_a_sampler_reaches_the_exact_posterior():
    """The replay, drawing for itself with the device's counters, is the collapsed Gibbs sampler: N = 4, K = 5,
    2e4 sweeps, TV to the exact posterior over the 15 partitions <= 0.04."""
    rng = np.random.default_rng(3)
    N, K, alpha, nsweeps = 4, 5, 1.1, 20000
    F1 = orc.Family(orc.BB, dict(alpha=1.0, beta=1.0))
    F2 = orc.Family(orc.NICH, dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0))
    v1 = np.array([True, True, False, True], dtype=np.bool_)
    v2 = np.array([0.1, -0.3, 2.5, 0.4], dtype=np.float32)
    parts, p = sh.exact_posterior([(F1, v1), (F2, v2)], alpha)
    rp = sh.Replay([(F1, v1), (F2, v2)], K, alpha, np.full(N, -1, np.int32))
    traces = np.empty((nsweeps, N), np.int32)
    rows = np.arange(N)
    for s in range(nsweeps):
        order = rng.permutation(N) if s % 2 else rows
        rp.sweep(order, 7, s, order)
        traces[s] = rp.z
    freq = sh.partition_frequencies(traces[100:], parts)
    tv, kl = sh.tv_kl(freq, p)
    assert tv <= 0.04, (tv, kl)
    # the replay's tables stay the oracle's accumulate of its assignment
    ss, cnt = rp.tables()
    assert np.array_equal(cnt, np.bincount(rp.z, minlength=K))
    want = F1.accumulate(K, v1, rp.z)
    assert np.array_equal(ss[0]["heads"], want["heads"]) and np.array_equal(ss[0]["tails"], want["tails"])
    assert math.isfinite(kl)
