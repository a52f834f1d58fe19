"""Scores at production-sized groups against the 60-digit fixture (tests/golden/heavy.json; tests/heavy_cases.py for the
rungs and values): one group holding most of 1e7 - 1e8 rows next to singletons and empty slots.  The oracle's double
twin is no arbiter there (tests/test_heavy_cpu.py measures where it ends), so every expectation below is the fixture's.

Statistics go in through set_ss / set_group_counts, no rows are accumulated.  Two layouts: K = one group per rung, and
K = 300 with group k on rung k mod (number of rungs) -- past the tile kernels' 256 with a tail of 44.  512 rows, row i
holding value i mod (number of values).  Gate: the project's TOL on rel_err, every check through audit().

What these tests caught (MI355X, the library before family_math.hpp took differences of lgamma term by term from 2^20
on): score_value of gp off by 7.6e-6 at 1e8 rows (both layouts), dm's leave-one-out tables by 1.06e-6, and with them
predictive_logp; bnb (8.1e-7), dm plain (6.9e-7) and the mixed state (6.4e-7) inside the gate by little.  After: gp
5.2e-8, dm 4.9e-8, bnb 5.5e-8, mixed 1.9e-7; nich 1.6e-7 before and after (its float evaluation).

The last test is the exact one of lopsided accumulation: 2^22 rows, all but 70 in one group.

This file holds the batched routes.  tests/test_gpu_heavy_chains.py holds the routes built since to the same fixture, with
install() and Heavy from here (the expectations themselves are hc.Expect, host side): the ensemble's row predictive, one
visit of the sequential sweep per chain -- untempered, tempered and through the single-chain call -- the tables a visit
leaves, and the log joint of a state and of an ensemble, whose CRP term is the fixture's score_assignment.  It caught no
wrong constant: every score is within 1.7e-7 and every joint entry within 4e-15.  What it measured is where the additive
tables end: on the lopsided rungs the double sum of squares is 1e10 times count_times_variance, and a visit leaves that
field off by up to 1.67e-6 whatever the commit does (held there to the sum's representation bound, derived in the test).
Split-merge acceptance and the blocked sampler's parameter draws at heavy groups are held by neither file: their states
need real rows in the heavy group, or statistical gates."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import common_amd
from oracle import oracle as orc
from tests import heavy_cases as hc
from tests.gpu_helpers import TOL, audit, rel_err

pytestmark = pytest.mark.gpu
N = 512
ALPHA = 1.3
fixture = hc.fixture


def install(st, names, rung, counts):
    """the heavy tables into any State of the named families' features -- a ChainEnsemble's ens.states[c] as well:
    hyperparameters, the rungs' statistics of every feature, the group counts and alpha"""
    for i, n in enumerate(names):
        fam, dim = hc.FAMILIES[n]
        st.set_hp(i, hc.hp_of(n))
        src = hc.rungs(n)[rung]
        ss = np.zeros(len(rung), dtype=common_amd.ss_dtype(fam, dim))
        for f in ss.dtype.names:
            ss[f] = src[f]
        st.set_ss(i, ss)
    st.set_group_counts(counts.astype(np.uint32))
    st.set_alpha(ALPHA)


class Heavy(hc.Expect):
    """a state of the named families on the heavy rungs, and the fixture's expectations for it (hc.Expect: host side)"""

    def __init__(self, ctx, names, K=None, n=N, vmax=None):
        hc.Expect.__init__(self, names, K, n, vmax)
        self.ctx = ctx
        assert (self.z >= 0).mean() > 0.5 and len(self.rungs_left) >= self.R // 2
        self.rec = self.records()
        self.view = common_amd.DataView.from_recarray(ctx, self.rec)
        self.st = common_amd.State(ctx, [hc.FAMILIES[n] for n in names], self.K)
        self.install(self.st)
        self.zt = torch.from_numpy(self.z).to(ctx.torch_device)

    def install(self, st):
        install(st, self.names, self.rung, self.counts)

    def totals(self, loo=False):
        return hc.Expect.totals(self, loo, ALPHA)


def check(name, got, want):
    """no NaN / inf but the fixture's own -inf, and the TOL gate on the rest"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), name
    assert np.all(np.isfinite(got[~inf])), name
    e = rel_err(got[~inf], want[~inf])
    print("%s: worst rel_err %.3g" % (name, e.max()))
    audit("heavy." + name, e.max(), TOL)


SINGLES = [[n] for n in hc.FAMILIES]
CASES = SINGLES + [hc.MIXED]
LAYOUTS = [None, 300]
_id = lambda names: "mixed" if len(names) > 1 else names[0]


@pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])
@pytest.mark.parametrize("names", CASES, ids=_id)
def test_score_value_on_heavy_groups(gpu_ctx, names, K):
    h = Heavy(gpu_ctx, names, K)
    tag = "%s.K%d" % (_id(names), h.K)
    got = h.st.score_value(h.view).cpu().numpy()
    kernel = gpu_ctx.last_kernel("score")
    if len(names) > 1 and K == 300:
        assert kernel.startswith("k_score_tile<"), kernel
    if names == ["nich"] and K == 300:      # (one group per rung is a narrow state: the route sends it to the tile kernels)
        assert kernel.startswith("k_score_nich1"), kernel
    check("score_value." + tag, got, h.expected())
    got = h.st.score_value(h.view, z=h.zt).cpu().numpy()
    check("score_value_loo." + tag, got, h.expected(loo=True))


@pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])
@pytest.mark.parametrize("names", CASES, ids=_id)
def test_score_data_on_heavy_groups(gpu_ctx, names, K):
    h = Heavy(gpu_ctx, names, K)
    check("score_data.%s.K%d" % (_id(names), h.K), h.st.score_data().cpu().numpy(), h.data)


@pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])
@pytest.mark.parametrize("loo", [False, True], ids=["plain", "loo"])
def test_predictive_logp_on_heavy_groups(gpu_ctx, K, loo):
    h = Heavy(gpu_ctx, hc.MIXED, K)
    logp, mp, _ = h.st.predictive_logp(h.view, z=h.zt if loo else None, want_map=True)
    t, want = h.totals(loo)
    check("predictive_logp.%s.K%d" % ("loo" if loo else "plain", h.K), logp.cpu().numpy(), want)
    # the MAP group: the expected one, except where the two largest expected totals lie within 1e-5 (rungs repeat over the
    # groups of K = 300 and the two empty rungs are one group twice, so ties are the rule there): then one of that band
    mp = mp.cpu().numpy()
    top2 = np.sort(t, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-5
    assert np.array_equal(mp[clear], t.argmax(axis=1)[clear])
    assert np.all(t[np.arange(N), mp] >= top2[:, 1] - 1e-5 - 2 * TOL * np.abs(top2[:, 1]))


def _sweep_check(h, seed, sweep_idx):
    from tests.test_gpu_sweep import _check_agreement
    zt = h.zt.clone()
    h.st.sweep_assign(h.view, zt, seed=seed, sweep=sweep_idx)
    got = zt.cpu().numpy()
    assert np.all((got >= 0) & (got < h.K))
    t, _ = h.totals(loo=True)
    want = np.empty(N, dtype=np.int64)
    for n in range(N):
        cdf = np.cumsum(orc.scores_to_probs(t[n]))
        want[n] = min(int(np.searchsorted(cdf, orc.uniform01(seed, sweep_idx, n), side="right")), h.K - 1)
    print("sweep agreement %.4f" % (got == want).mean())
    _check_agreement(got, want, t, seed, sweep_idx, 0.98)


@pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])
@pytest.mark.parametrize("mode", ["rowwise", "transposed"])
def test_sweep_of_a_heavy_single_nich_state(gpu_ctx, K, mode, monkeypatch):
    monkeypatch.setenv("MSC_SWEEP_NICH1", {"rowwise": "1", "transposed": "2"}[mode])
    _sweep_check(Heavy(gpu_ctx, ["nich"], K), 41, 2)


@pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])
def test_sweep_of_a_heavy_mixed_state(gpu_ctx, K):
    _sweep_check(Heavy(gpu_ctx, hc.MIXED, K), 43, 1)


@pytest.mark.parametrize("name", ["gp", "bnb", "dm", "nich", "niw3"])
def test_per_value_route_on_the_largest_rungs(gpu_ctx, name):
    """the per-value mailbox (Context.value_op) evaluates the same differences in its own kernel: the four largest
    rungs, every value"""
    fx = fixture()
    fam, dim = hc.FAMILIES[name]
    src = hc.rungs(name)
    got, want = [], []
    for r in range(len(src) - 4, len(src)):
        rec = np.zeros(1, dtype=common_amd.ss_dtype(fam, dim))
        for f in rec.dtype.names:
            rec[f] = src[r][f]
        for j, v in enumerate(hc.values(name)):
            got.append(gpu_ctx.value_op(fam, dim, "score_value", hc.hp_of(name), rec, np.asarray(v)))
            want.append(fx[name]["score_value"][r, j])
    check("value_op." + name, got, want)


# ---- lopsided accumulation, exact ------------------------------------------------------------------------------------

def _exact_stats(cols, z, K, lo, hi):
    """integer statistics of rows [lo, hi) with numpy's integer arithmetic; the nich moments as exact rationals from
    xi = 64 x (an integer below 2^15: sum xi < 2^37, sum xi^2 < 2^52)"""
    sl = slice(lo, hi)
    zz = z[sl]
    on = zz >= 0
    g = zz[on]
    cnt = np.bincount(g, minlength=K)

    def isum(a):                                       # per group, in int64: group 0 by subtraction of the few other rows
        a = a[sl][on].astype(np.int64)
        out = np.zeros(K, dtype=np.int64)
        rest = g != 0
        np.add.at(out, g[rest], a[rest])
        out[0] = a.sum() - out.sum()
        return out
    xi = np.rint(cols["nich"].astype(np.float64) * 64.0).astype(np.int64)
    assert np.array_equal(xi / 64.0, cols["nich"].astype(np.float64))
    sx, sxx = isum(xi), isum(xi * xi)
    out = dict(count=cnt, gp_sum=isum(cols["gp"]), bnb_sum=isum(cols["bnb"]), heads=isum(cols["bb"]),
               dd=np.stack([isum(cols["dd"] == c) for c in range(7)], axis=1), mean=[], ctv=[])
    for k in range(K):
        n = int(cnt[k])
        out["mean"].append(Fraction(int(sx[k]), 64 * n) if n else None)
        out["ctv"].append(Fraction(int(sxx[k]) * n - int(sx[k]) ** 2, 4096 * n) if n else None)
    return out


def _check_accumulated(st, want, tag):
    K = len(want["count"])
    nich, gp, bnb, dd, bb = (st.get_ss(i) for i in range(5))
    assert np.array_equal(nich["count"], want["count"]) and np.array_equal(gp["count"], want["count"])
    assert np.array_equal(bnb["count"], want["count"]) and np.array_equal(dd["count_sum"], want["count"])
    assert np.array_equal(gp["sum"], want["gp_sum"]) and np.array_equal(bnb["sum"], want["bnb_sum"])
    assert np.array_equal(dd["counts"], want["dd"])
    assert np.array_equal(bb["heads"], want["heads"]) and np.array_equal(bb["tails"], want["count"] - want["heads"])
    worst_ulp, worst_ctv = 0.0, 0.0
    for k in range(K):
        if want["mean"][k] is None:
            assert np.isfinite(nich["mean"][k]) and np.isfinite(nich["count_times_variance"][k])
            continue
        m, c = want["mean"][k], want["ctv"][k]
        ulp = float(np.spacing(np.abs(np.float32(float(m)))))
        worst_ulp = max(worst_ulp, abs(float(Fraction(float(nich["mean"][k])) - m)) / ulp)
        # relative; a singleton's exact 0 is held to 1e-6 absolute (a difference of x^2 ~ 1e4 in double: 1e-12)
        worst_ctv = max(worst_ctv, abs(float(Fraction(float(nich["count_times_variance"][k])) - c)) / max(float(c), 1.0 if c == 0 else 0.0))
    print("%s: mean off by %.3f ulp, ctv by %.3g relative" % (tag, worst_ulp, worst_ctv))
    audit("heavy.accumulate_mean_ulp." + tag, worst_ulp, 1.0)
    audit("heavy.accumulate_ctv." + tag, worst_ctv, TOL)


def test_lopsided_accumulation_is_exact(gpu_ctx):
    """2^22 rows, all but 70 of them in group 0, one each in groups 1 .. 64, five groups empty, six rows unassigned: the
    LDS histogram of k_accumulate with every lane on one address"""
    n, K = 1 << 22, 70
    rng = np.random.default_rng(22)
    cols = dict(nich=(100.0 + rng.integers(-156 * 64, 156 * 64 + 1, n) / 64.0).astype(np.float32),
                gp=rng.integers(0, 50, n).astype(np.uint32), bnb=rng.integers(0, 9, n).astype(np.uint32),
                dd=np.minimum(rng.integers(0, 40, n), 6).astype(np.int32), bb=rng.random(n) < 0.03)
    assert cols["nich"].min() >= -256 and cols["nich"].max() <= 256
    z = np.zeros(n, dtype=np.int32)
    apart = rng.choice(n, 70, replace=False)
    z[apart[:64]] = np.arange(1, 65)
    z[apart[64:]] = -1
    rec = np.zeros(n, dtype=[("f0", np.float32), ("f1", np.uint32), ("f2", np.uint32), ("f3", np.int32), ("f4", np.bool_)])
    for i, c in enumerate(("nich", "gp", "bnb", "dd", "bb")):
        rec["f%d" % i] = cols[c]
    view = common_amd.DataView.from_recarray(gpu_ctx, rec)
    st = common_amd.State(gpu_ctx, [(orc.NICH, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 7), (orc.BB, 0)], K)
    for i, name in enumerate(("nich", "gp", "bnb", "dd", "bb")):
        st.set_hp(i, hc.hp_of(name))
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    st.accumulate(view, zt)
    _check_accumulated(st, _exact_stats(cols, z, K, 0, n), "all")
    st.accumulate(view, zt[:n // 2].contiguous(), row0=0, nrows=n // 2, reset=False, subtract=True)
    _check_accumulated(st, _exact_stats(cols, z, K, n // 2, n), "second_half")
