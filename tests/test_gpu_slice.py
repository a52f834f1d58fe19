"""Slice sampling on the device (msc_hp_slice / msc_theta_slice, State.hp_slice / theta_slice, hypers.FeatureHpSlice):
every device update replayed by the host twin (tests/slice_helpers.py) from the device's pre-step values, stationarity of
the device chains against posteriors taken from msc_hp_grid_score and the Beta law, installation against set_hp /
set_alpha / set_ss through scoring and sweeps, determinism, and the argument checks."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import slice_helpers as sh
from tests.gpu_helpers import audit, make_feature, recarray_of
from tests.test_gpu_hp_grid import _records, _ss64

pytestmark = pytest.mark.gpu

EXP, NORMAL, BETA = sh.PRIOR_EXPONENTIAL, sh.PRIOR_NORMAL, sh.PRIOR_NONINF_BETA
# per family: its hp, and the entries (coord, prior, a, b, partner, width) of a step
SPECS = [
    (orc.BB, [2.0, 1.5], [(0, BETA, 0, 0, 1, 1.0), (1, BETA, 0, 0, 0, 1.0)]),
    (orc.BBNC, [1.5, 3.0], [(1, BETA, 0, 0, 0, 0.5), (0, BETA, 0, 0, 1, 2.0)]),
    (orc.BNB, [1.5, 2.0, 3.0], [(0, BETA, 0, 0, 1, 1.0), (1, BETA, 0, 0, 0, 1.0)]),
    (orc.GP, [3.0, 0.5], [(0, EXP, 1.0, 0, 0, 1.0), (1, EXP, 0.5, 0, 0, 0.25)]),
    (orc.NICH, [0.25, 2.0, 1.5, 3.0], [(0, NORMAL, 0.0, 1.0, 0, 1.0), (1, EXP, 1.0, 0, 0, 1.0), (2, EXP, 1.0, 0, 0, 1.0),
                                       (3, EXP, 0.5, 0, 0, 3.0)]),
]
ALPHA_ENTRY = (EXP, 1.0, 0, 2.0)        # prior, a, b, width


def _coord(f, c):
    coord, prior, a, b, partner, w = c
    return {"feature": f, "coord": coord, "width": w, "prior": prior, "a": a, "b": b, "partner": partner}


def _mixed_state(gpu_ctx, K, seed):
    import common_amd
    rng = np.random.default_rng(seed)
    st = common_amd.State(gpu_ctx, [(F, 0) for F, _, _ in SPECS], K)
    empty = rng.random(K) < 0.3
    empty[0] = True                      # (bbnc: p = 7 sits in slot 0, which is never counted)
    empty[-1] = False
    recs, n = [], None
    for f, (F, hp, _) in enumerate(SPECS):
        rec, n = _records(F, 0, K, rng, empty)
        st.set_ss(f, rec)
        st.set_hp(f, np.array(hp, np.float32))
        recs.append(rec)
    st.set_group_counts(n)
    st.set_alpha(1.3)
    coords = [_coord(f, c) for f, (_, _, cs) in enumerate(SPECS) for c in cs]
    coords.append({"feature": "alpha", "coord": 0, "width": ALPHA_ENTRY[3], "prior": ALPHA_ENTRY[0],
                   "a": ALPHA_ENTRY[1], "b": ALPHA_ENTRY[2]})
    return st, recs, n, coords


def _replay(st, recs, counts, coords, pre_hp, pre_alpha, values, evals, seed, sweep, tally):
    """replay every entry of one device step with the twin, each from the device's values before it"""
    nfeat = len(SPECS)
    counted = counts > 0
    entry_of = {}
    cur = {f: [float(v) for v in pre_hp[f]] for f in range(nfeat)}
    alpha = pre_alpha
    for i, c in enumerate(coords):
        f = c["feature"]
        e = entry_of.get(f, 0)
        entry_of[f] = e + 1
        if f == "alpha":
            g = sh.alpha_target(counts, c["prior"], c["a"], c["b"])
            x, ev, status, cmps = sh.slice_update(g, sh.support(True), alpha, c["width"],
                                                  sh.hp_uniforms(seed, nfeat, e, sweep))
            alpha = float(values[i])
        else:
            F = SPECS[f][0]
            k = c["coord"]
            g = sh.feature_target(F, 0, cur[f], k, _ss64(F, 0, recs[f]), counted, c["prior"], c["a"], c["b"],
                                  cur[f][c["partner"]])
            x, ev, status, cmps = sh.slice_update(g, sh.support(sh.positive_support(F, k)), cur[f][k], c["width"],
                                                  sh.hp_uniforms(seed, f, e, sweep))
            cur[f][k] = float(values[i])
        assert status != sh.NON_FINITE
        tally["n"] += 1
        if x == float(values[i]):
            tally["exact"] += 1
            assert ev == int(evals[i]), (i, ev, int(evals[i]))
        else:
            # the device's double sum runs in another order than the oracle's: a comparison this close may go either way
            audit("slice.replay_deciding_comparison", sh.deciding_margin(cmps), 1e-9)
    return cur, alpha


@pytest.mark.parametrize("K", [7, 256, 1000])
def test_hp_steps_replay_against_the_twin(gpu_ctx, K):
    st, recs, n, coords = _mixed_state(gpu_ctx, K, 100 + K)
    tally = {"n": 0, "exact": 0}
    alpha = 1.3
    for sweep in range(4):
        pre = [st.get_hp(f).copy() for f in range(len(SPECS))]
        values, evals = st.hp_slice(coords, seed=77, sweep=sweep)
        assert np.all(evals >= 1)
        cur, _ = _replay(st, recs, n, coords, pre, alpha, values, evals, 77, sweep, tally)
        for f in range(len(SPECS)):                  # the chain of a feature ends in the block the state now holds
            assert np.array_equal(st.get_hp(f), np.array(cur[f], np.float32))
        alpha = float(values[-1])
    assert tally["exact"] >= 0.99 * tally["n"], tally
    # a caller's mask: empty slots counted (bbnc's slot 0 with p = 7 excluded), some occupied ones not
    rng = np.random.default_rng(K)
    mask = rng.random(K) < 0.6
    mask[0] = False
    mdev = torch.from_numpy(mask.astype(np.uint8)).to(gpu_ctx.torch_device)
    feat_coords = coords[:-1]
    pre = [st.get_hp(f).copy() for f in range(len(SPECS))]
    values, evals = st.hp_slice(feat_coords, seed=5, sweep=9, slots=mdev)
    tally = {"n": 0, "exact": 0}
    _replay(st, recs, mask.astype(np.uint32), feat_coords, pre, alpha, values, evals, 5, 9, tally)
    assert tally["exact"] >= 0.99 * tally["n"], tally
    st.close()


@pytest.mark.parametrize("K", [7, 256, 1000])
def test_theta_steps_replay_against_the_twin(gpu_ctx, K):
    import common_amd
    rng = np.random.default_rng(5 + K)
    st = common_amd.State(gpu_ctx, [(orc.BB, 0), (orc.BBNC, 0), (orc.BBNC, 0)], K)
    empty = rng.random(K) < 0.3
    empty[0] = True
    empty[-1] = False
    recs = {}
    n = None
    for f, hp in ((1, [1.5, 2.5]), (2, [0.7, 0.9])):
        rec, n = _records(orc.BBNC, 0, K, rng, empty)          # slot 0: p = 7, not counted: never read
        st.set_ss(f, rec)
        st.set_hp(f, np.array(hp, np.float32))
        recs[f] = rec
    st.set_group_counts(n)
    exact = total = 0
    for sweep in range(3):
        pre = {f: st.get_ss(f) for f in recs}
        evals = st.theta_slice({2: {"p": 0.1}, 1: {"p": 0.3}}, seed=13, sweep=sweep)
        for f, w in ((1, 0.3), (2, 0.1)):
            post = st.get_ss(f)
            hp = st.get_hp(f)
            assert post["p"][0] == np.float32(7.0)           # not counted: not touched
            assert np.array_equal(post["p"][empty], pre[f]["p"][empty])
            ev_sum = 0
            for k in np.flatnonzero(~empty):
                g = sh.theta_target(hp, int(pre[f]["heads"][k]), int(pre[f]["tails"][k]))
                x, ev, status, cmps = sh.slice_update(g, sh.theta_support, float(pre[f]["p"][k]), w,
                                                      sh.theta_uniforms(13, int(k), f, sweep))
                assert status == sh.OK
                total += 1
                ev_sum += ev
                if x == float(post["p"][k]):
                    exact += 1
                else:
                    audit("slice.theta_replay_deciding_comparison", sh.deciding_margin(cmps), 1e-9)
            if exact == total:
                assert evals[f] == ev_sum, (f, evals[f], ev_sum)
    assert exact >= 0.99 * total, (exact, total)
    st.close()


def _posterior_cdf(score_fn, lo, hi, logprior):
    """CDF of exp(score + logprior) on [lo, hi] from 10^4 grid points (trapezoid), as a callable"""
    xs = np.linspace(lo, hi, 10000)
    s = score_fn(xs) + logprior(xs)
    p = np.exp(s - s.max())
    c = np.concatenate([[0.0], np.cumsum(0.5 * (p[1:] + p[:-1]) * np.diff(xs))])
    c /= c[-1]
    return lambda v: np.interp(v, xs, c)


def _support_bounds(score_fn, logprior, lo, hi):
    xs = np.logspace(np.log10(lo), np.log10(hi), 10000)
    s = score_fn(xs) + logprior(xs)
    keep = xs[s > s.max() - 40.0]
    return keep.min() * 0.9, keep.max() * 1.1


# Gates of the stationarity tests: the KS distance of n independent draws exceeds 1.95 / sqrt(n) with probability 1e-3;
# a slice chain's draws are correlated, and the gates allow an effective sample size of a quarter (the bound doubles).
# Seeds are fixed, so each outcome is deterministic.

def test_gp_alpha_chain_is_stationary(gpu_ctx):
    import common_amd
    from scipy import stats
    rng = np.random.default_rng(31)
    K = 64
    st = common_amd.State(gpu_ctx, [(orc.GP, 0)], K)
    empty = np.zeros(K, bool)
    empty[::5] = True
    rec, n = _records(orc.GP, 0, K, rng, empty)
    st.set_ss(0, rec)
    st.set_group_counts(n)
    st.set_hp(0, np.array([2.0, 0.5], np.float32))
    lam = sh.f32(1.0)

    def score(xs):
        blocks = np.stack([xs.astype(np.float32), np.full(xs.shape, 0.5, np.float32)], 1)
        return st.hp_grid(0, blocks).scores().cpu().numpy()

    def prior(xs):
        return math.log(lam) - lam * np.asarray(xs, np.float64)
    coords = [{"feature": 0, "coord": 0, "width": 1.0, "prior": "exponential", "a": 1.0}]
    N = 4000
    xs = np.empty(N)
    for t in range(N):
        v, _ = st.hp_slice(coords, seed=3, sweep=t)
        xs[t] = v[0]
    lo, hi = _support_bounds(score, prior, 1e-3, 1e3)
    d = stats.kstest(xs, _posterior_cdf(score, lo, hi, prior)).statistic
    audit("slice.gp_alpha_ks", d, 2 * 1.95 / math.sqrt(N))
    st.close()


def test_crp_alpha_chain_is_stationary(gpu_ctx):
    import common_amd
    from scipy import stats
    rng = np.random.default_rng(32)
    K = 64
    st = common_amd.State(gpu_ctx, [(orc.BB, 0)], K)
    n = rng.integers(1, 40, K).astype(np.uint32)
    n[rng.random(K) < 0.6] = 0
    st.set_group_counts(n)
    st.set_alpha(1.0)

    def score(xs):
        return st.crp_grid(np.asarray(xs, np.float32)).scores().cpu().numpy()

    def prior(xs):
        return -np.asarray(xs, np.float64)
    coords = [{"feature": "alpha", "width": 2.0, "prior": "exponential", "a": 1.0}]
    N = 4000
    xs = np.empty(N)
    for t in range(N):
        v, _ = st.hp_slice(coords, seed=4, sweep=t)
        xs[t] = v[0]
    lo, hi = _support_bounds(score, prior, 1e-3, 1e3)
    d = stats.kstest(xs, _posterior_cdf(score, lo, hi, prior)).statistic
    audit("slice.crp_alpha_ks", d, 2 * 1.95 / math.sqrt(N))
    st.close()


def test_theta_chains_are_beta_distributed(gpu_ctx):
    import common_amd
    from scipy import stats
    rng = np.random.default_rng(33)
    K = 64
    a, b = 1.5, 2.0
    st = common_amd.State(gpu_ctx, [(orc.BBNC, 0)], K)
    rec = np.zeros(K, dtype=common_amd.ss_dtype(orc.BBNC, 0))
    rec["heads"] = rng.integers(0, 40, K)
    rec["tails"] = rng.integers(0, 40, K)
    rec["heads"][:4] = [0, 0, 50, 1]
    rec["tails"][:4] = [0, 50, 0, 1]
    rec["p"] = 0.5
    st.set_ss(0, rec)
    st.set_hp(0, np.array([a, b], np.float32))
    slots = torch.ones(K, dtype=torch.uint8, device=gpu_ctx.torch_device)   # (a group with no data is counted too)
    N = 2000
    ps = np.empty((N, K))
    for t in range(N):
        st.theta_slice({0: {"p": 0.3}}, seed=6, sweep=t, slots=slots)
        ps[t] = st.get_ss(0)["p"]
    A, B = a + rec["heads"].astype(np.float64), b + rec["tails"].astype(np.float64)
    pit = stats.beta(A, B).cdf(ps).ravel()
    d = stats.kstest(pit, "uniform").statistic
    audit("slice.theta_pooled_pit_ks", d, 2 * 1.95 / math.sqrt(pit.size / 4))
    mean, var = A / (A + B), A * B / ((A + B) ** 2 * (A + B + 1))
    # per group: the chain mean within 5 standard errors (effective sample size N / 4), the variance within 35 % (its
    # relative standard error is sqrt((kurtosis - 1) / ESS): 6 % for a symmetric Beta at N / 4 draws, up to ~13 % for the
    # most skewed groups here, Beta(51.5, 2) and Beta(1.5, 52), which also mix slowest; the worst of 64 groups was 0.23
    # when written)
    audit("slice.theta_mean_z", np.max(np.abs(ps.mean(0) - mean) / np.sqrt(var / (N / 4))), 5.0)
    audit("slice.theta_var_rel", np.max(np.abs(ps.var(0) / var - 1)), 0.35)
    st.close()


@pytest.mark.parametrize("graph", [False, True])
def test_installed_values_equal_set_hp_through_scoring_and_sweeps(gpu_ctx, graph, monkeypatch):
    import common_amd
    from common_amd import hypers, models, scalar_functions as sf
    monkeypatch.setenv("MSC_SWEEP_GRAPH", "1" if graph else "0")
    N, K = 3000, 32
    rng = np.random.default_rng(41)
    specs = [(orc.BB, models.bb), (orc.GP, models.gp), (orc.NICH, models.nich), (orc.BBNC, models.bbnc)]
    feats = [make_feature(f, N, K, rng) for f, _ in specs]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    z0 = rng.integers(0, K - 4, N).astype(np.int32)
    p0 = rng.uniform(0.05, 0.95, K).astype(np.float32)
    pair = []
    for _ in range(2):
        st = common_amd.State(gpu_ctx, [(f, 0) for f, _ in specs], K)
        st.set_alpha(1.0)
        z = torch.from_numpy(z0).to(gpu_ctx.torch_device)
        st.accumulate(view, z)
        rec = st.get_ss(3)
        rec["p"] = p0
        st.set_ss(3, rec)
        pair.append((st, z))
    (a, za), (b, zb) = pair
    sl = hypers.FeatureHpSlice(a, [d for _, d in specs], cparam={"alpha": (sf.log_exponential(1.0), 1.0)})
    out = sl.step(seed=4, sweep=0)
    ev = a.theta_slice({3: {"p": 0.25}}, seed=4, sweep=0)
    assert ev[3] > 0
    for f in range(len(specs)):
        hp = a.get_hp(f)
        assert hypers.unpack_hp(specs[f][0], hp) == out[f]
        b.set_hp(f, hp)
    b.set_alpha(out["alpha"])
    b.set_ss(3, a.get_ss(3))
    assert not np.array_equal(a.get_ss(3)["p"], p0)
    sa = a.score_value(view, nrows=256, crp_prior=True).cpu().numpy()   # (the bbnc tables follow the new p)
    sb = b.score_value(view, nrows=256, crp_prior=True).cpu().numpy()
    assert np.array_equal(sa, sb)
    assert np.array_equal(a.score_data().cpu().numpy(), b.score_data().cpu().numpy())
    for sweep in range(3):
        a.sweep_step(view, za, seed=9, sweep=sweep)
        b.sweep_step(view, zb, seed=9, sweep=sweep)
        assert torch.equal(za, zb)
    assert np.array_equal(a.score_data().cpu().numpy(), b.score_data().cpu().numpy())
    for f in range(len(specs)):
        ra, rb = a.get_ss(f), b.get_ss(f)
        for name in ra.dtype.names:
            assert np.array_equal(ra[name], rb[name]), (f, name)


def test_same_seed_same_bits_other_seed_other_draws(gpu_ctx):
    st, recs, n, coords = _mixed_state(gpu_ctx, 300, 8)
    pre = [st.get_hp(f).copy() for f in range(len(SPECS))]
    bbnc_pre = st.get_ss(1)
    runs = []
    for seed in (21, 21, 22):
        for f in range(len(SPECS)):
            st.set_hp(f, pre[f])
        st.set_alpha(1.3)
        st.set_ss(1, bbnc_pre)
        v, e = st.hp_slice(coords, seed=seed, sweep=2)
        st.theta_slice({1: {"p": 0.2}}, seed=seed, sweep=2)
        runs.append((v, e, st.get_ss(1)["p"], [st.get_hp(f).copy() for f in range(len(SPECS))]))
    (v1, e1, p1, h1), (v2, e2, p2, h2), (v3, _, p3, _) = runs
    assert np.array_equal(v1.view(np.uint32), v2.view(np.uint32)) and np.array_equal(e1, e2)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(h1, h2))
    assert np.count_nonzero(v1 != v3) >= len(v1) - 1
    counted = n > 0
    assert np.count_nonzero(p1[counted] != p3[counted]) >= counted.sum() - 1
    st.close()


def test_unsupported_families_and_coordinates(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    st = common_amd.State(gpu_ctx, [(orc.NIW, 2), (orc.DD, 3), (orc.DM, 3), (orc.BNB, 0), (orc.BB, 0)], 8)
    for f, k in ((0, 0), (1, 0), (2, 1), (3, 2)):
        with pytest.raises(MicroscopesHipError) as e:
            st.hp_slice([{"feature": f, "coord": k, "width": 1.0}], seed=1, sweep=0)
        assert e.value.code == -4, (f, k)                          # MSC_EUNSUPPORTED
    with pytest.raises(MicroscopesHipError) as e:
        st.theta_slice({4: {"p": 0.1}}, seed=1, sweep=0)           # bb groups carry no parameter
    assert e.value.code == -1
    st.close()


def test_bad_arguments_install_nothing(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    st, recs, n, coords = _mixed_state(gpu_ctx, 64, 9)
    pre = [st.get_hp(f).copy() for f in range(len(SPECS))]
    bad = [dict(coords[0], width=0.0), dict(coords[0], width=-1.0), dict(coords[0], width=float("inf")),
           dict(coords[0], coord=2), dict(coords[6], prior="exponential", a=0.0), dict(coords[6], prior=9),
           dict(coords[0], partner=0), {"feature": "alpha", "coord": 1, "width": 1.0}, {"feature": 9, "width": 1.0}]
    for c in bad:
        with pytest.raises(MicroscopesHipError) as e:
            st.hp_slice(coords[:3] + [c], seed=1, sweep=0)
        assert e.value.code == -1, c
        assert all(np.array_equal(st.get_hp(f), pre[f]) for f in range(len(SPECS)))
    for t in ({1: {"p": 0.0}}, {1: {"p": -2.0}}, {0: {"p": 0.1}}):
        with pytest.raises(MicroscopesHipError) as e:
            st.theta_slice(t, seed=1, sweep=0)
        assert e.value.code == -1
    st.close()


def test_non_finite_start_keeps_its_value_and_the_rest_is_installed(gpu_ctx):
    from common_amd import MicroscopesHipError
    st, recs, n, coords = _mixed_state(gpu_ctx, 64, 10)
    # nich mu under an exponential prior at mu = -1: the prior is -inf there (mu's support is every real)
    st.set_hp(4, np.array([-1.0, 2.0, 1.5, 3.0], np.float32))
    pre = [st.get_hp(f).copy() for f in range(len(SPECS))]
    cs = [_coord(0, SPECS[0][2][0]), {"feature": 4, "coord": 0, "width": 1.0, "prior": "exponential", "a": 1.0},
          _coord(4, SPECS[4][2][1])]
    with pytest.raises(MicroscopesHipError) as e:
        st.hp_slice(cs, seed=2, sweep=0)
    assert e.value.code == -1 and "feature 4" in str(e.value)
    assert st.get_hp(4)[0] == np.float32(-1.0)                   # left unchanged ...
    assert st.get_hp(4)[1] != pre[4][1] and st.get_hp(0)[0] != pre[0][0]   # ... the rest installed
    # a counted bbnc slot whose p is not a probability
    rec = st.get_ss(1)
    k = int(np.flatnonzero(n > 0)[0])
    rec["p"][k] = 7.0
    st.set_ss(1, rec)
    with pytest.raises(MicroscopesHipError) as e:
        st.theta_slice({1: {"p": 0.2}}, seed=2, sweep=0)
    assert e.value.code == -1 and ("slot %d" % k) in str(e.value)
    post = st.get_ss(1)
    assert post["p"][k] == np.float32(7.0)
    others = (n > 0) & (np.arange(len(n)) != k)
    assert np.count_nonzero(post["p"][others] != rec["p"][others]) >= others.sum() - 1
    st.close()


def test_refused_inside_a_sharded_step(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    N, K = 500, 8
    rng = np.random.default_rng(2)
    feats = [make_feature(orc.BBNC, N, K, rng)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = common_amd.State(gpu_ctx, [(orc.BBNC, 0)], K)
    st.set_alpha(1.0)
    z = torch.from_numpy(rng.integers(0, K, N).astype(np.int32)).to(gpu_ctx.torch_device)
    st.accumulate(view, z)
    rec = st.get_ss(0)
    rec["p"] = 0.5
    st.set_ss(0, rec)
    coords = [{"feature": 0, "coord": 0, "width": 1.0, "prior": "noninf_beta", "partner": 1}]
    st.sweep_step_begin(view, z, seed=1, sweep=0)
    for call in (lambda: st.hp_slice(coords, 1, 0), lambda: st.theta_slice({0: {"p": 0.1}}, 1, 0)):
        with pytest.raises(MicroscopesHipError) as e:
            call()
        assert e.value.code == -1
    st.commit_reduce()
    st.hp_slice(coords, 1, 0)
    st.theta_slice({0: {"p": 0.1}}, 1, 0)
