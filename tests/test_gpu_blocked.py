"""GPU: the blocked Gibbs sampler (msc_blocked_draw / _tables / _assign, msc_sweep_blocked) -- the assignment replayed in
double from the drawn tables, the draws against their posteriors, the exact posterior of six rows, determinism and the
shard rule, the tables on return, and the error cases."""
import math

import numpy as np
import pytest
import torch
from scipy import stats

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]
P_GATE = 1e-3


def _setup(gpu_ctx, specs, N, K, seed, alpha=1.3, masked=False, gp_large=False, empty=2, z=None, all_masked_row=None):
    """features, a view, a state accumulated from z on the device, and the replay's (family, values, mask)"""
    import common_amd
    rng = np.random.default_rng(seed)
    feats = [make_feature(f, N, max(K, 2), rng, d) for f, d in specs]
    if gp_large:
        for f in feats:
            if f["family"] in (orc.GP, orc.BNB):
                f["values"] = f["values"].copy()
                f["values"][::37] = rng.integers(1024, 3000, len(f["values"][::37])).astype(np.uint32)
    masks = [rng.random(N) < 0.2 for _ in feats] if masked else [None] * len(feats)
    if all_masked_row is not None:
        for m in masks:
            m[all_masked_row] = True
    data = recarray_of(feats)
    if masked:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in data.dtype.names])
        for i, m in enumerate(masks):
            mask["f%d" % i] = m
        data = np.ma.masked_array(data, mask=mask)
    view = common_amd.DataView.from_recarray(gpu_ctx, data)
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    for i, f in enumerate(feats):
        st.set_hp(i, f["hp"])
    st.set_alpha(alpha)
    if z is None:
        z = rng.integers(0, max(1, K - empty), N).astype(np.int32)
    st.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device))
    return dict(view=view, st=st, z=z, alpha=alpha, K=K, N=N, feats=feats,
                rfeats=[(f["family"], f["values"], m) for f, m in zip(feats, masks)])


def _scores(tabs, rfeats, rows):
    """s[r, k] = log pi_k + sum over features of the log-likelihood of row r under slot k, in float64 from the float32
    tables"""
    s = np.repeat(tabs["logw"].cpu().numpy().astype(np.float64)[None, :], len(rows), axis=0)
    for i, (family, values, mask) in enumerate(rfeats):
        t = tabs[i].cpu().numpy().astype(np.float64)
        v = values[rows]
        if family == orc.BB:
            add = np.where(v.astype(bool)[:, None], t[1][None, :], t[0][None, :])
        elif family in (orc.GP, orc.BNB):
            add = t[0][None, :] + v.astype(np.float64)[:, None] * t[1][None, :]
        elif family == orc.DD:
            add = t[v.astype(np.int64)]
        else:
            add = t[0][None, :] + t[2][None, :] * (v.astype(np.float64)[:, None] - t[1][None, :]) ** 2
        if mask is not None:
            add = np.where(mask[rows][:, None], 0.0, add)
        s += add
    return s


def _check_assign(s, got, seed, sweep, row_ids, tol=1e-5):
    n_off = 0
    for r in range(len(got)):
        p = orc.scores_to_probs(s[r])
        u = orc.uniform01(seed, sweep, int(row_ids[r]))
        want = int(orc.sample_discrete(p, u))
        if int(got[r]) != want:
            cdf = np.cumsum(p)
            lo, hi = sorted((int(got[r]), want))
            assert abs(cdf[lo] - u) < tol or p[lo + 1:hi + 1].sum() < tol, (r, got[r], want, cdf[lo], u)
            n_off += 1
    assert n_off <= max(3, 0.005 * len(got)), n_off
    return n_off


def _draw_assign_replay(gpu_ctx, s, seed, sweep, row0=0, nrows=None, row_id0=None):
    st, view = s["st"], s["view"]
    n = s["N"] - row0 if nrows is None else nrows
    rid0 = row0 if row_id0 is None else row_id0
    st.blocked_draw(seed, sweep)
    tabs = st.blocked_tables()
    for t in tabs.values():
        assert bool(torch.isfinite(t).all())
    zt = torch.full((n,), -5, dtype=torch.int32, device=gpu_ctx.torch_device)
    st.blocked_assign(view, zt, seed, sweep, row0=row0, nrows=n, row_id0=row_id0)
    got = zt.cpu().numpy()
    assert ((got >= 0) & (got < s["K"])).all()
    rows = np.arange(row0, row0 + n)
    _check_assign(_scores(tabs, s["rfeats"], rows), got, seed, sweep, rid0 + np.arange(n))
    return got, tabs


FAMILY_CASES = {
    "bb": dict(specs=[(orc.BB, 0)] * 3),
    "gp": dict(specs=[(orc.GP, 0)]),
    "gp_beyond_table": dict(specs=[(orc.GP, 0)], gp_large=True),
    "bnb": dict(specs=[(orc.BNB, 0)]),
    "dd2": dict(specs=[(orc.DD, 2)]),
    "dd128": dict(specs=[(orc.DD, 128)]),
    "nich": dict(specs=[(orc.NICH, 0)]),
    "c3_mix": dict(specs=C3_SMALL),
    "masked_mix": dict(specs=C3_SMALL + [(orc.BNB, 0)], masked=True),
}


@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_assign_replay_per_family(gpu_ctx, case):
    c = FAMILY_CASES[case]
    s = _setup(gpu_ctx, c["specs"], 2000, 48, seed=sum(map(ord, case)), masked=c.get("masked", False),
               gp_large=c.get("gp_large", False))
    _draw_assign_replay(gpu_ctx, s, seed=11, sweep=2)


@pytest.mark.parametrize("K", [1, 2, 7, 64, 65, 256, 257, 1000, 1024])
def test_assign_replay_across_slot_counts(gpu_ctx, K):
    s = _setup(gpu_ctx, C3_SMALL, 2000, K, seed=100 + K)
    _draw_assign_replay(gpu_ctx, s, seed=5 + K, sweep=1)


def test_assign_replay_row_offsets(gpu_ctx):
    s = _setup(gpu_ctx, C3_SMALL, 2000, 48, seed=9, masked=True)
    _draw_assign_replay(gpu_ctx, s, seed=21, sweep=7, row0=300, nrows=1200, row_id0=50000)


def test_assign_replay_many_features_takes_the_other_kernels(gpu_ctx):
    """beyond 64 features the staged kernel runs 64 rows a workgroup, beyond 256 the values are re-read from the columns"""
    for nfeat, N in ((70, 600), (260, 300)):
        s = _setup(gpu_ctx, [(orc.BB, 0)] * (nfeat - 2) + [(orc.NICH, 0), (orc.DD, 5)], N, 20, seed=nfeat)
        _draw_assign_replay(gpu_ctx, s, seed=3, sweep=nfeat)


def test_a_row_with_every_entry_masked_draws_from_the_weights(gpu_ctx):
    s = _setup(gpu_ctx, C3_SMALL, 2000, 48, seed=19, masked=True, all_masked_row=777)
    got, tabs = _draw_assign_replay(gpu_ctx, s, seed=8, sweep=3)
    w = np.exp(tabs["logw"].cpu().numpy().astype(np.float64))
    u = orc.uniform01(8, 3, 777)
    want = int(orc.sample_discrete(orc.scores_to_probs(np.log(w)), u))
    cdf = np.cumsum(w / w.sum())
    assert got[777] == want or abs(cdf[min(got[777], want)] - u) < 1e-5


# ---- the draws ---------------------------------------------------------------------------------------------------------
def _ks(x, dist):
    p = stats.kstest(x, dist.cdf).pvalue
    assert p >= P_GATE, p


def _identical_slots(gpu_ctx, family, dim, hp, record, K=4096, count=0):
    import common_amd
    st = common_amd.State(gpu_ctx, [(family, dim)], K)
    st.set_hp(0, hp)
    st.set_alpha(1.0)
    rec = np.zeros(K, dtype=common_amd.ss_dtype(family, dim))
    for name, v in record.items():
        rec[name] = v
    st.set_ss(0, rec)
    st.set_group_counts(np.full(K, count, dtype=np.uint32))
    st.blocked_draw(123, 4)
    tabs = st.blocked_tables()
    t = tabs[0].cpu().numpy().astype(np.float64)
    assert np.isfinite(t).all() and np.isfinite(tabs["logw"].cpu().numpy()).all()
    return t, tabs


@pytest.mark.parametrize("n", [0, 500])
def test_device_draws_follow_the_posterior(gpu_ctx, n):
    rng = np.random.default_rng(5 + n)
    # bb
    heads = int((rng.random(n) < 0.3).sum())
    t, _ = _identical_slots(gpu_ctx, orc.BB, 0, dict(alpha=1.5, beta=0.7), dict(heads=heads, tails=n - heads), count=n)
    _ks(np.exp(t[1]), stats.beta(1.5 + heads, 0.7 + n - heads))
    _ks(np.exp(t[0]), stats.beta(0.7 + n - heads, 1.5 + heads))
    # gp
    tot = int(rng.poisson(4.0, n).sum())
    t, _ = _identical_slots(gpu_ctx, orc.GP, 0, dict(alpha=2.0, inv_beta=0.5), dict(count=n, sum=tot), count=n)
    _ks(-t[0], stats.gamma(2.0 + tot, scale=1.0 / (0.5 + n)))
    _ks(np.exp(t[1]), stats.gamma(2.0 + tot, scale=1.0 / (0.5 + n)))
    # bnb
    t, _ = _identical_slots(gpu_ctx, orc.BNB, 0, dict(alpha=1.5, beta=2.0, r=3), dict(count=n, sum=tot), count=n)
    _ks(np.exp(t[0] / 3.0), stats.beta(1.5 + 3.0 * n, 2.0 + tot))
    _ks(np.exp(t[1]), stats.beta(2.0 + tot, 1.5 + 3.0 * n))
    # dd
    dim = 5
    counts = np.bincount(rng.integers(0, dim, n), minlength=dim)
    alphas = [0.4, 1.0, 2.5, 0.9, 1.3]
    t, _ = _identical_slots(gpu_ctx, orc.DD, dim, dict(alphas=alphas), dict(count_sum=n, counts=counts), count=n)
    a = np.asarray(alphas, dtype=np.float32).astype(np.float64) + counts
    assert np.allclose(np.exp(t).sum(0), 1.0, atol=1e-5)
    for i in range(dim):
        _ks(np.exp(t[i]), stats.beta(a[i], a.sum() - a[i]))
    # nich
    v = rng.normal(2.0, 1.5, n).astype(np.float32).astype(np.float64)
    mean = np.float32(v.mean()) if n else np.float32(0)
    ctv = np.float32(((v - float(mean)) ** 2).sum()) if n else np.float32(0)
    mu, kappa, sigmasq, nu = 0.25, 0.75, 1.5, 2.5
    t, _ = _identical_slots(gpu_ctx, orc.NICH, 0, dict(mu=mu, kappa=kappa, sigmasq=sigmasq, nu=nu),
                            dict(count=n, mean=mean, count_times_variance=ctv), count=n)
    mean, ctv = float(mean), float(ctv)
    kn, nun = kappa + n, nu + n
    mu_n = (kappa * mu + n * mean) / kn
    s_n = (nu * sigmasq + ctv + n * kappa * (mu - mean) ** 2 / kn) / nun
    sig2 = -0.5 / t[2]
    _ks(sig2, stats.invgamma(nun / 2.0, scale=nun * s_n / 2.0))
    _ks((t[1] - mu_n) / np.sqrt(sig2 / kn), stats.norm())
    assert np.allclose(t[0], -0.5 * np.log(2.0 * math.pi * sig2), rtol=1e-5, atol=1e-5)


def test_device_stick_weights(gpu_ctx):
    """the weights sum to one, and V_k = pi_k / (1 - sum_{l < k} pi_l) passes a probability integral transform under
    Beta(1 + n_k, alpha + sum_{l > k} n_l) wherever the float32 weights still resolve it (remaining mass above 1e-2)"""
    import common_amd
    K, alpha = 4096, 0.7
    rng = np.random.default_rng(17)
    cnt = (rng.integers(0, 30, K) * (rng.random(K) < 0.6)).astype(np.uint32)
    after = np.concatenate([np.cumsum(cnt[::-1].astype(np.float64))[::-1][1:], [0.0]])
    st = common_amd.State(gpu_ctx, [(orc.BB, 0)], K)
    st.set_alpha(alpha)
    st.set_group_counts(cnt)
    pit = []
    for sweep in range(8):
        st.blocked_draw(9, sweep)
        lw = st.blocked_tables()["logw"].cpu().numpy().astype(np.float64)
        assert np.isfinite(lw).all()
        w = np.exp(lw)
        # float32 log weights near -8 carry 5e-7 absolute error each: the sum is within 1e-5 of one
        assert abs(w.sum() - 1.0) <= 1e-5
        rest = 1.0 - np.concatenate([[0.0], np.cumsum(w)[:-1]])
        keep = np.nonzero(rest > 1e-2)[0]
        pit.append(stats.beta(1.0 + cnt[keep], alpha + after[keep]).cdf(w[keep] / rest[keep]))
    pit = np.concatenate(pit)
    assert pit.size >= 8 * 1000
    assert stats.kstest(pit, "uniform").pvalue >= P_GATE


def test_draws_are_finite_under_edge_hyperparameters(gpu_ctx):
    t, _ = _identical_slots(gpu_ctx, orc.NICH, 0, dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=0.5),
                            dict(count=0, mean=0.0, count_times_variance=0.0))
    assert np.isfinite(t).all()
    t, _ = _identical_slots(gpu_ctx, orc.GP, 0, dict(alpha=0.05, inv_beta=1.0), dict(count=300, sum=0), count=300)
    assert np.isfinite(t).all() and (t[0] <= 0).all()
    t, _ = _identical_slots(gpu_ctx, orc.BB, 0, dict(alpha=1.0, beta=1.0), dict(heads=1000000, tails=0), count=1000000)
    assert np.isfinite(t).all() and (t[1] <= 0).all() and (t[1] > -1e-3).all()


# ---- the chain ---------------------------------------------------------------------------------------------------------
def test_exact_posterior_of_six_rows(gpu_ctx):
    """N = 6, K = 32, alpha = 1: 5e4 blocked sweeps visit the 203 partitions with the exact posterior's frequencies
    (truncation bound 4 N exp(-(K - 1) / alpha) = 8e-13)"""
    import common_amd
    rng = np.random.default_rng(2024)
    dev = gpu_ctx.torch_device
    N, K, alpha, per_call, calls = 6, 32, 1.0, 10000, 5
    datasets = {
        "bb3": [make_feature(orc.BB, N, 2, rng) for _ in range(3)],
        "nich_bb": [make_feature(orc.NICH, N, 2, rng), make_feature(orc.BB, N, 2, rng)],
    }
    datasets["nich_bb"][0]["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    for name, feats in datasets.items():
        Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
        parts, p = sh.exact_posterior([(F, f["values"]) for F, f in zip(Fs, feats)], alpha)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
        st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
        for i, F in enumerate(Fs):
            st.set_hp(i, F.hp)
        st.set_alpha(alpha)
        zt = torch.full((N,), -1, dtype=torch.int32, device=dev)
        st.accumulate(view, zt)
        trace = torch.empty(per_call * N, dtype=torch.int32, device=dev)
        top = torch.empty(per_call, dtype=torch.int32, device=dev)
        traces = []
        for c in range(calls):
            st.sweep_blocked(view, zt, 77, c * per_call, nsweeps=per_call, trace=trace, top_slot=top)
            traces.append(trace.cpu().numpy().reshape(per_call, N))
            tp = top.cpu().numpy()
            assert (tp >= 0).all() and (tp <= K - 1).all()
            assert np.array_equal(tp, traces[-1].max(axis=1))
        freq = sh.partition_frequencies(np.concatenate(traces), parts)
        tv, kl = sh.tv_kl(freq, p)
        print("exact posterior %s: blocked TV %.4f KL %.5f" % (name, tv, kl))
        assert tv <= 0.05 and kl <= 0.01, (name, tv, kl)


def _tables_bits(st):
    return {k: t.cpu().numpy().view(np.uint32).copy() for k, t in st.blocked_tables().items()}


def test_same_arguments_same_bits_and_split_calls(gpu_ctx):
    dev = gpu_ctx.torch_device
    runs = []
    for way in ("one", "one", "two"):
        s = _setup(gpu_ctx, C3_SMALL, 1500, 50, seed=61)
        zt = torch.from_numpy(s["z"].copy()).to(dev)
        if way == "one":
            s["st"].sweep_blocked(s["view"], zt, 17, 4, nsweeps=2)
        else:
            s["st"].sweep_blocked(s["view"], zt, 17, 4)
            s["st"].sweep_blocked(s["view"], zt, 17, 5)
        runs.append((zt.cpu().numpy(), _tables_bits(s["st"]), s["st"].get_group_counts()))
    for z, tb, cnt in runs[1:]:
        assert np.array_equal(z, runs[0][0])
        assert np.array_equal(cnt, runs[0][2])
        for k in tb:
            assert np.array_equal(tb[k], runs[0][1][k]), k


def test_equal_tables_draw_equal_parameters_and_shards_assign_the_same(gpu_ctx):
    dev = gpu_ctx.torch_device
    a = _setup(gpu_ctx, C3_SMALL + [(orc.BNB, 0)], 2000, 48, seed=71, masked=True)
    b = _setup(gpu_ctx, C3_SMALL + [(orc.BNB, 0)], 2000, 48, seed=71, masked=True)
    a["st"].blocked_draw(31, 6)
    b["st"].blocked_draw(31, 6)
    ta, tb = _tables_bits(a["st"]), _tables_bits(b["st"])
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    # another (seed, sweep) gives other parameters
    b["st"].blocked_draw(31, 7)
    assert not np.array_equal(ta["logw"], _tables_bits(b["st"])["logw"])
    N = a["N"]
    whole = torch.full((N,), -1, dtype=torch.int32, device=dev)
    parts = torch.full((N,), -1, dtype=torch.int32, device=dev)
    a["st"].blocked_assign(a["view"], whole, 31, 6)
    h = N // 2
    a["st"].blocked_assign(a["view"], parts[:h], 31, 6, row0=0, nrows=h, row_id0=0)
    a["st"].blocked_assign(a["view"], parts[h:], 31, 6, row0=h, nrows=N - h, row_id0=h)
    assert np.array_equal(whole.cpu().numpy(), parts.cpu().numpy())


def _compare_tables(gpu_ctx, s, z):
    """the state after the call against a fresh state accumulated from the final z"""
    import common_amd
    st, view = s["st"], s["view"]
    fresh = common_amd.State(gpu_ctx, st.features, s["K"])
    for i in range(len(st.features)):
        fresh.set_hp(i, st.get_hp(i))
    fresh.set_alpha(s["alpha"])
    fresh.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device), reset=True)
    assert np.array_equal(st.get_group_counts(), fresh.get_group_counts())
    assert np.array_equal(st.get_group_counts(), np.bincount(z, minlength=s["K"]).astype(np.uint32))
    for i in range(len(st.features)):
        a, b = st.get_ss(i), fresh.get_ss(i)
        for name in a.dtype.names:
            x, y = a[name].astype(np.float64), b[name].astype(np.float64)
            if np.issubdtype(a.dtype[name].base, np.integer):
                assert np.array_equal(x, y), name
            else:
                assert np.all(np.abs(x - y) <= 1e-6 * np.maximum(1.0, np.abs(y))), name


def test_tables_current_on_return_and_batched_stream_untouched(gpu_ctx):
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, C3_SMALL + [(orc.BNB, 0)], 3000, 96, seed=12, masked=True)
    st = s["st"]
    zt = torch.from_numpy(s["z"].copy()).to(dev)
    st.sweep_step(s["view"], zt, 23, 0)
    stats_before = st.sweep_step_stats()
    zb = zt.clone()
    top = torch.full((3,), -1, dtype=torch.int32, device=dev)
    st.sweep_blocked(s["view"], zb, 3, 0, nsweeps=3, top_slot=top)
    got = zb.cpu().numpy()
    assert ((got >= 0) & (got < s["K"])).all()
    assert int(top[-1].item()) == int(got.max())
    _compare_tables(gpu_ctx, s, got)
    assert st.sweep_step_stats() == stats_before
    # the batched stream goes on as on a state that never ran the blocked sweep
    import common_amd
    st.accumulate(s["view"], zt, reset=True)
    twin = common_amd.State(gpu_ctx, st.features, s["K"])
    for i in range(len(st.features)):
        twin.set_hp(i, st.get_hp(i))
    twin.set_alpha(s["alpha"])
    zt2 = zt.clone()
    twin.accumulate(s["view"], zt2, reset=True)
    st.sweep_step(s["view"], zt, 23, 1)
    twin.sweep_step(s["view"], zt2, 23, 1)
    assert np.array_equal(zt.cpu().numpy(), zt2.cpu().numpy())


@pytest.mark.parametrize("spec", [(orc.NIW, 3), (orc.DM, 4), (orc.BBNC, 0)])
def test_unsupported_families(gpu_ctx, spec):
    import common_amd
    s = _setup(gpu_ctx, [spec, (orc.NICH, 0)], 200, 8, seed=81)
    zt = torch.from_numpy(s["z"].copy()).to(gpu_ctx.torch_device)
    for call in (lambda: s["st"].blocked_draw(1, 0), lambda: s["st"].blocked_tables(),
                 lambda: s["st"].blocked_assign(s["view"], zt, 1, 0), lambda: s["st"].sweep_blocked(s["view"], zt, 1, 0)):
        with pytest.raises(common_amd.MicroscopesHipError) as e:
            call()
        assert e.value.code == -4


def test_errors(gpu_ctx):
    import common_amd
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, C3_SMALL, 500, 20, seed=91)
    st, view = s["st"], s["view"]
    zt = torch.from_numpy(s["z"].copy()).to(dev)

    def einval(call):
        with pytest.raises(common_amd.MicroscopesHipError) as e:
            call()
        assert e.value.code == -1

    assign = lambda: st.blocked_assign(view, zt.clone(), 1, 0)
    einval(assign)                                   # before any draw
    st.blocked_draw(1, 0)
    assign()
    st.accumulate(view, zt, reset=True)
    einval(assign)                                   # the draw is stale: the tables changed
    st.blocked_draw(1, 0)
    st.set_hp(0, dict(alpha=2.0, beta=1.0))
    einval(assign)
    st.blocked_draw(1, 0)
    st.set_alpha(2.0)
    einval(assign)
    st.blocked_draw(1, 0)
    st.set_group_counts(st.get_group_counts())
    einval(assign)
    st.blocked_draw(1, 0)
    st.sweep_step(view, zt, 1, 0)
    einval(assign)
    st.blocked_draw(1, 0)
    st.sweep_blocked(view, zt, 1, 0)                 # (leaves its own last draw stale: it accumulated after it)
    einval(assign)
    # between sweep_step_begin and commit_reduce
    st.sweep_step_begin(view, zt, 1, 0)
    einval(lambda: st.blocked_draw(1, 0))
    einval(assign)
    einval(lambda: st.sweep_blocked(view, zt, 1, 0))
    st.commit_reduce()
    st.blocked_draw(1, 1)
    assign()
    # bad tensors
    with pytest.raises(ValueError):
        st.sweep_blocked(view, zt.to(torch.int64), 1, 0)
    with pytest.raises(ValueError):
        st.sweep_blocked(view, zt, 1, 0, nsweeps=2, trace=torch.empty(500, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        st.sweep_blocked(view, zt, 1, 0, nsweeps=2, top_slot=torch.empty(1, dtype=torch.int32, device=dev))
    gpu_ctx.synchronize()
