"""Posterior predictive draws and imputation from a whole chain ensemble on the device (msc_chains_sample_predictive,
ChainEnsemble.sample_predictive / impute): the chain draw against the numpy running-sum rule over the device's own
per-chain rows, the group draw against the chosen chain's totals from State.score_value, the values bit for bit against
State.sample_predictive on the chosen chain and group, and the whole against an enumeration over set partitions.  The
cases, the uniforms and the rule for a row the comparison cannot decide are in tests/chains_predictive_helpers.py; that
the cases stay within the caps on such rows is checked without a device in tests/test_chains_predictive_cpu.py."""
import os
import re
import time

import numpy as np
import pytest
import torch
from scipy import stats

import common_amd
from oracle import oracle as orc
from tests import chains_marginal_helpers as M
from tests import chains_predictive_helpers as P
from tests import smc_helpers as H
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

SENTINEL = 7


def case(ctx, name):
    return M.EnsembleCase(ctx, P.twin_of(name))


def drawn_features(c):
    return [i for i, (fam, _) in enumerate(c.twin.specs) if fam != M.NOOP]


def sentinels(c, n, feats=None):
    """one output tensor a drawn feature, every entry SENTINEL in the family's type"""
    out = {}
    for f in drawn_features(c) if feats is None else feats:
        dt = common_amd.State._PRED_DTYPES[c.twin.specs[f][0]]
        if dt in (torch.float32, torch.uint8):
            out[f] = torch.full((n,), SENTINEL, dtype=dt, device=c.ctx.torch_device)
        else:                                          # (uint32, int32)
            out[f] = torch.full((n,), SENTINEL, dtype=torch.int32, device=c.ctx.torch_device).view(dt)
    return out


def bits(t):
    """a tensor's bits in a dtype torch indexes and compares (uint32 and float32 as int32)"""
    return t.view(torch.int32) if t.element_size() == 4 else t


def host(t):
    """a value tensor on the host, in its own type"""
    np_of = {torch.uint8: np.uint8, torch.uint32: np.uint32, torch.int32: np.int32, torch.float32: np.float32}
    return bits(t).cpu().numpy().view(np_of[t.dtype])


def draw(c, weights=None, masked_only=False, **kw):
    n = kw.get("nrows", int(c.view.nrows) - kw.get("row0", 0))
    kw.setdefault("out", sentinels(c, n))
    kw.setdefault("features", drawn_features(c))
    vals, chains, groups = c.ens.sample_predictive(c.view, weights=weights, seed=P.SEED, sweep=P.SWEEP,
                                                   masked_only=masked_only, **kw)
    torch.cuda.synchronize()
    return vals, chains, groups


def same_bytes(a, b):
    return all(torch.equal(bits(a[0][f]), bits(b[0][f])) for f in a[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_the_chain_draw_is_the_running_sum_rule_over_the_devices_own_rows(gpu_ctx, name):
    c = case(gpu_ctx, name)
    n = int(c.view.nrows)
    u1, _ = P.uniforms(P.SEED, np.arange(n), P.SWEEP)
    for logw in (None, P.weights_of(name)):
        _, Lf = c.ens.predictive_logp(c.view, weights=logw, per_chain=True)
        _, chains, _ = draw(c, weights=logw)
        want, undecided = P.chain_rule(M.normalised(logw, c.twin.nchains), Lf.cpu().numpy(), u1)
        got = chains.cpu().numpy()
        print("%s: %d rows, %d undecided, %d chains drawn" % (name, n, undecided.sum(), len(np.unique(got))))
        assert undecided.mean() <= P.CHAIN_CAP
        assert np.array_equal(got[~undecided], want[~undecided])
        assert (got >= 0).all() and (got < c.twin.nchains).all()
        if logw is not None and c.twin.nchains >= 3:
            assert not np.isin(got, np.flatnonzero(np.isneginf(logw))).any()    # (a weight of -inf leaves a chain out)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_the_group_draw_follows_the_chosen_chains_scores(gpu_ctx, name):
    c = case(gpu_ctx, name)
    n = int(c.view.nrows)
    _, u2 = P.uniforms(P.SEED, np.arange(n), P.SWEEP)
    _, chains, groups = draw(c, weights=P.weights_of(name))
    chains, groups = chains.cpu().numpy(), groups.cpu().numpy()
    undecided, want = np.zeros(n, dtype=bool), np.full(n, -1)
    for ch in np.unique(chains):
        mine = np.flatnonzero(chains == ch)
        t = c.ens.states[int(ch)].score_value(c.view, crp_prior=True).cpu().numpy()
        want[mine], undecided[mine] = P.group_rule(t[mine], u2[mine])
    print("%s: %d rows, undecided group %.4f" % (name, n, undecided.mean()))
    assert undecided.mean() <= P.GROUP_CAP
    assert np.array_equal(groups[~undecided], want[~undecided])
    assert (groups >= 0).all() and (groups < c.twin.K).all()


@pytest.mark.parametrize("masked_only", [False, True])
@pytest.mark.parametrize("name", sorted(P.CASES))
def test_the_values_are_the_chosen_states_own_draws_bit_for_bit(gpu_ctx, name, masked_only):
    c = case(gpu_ctx, name)
    n = int(c.view.nrows)
    feats = drawn_features(c)
    vals, chains, groups = draw(c, weights=P.weights_of(name), masked_only=masked_only)
    for ch in torch.unique(chains).tolist():
        rows = chains == ch
        z = torch.where(rows, groups, torch.full_like(groups, -1))
        own, used = c.ens.states[ch].sample_predictive(c.view, z=z, seed=P.SEED, sweep=P.SWEEP, masked_only=masked_only,
                                                       features=feats, out=sentinels(c, n))
        assert torch.equal(used[rows], groups[rows])
        for f in feats:
            assert torch.equal(bits(own[f])[rows], bits(vals[f])[rows]), (name, ch, f)
    if masked_only:                                    # observed entries are the view's
        for f in feats:
            seen = ~c.twin.masks[f]
            held = c.twin.held[f]["values"]
            got = host(vals[f])
            assert np.array_equal(got[seen], held[seen].astype(got.dtype)), (name, f)


@pytest.mark.parametrize("name", ["mix_k64_masked", "nich_k8_70_chains"])
def test_one_hot_weights_draw_from_that_chain_alone(gpu_ctx, name):
    c = case(gpu_ctx, name)
    nchains = c.twin.nchains
    for pick in sorted({0, nchains // 2, nchains - 1}):
        logw = np.full(nchains, -np.inf)
        logw[pick] = -2.75
        _, chains, groups = draw(c, weights=logw)
        assert bool((chains == pick).all()) and bool((groups >= 0).all())


def test_rows_no_chain_can_hold_and_weights_that_hold_nothing_are_skipped(gpu_ctx):
    """a held-out nich value of +inf is a row no group of any chain can hold: chain and group -1, the sentinel stays;
    weights that are all -inf, or hold a NaN or +inf, skip every row"""
    twin = M.build_twin(P.NICH1, 8, 3, P.N_TRAIN, 300, seed=12)
    twin.held[0]["values"] = twin.held[0]["values"].copy()
    twin.held[0]["values"][[5, 299]] = np.inf
    c = M.EnsembleCase(gpu_ctx, twin)
    vals, chains, groups = draw(c, weights=np.array([-np.inf, 0.0, -np.inf]))
    skipped = np.zeros(300, dtype=bool)
    skipped[[5, 299]] = True
    sk = torch.from_numpy(skipped).to(gpu_ctx.torch_device)
    assert bool((chains[sk] == -1).all()) and bool((groups[sk] == -1).all()) and bool((vals[0][sk] == SENTINEL).all())
    assert bool((chains[~sk] == 1).all()) and bool((groups[~sk] >= 0).all()) and bool(torch.isfinite(vals[0][~sk]).all())
    for logw in (np.full(3, -np.inf), np.array([0.0, np.nan, 0.0]), np.array([0.0, np.inf, 0.0])):
        vals, chains, groups = draw(c, weights=logw)
        assert bool((chains == -1).all()) and bool((groups == -1).all()) and bool((vals[0] == SENTINEL).all())


@pytest.mark.parametrize("name", ["mix_k64_masked", "nich_k8_3_chains_4100_rows", "wide_k300_big_counts"])
def test_row_ranges_give_the_whole_calls_bytes_and_a_call_repeats_them(gpu_ctx, name):
    c = case(gpu_ctx, name)
    n = int(c.view.nrows)
    logw = P.weights_of(name)
    for masked_only in (False, True):
        whole = draw(c, weights=logw, masked_only=masked_only)
        assert same_bytes(whole, draw(c, weights=logw, masked_only=masked_only))
        a = n // 3 + 7
        for r0, r1 in ((0, a), (a, n)):
            part = draw(c, weights=logw, masked_only=masked_only, row0=r0, nrows=r1 - r0, row_id0=r0)
            cut = ({f: t[r0:r1] for f, t in whole[0].items()}, whole[1][r0:r1], whole[2][r0:r1])
            assert same_bytes(cut, part), (name, r0, r1)
        # ... and the global row id alone names the draw: the same rows under other ids draw otherwise
        moved = draw(c, weights=logw, masked_only=masked_only, row0=0, nrows=a, row_id0=1000003)
        assert not torch.equal(moved[2], whole[2][:a])


def test_a_call_of_more_than_one_chunk_of_rows(gpu_ctx):
    """2^18 rows go through the handle's scratch at a time: a call over more, against calls cut elsewhere"""
    n = (1 << 18) + 300
    twin = M.build_twin([(orc.BB, 0)], 4, 2, P.N_TRAIN, n, seed=3)
    c = M.EnsembleCase(gpu_ctx, twin)
    whole = draw(c)
    a = 1000
    for r0, r1 in ((0, a), (a, n)):
        part = draw(c, row0=r0, nrows=r1 - r0, row_id0=r0)
        cut = ({f: t[r0:r1] for f, t in whole[0].items()}, whole[1][r0:r1], whole[2][r0:r1])
        assert same_bytes(cut, part), (r0, r1)
    assert bool((whole[1] >= 0).all()) and bool((whole[2] >= 0).all()) and bool((whole[0][0] <= 1).all())


def test_the_chain_draws_follow_the_weights_times_the_likelihoods(gpu_ctx):
    """20000 identical rows under other row ids, 5 chains: chi-square of the chains' counts against softmax(lw + Lf).
    The weights are set against the device's own Lf so that the five probabilities are uneven but none is small:
    (0.4, 0.25, 0.2, 0.1, 0.05).  The draws are a fixed function of the seed: the test is deterministic."""
    n = 20000
    twin = M.build_twin(P.NICH1, 8, 5, P.N_TRAIN, n, seed=21)
    twin.held[0]["values"] = np.full(n, twin.held[0]["values"][0], dtype=np.float32)
    c = M.EnsembleCase(gpu_ctx, twin)
    _, Lf = c.ens.predictive_logp(c.view, per_chain=True)
    Lf = Lf.cpu().numpy().astype(np.float64)
    assert (Lf == Lf[:, :1]).all()
    logw = np.log([0.4, 0.25, 0.2, 0.1, 0.05]) - Lf[:, 0]
    a = M.normalised(logw, 5) + Lf[:, 0]
    p = np.exp(a - a.max())
    p /= p.sum()
    _, chains, _ = draw(c, weights=logw)
    counts = np.bincount(chains.cpu().numpy(), minlength=5)
    pvalue = float(stats.chisquare(counts, p * n).pvalue)
    print("chain counts %s against %s: p = %.4g" % (counts, np.round(p * n, 1), pvalue))
    assert pvalue > 1e-6


def test_the_partitions_of_five_rows_impute_the_sixth_at_its_exact_predictive(gpu_ctx):
    """52 chains, one per set partition of five bb rows, weighted by the partitions' exact posterior; 2^17 rows whose only
    entry is masked are imputed.  The frequency of ones lies within 5 binomial standard deviations of p(x_6 = 1 |
    x_1..5) from the enumeration over set partitions of six rows -- a route that shares no code with the kernels."""
    feat6 = H.six_row_datasets()["bb"][0]
    twin, logw, exact = M.partition_twin(feat6, 1.0)
    p1 = float(np.exp(exact)) if bool(feat6["values"][5]) else 1.0 - float(np.exp(exact))
    n = 1 << 17
    twin.held[0] = dict(twin.held[0], values=np.zeros(n, dtype=np.bool_))
    twin.masks[0] = np.ones(n, dtype=bool)
    c = M.EnsembleCase(gpu_ctx, twin)
    vals, chains, groups = c.ens.impute(c.view, weights=logw, seed=11, sweep=0)
    ones = float(vals[0].to(torch.float64).mean().item())
    sd = float(np.sqrt(p1 * (1.0 - p1) / n))
    print("imputed ones %.5f, exact %.5f, %.2f sd" % (ones, p1, (ones - p1) / sd))
    assert bool((chains >= 0).all()) and bool((groups >= 0).all()) and bool((vals[0] <= 1).all())
    assert abs(ones - p1) <= 5.0 * sd
    # the chains drawn follow the partitions' posterior (every entry masked: the likelihood term is 1 for all)
    freq = np.bincount(chains.cpu().numpy(), minlength=52) / n
    w = np.exp(M.normalised(logw, 52))
    assert np.all(np.abs(freq - w) <= 5.0 * np.sqrt(w * (1.0 - w) / n) + 1.0 / n)


def test_the_particle_filters_weights_go_straight_in(gpu_ctx):
    feats, _, view = H.data(gpu_ctx, H.C3_SMALL, 48, 8, 77)
    ens = H.ensemble(gpu_ctx, feats, 8, 16)
    res = ens.smc(view, seed=5)
    assert np.isfinite(res.log_evidence)
    hfeats, masks, held = H.data(gpu_ctx, H.C3_SMALL, 90, 8, 78, mask_col=3)
    vals, chains, groups = ens.impute(held, weights=ens.logw, seed=1)
    torch.cuda.synchronize()
    assert bool((chains >= 0).all()) and bool((chains < 16).all()) and bool((groups >= 0).all()) and bool((groups < 8).all())
    assert vals[0].dtype == torch.uint8 and vals[1].dtype == torch.uint32 and vals[2].dtype == torch.int32 \
        and vals[3].dtype == torch.float32
    assert bool(torch.isfinite(vals[3]).all()) and bool((vals[0] <= 1).all())
    d = vals[2].cpu().numpy()
    assert ((d >= 0) & (d < 9)).all()
    seen = ~masks[3]
    assert np.array_equal(vals[3].cpu().numpy()[seen], hfeats[3]["values"][seen])
    assert not np.array_equal(vals[3].cpu().numpy()[~seen], hfeats[3]["values"][~seen])     # (the masked ones are drawn)


SWEEP_SPECS = [(orc.BB, 0), (orc.GP, 0), (orc.NICH, 0)]


def seated(gpu_ctx, seed=31):
    feats, _, view = H.data(gpu_ctx, SWEEP_SPECS, 120, 8, seed)
    ens = H.ensemble(gpu_ctx, feats, 8, 6, alpha=1.25)
    ens.seat(view, seed=17)
    return ens, view


def test_the_ensemble_is_read_only(gpu_ctx):
    """the bits of every member (and z, logw) are the same before and after, and a sweep on the training view that
    follows gives the z and the tables it gives without the call"""
    held_feats = [make_feature(f, 77, 6, np.random.default_rng(8), d) for f, d in SWEEP_SPECS]
    held_feats[1]["values"] = (held_feats[1]["values"] + 40).astype(np.uint32)
    held = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(held_feats))
    ens, view = seated(gpu_ctx)
    before = H.ensemble_bits(ens)
    ens.sample_predictive(held, seed=4)
    ens.impute(held, weights=np.log(np.arange(1.0, 7.0)), seed=4, sweep=1)
    assert H.ensemble_bits(ens) == before
    ens.sweep(view, 2, seed=9, sweep=1)
    torch.cuda.synchronize()
    with_call = H.ensemble_bits(ens)
    plain, view2 = seated(gpu_ctx)
    plain.sweep(view2, 2, seed=9, sweep=1)
    torch.cuda.synchronize()
    assert H.ensemble_bits(plain) == with_call


def test_bad_arguments(gpu_ctx):
    """every refusal of the entry point leaves the sentinel-filled outputs as they were.  (A drawn feature index >= 32768
    is refused too, but no ensemble reaches it: msc_chains_create takes at most 256 features.)"""
    twin = M.build_twin([(orc.NICH, 0), (orc.BB, 0), (M.NOOP, 0)], 8, 3, P.N_TRAIN, 100, seed=1)
    c = M.EnsembleCase(gpu_ctx, twin)
    dev, lib, ens, view = gpu_ctx.torch_device, gpu_ctx.lib, c.ens, c.view
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    einval = int(re.search(r"MSC_EINVAL\s*=\s*(-?\d+)", text).group(1))
    eunsup = int(re.search(r"MSC_EUNSUPPORTED\s*=\s*(-?\d+)", text).group(1))
    CT = common_amd._lib.C
    chain = torch.full((100,), SENTINEL, dtype=torch.int32, device=dev)
    z = torch.full((100,), SENTINEL, dtype=torch.int32, device=dev)
    o0 = torch.full((100,), float(SENTINEL), dtype=torch.float32, device=dev)
    o1 = torch.full((100,), SENTINEL, dtype=torch.uint8, device=dev)
    o2 = torch.full((100,), SENTINEL, dtype=torch.uint8, device=dev)
    outs = (CT.c_void_p * 3)(o0.data_ptr(), o1.data_ptr(), None)
    outs_noop = (CT.c_void_p * 3)(o0.data_ptr(), o1.data_ptr(), o2.data_ptr())
    u32 = lambda *v: (CT.c_uint32 * len(v))(*v)          # noqa: E731

    def call(h=ens._h, v=view._h, cols=None, row0=0, nrows=100, flags=0, o=outs):
        return lib.msc_chains_sample_predictive(h, v, cols, row0, nrows, row0, None, flags, 5, 0, chain.data_ptr(),
                                                z.data_ptr(), o)

    def refused(rc, code=einval):
        assert rc == code, rc
        torch.cuda.synchronize()
        for t in (chain, z, o0, o1, o2):
            assert bool((t == SENTINEL).all())
    refused(call(h=None))                                                 # null arguments
    refused(call(v=None))
    refused(call(o=None))
    refused(call(flags=2))                                                # unknown flags
    refused(call(flags=3))
    refused(call(nrows=1 << 32))
    refused(call(row0=50, nrows=51))                                      # rows outside the view
    rec3 = np.zeros(100, dtype=[("f0", np.float32), ("f1", np.bool_), ("f2", np.float32, (3,))])
    view3 = common_amd.DataView.from_recarray(gpu_ctx, rec3)
    refused(call(v=view3._h, cols=u32(2, 1, 1)))                          # three elements a value do not fit the nich feature
    refused(call(cols=u32(0, 9, 1)))                                      # a column outside the view
    refused(call(o=outs_noop), eunsup)                                    # the noop model has no values to draw
    zt = torch.zeros(100, dtype=torch.int32, device=dev)                  # member 1 between step_begin and commit_reduce
    ens.states[1].sweep_step_begin(view, zt, seed=3, sweep=0)
    refused(call())
    assert "state 1" in lib.msc_last_error().decode()                    # (the member is named)
    ens.states[1].commit_reduce()
    refused(call(nrows=0), 0)                                             # binds the view, writes nothing, MSC_OK
    assert call(flags=1) == 0
    torch.cuda.synchronize()
    assert bool((chain >= 0).all()) and bool((z >= 0).all()) and bool(torch.isfinite(o0).all()) and bool((o1 <= 1).all())
    assert bool((o2 == SENTINEL).all())
    # the binding's own checks come before any device call
    for kw in (dict(weights=np.zeros(3, dtype=np.float32)), dict(weights=np.zeros(4)), dict(features=[3]), dict(row0=-1),
               dict(row0=50, nrows=51), dict(seed=-1), dict(sweep=1 << 64),
               dict(features=[0], out={0: torch.empty(99, dtype=torch.float32, device=dev)}),
               dict(features=[0], out={0: torch.empty(100, dtype=torch.int32, device=dev)}),
               dict(features=[0], out={0: torch.empty(100, dtype=torch.float32)})):
        with pytest.raises(ValueError):
            ens.sample_predictive(view, **kw)
    with pytest.raises(common_amd._lib.MicroscopesHipError):
        ens.sample_predictive(view, features=[2])                         # (the noop column)
    vals, chains, groups = ens.sample_predictive(view, features=[0, 1], nrows=0)
    assert chains.numel() == 0 and groups.numel() == 0 and all(t.numel() == 0 for t in vals.values())


def test_members_whose_count_tables_differ_are_refused(gpu_ctx):
    twin = M.build_twin([(orc.GP, 0), (orc.NICH, 0)], 8, 3, P.N_TRAIN, 100, seed=2)
    c = M.EnsembleCase(gpu_ctx, twin)
    out = sentinels(c, 100)
    c.ens.states[2].set_col_bounds([int(twin.held[0]["values"].max()) + 40])
    with pytest.raises(common_amd._lib.MicroscopesHipError) as err:
        c.ens.sample_predictive(c.view, out=out)
    assert "state 2" in str(err.value) and "feature 0" in str(err.value)
    torch.cuda.synchronize()
    assert bool((bits(out[0]) == SENTINEL).all()) and bool((out[1] == SENTINEL).all())       # (gp as int32, nich float)
    c.ens.states[2].set_col_bounds(None)
    _, chains, _ = c.ens.sample_predictive(c.view, out=out)
    assert bool((chains >= 0).all())


def test_faster_than_the_loop_over_the_states(gpu_ctx):
    """128 chains, one nich column, K = 64, 2048 held-out rows with half the entries masked: one ens.impute against what
    callers had -- 128 State.predictive_logp calls and torch.multinomial on the stacked softmax, then 128
    State.impute(z=None) calls and a torch.where by chosen chain.  Medians of 7 device-synchronised wall times each,
    warmed up; the only bar is faster."""
    nchains, K, n = 128, 64, 2048
    rng = np.random.default_rng(6)
    train, held = make_feature(orc.NICH, 1000, K, rng), make_feature(orc.NICH, n, K, rng)
    view_t = common_amd.DataView.from_recarray(gpu_ctx, recarray_of([train]))
    mask = np.zeros(n, dtype=[("f0", np.bool_)])
    mask["f0"] = rng.random(n) < 0.5
    view_h = common_amd.DataView.from_recarray(gpu_ctx, np.ma.masked_array(recarray_of([held]), mask=mask))
    ens = common_amd.ChainEnsemble(gpu_ctx, P.NICH1, K, nchains, hps=[train["hp"]])
    ens.assign(view_t, torch.from_numpy(rng.integers(0, K, (nchains, 1000)).astype(np.int32)))
    lw = torch.full((nchains, 1), -float(np.log(nchains)), dtype=torch.float32, device=gpu_ctx.torch_device)

    def fused():
        return ens.impute(view_h, seed=3)[0][0]

    def loop():
        logp = torch.stack([st.predictive_logp(view_h) for st in ens.states]) + lw
        chosen = torch.multinomial(torch.softmax(logp, dim=0).T, 1)[:, 0]
        out = torch.zeros(n, dtype=torch.float32, device=gpu_ctx.torch_device)
        for ch, st in enumerate(ens.states):
            out = torch.where(chosen == ch, st.impute(view_h, seed=3)[0][0], out)
        return out

    def median_ms(fn, reps=7):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))
    t_fused, t_loop = median_ms(fused), median_ms(loop)
    print("128 chains x 2048 rows, nich K = 64: ens.impute %.3f ms, the loop over the states %.3f ms (x %.1f)"
          % (t_fused, t_loop, t_loop / t_fused))
    seen = torch.from_numpy(~mask["f0"]).to(gpu_ctx.torch_device)
    assert torch.equal(fused()[seen], loop()[seen])                      # (both copy the observed entries)
    assert t_fused < t_loop, (t_fused, t_loop)
