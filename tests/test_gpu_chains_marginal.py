"""The posterior-averaged row predictive density over a chain ensemble on the device (msc_chains_score_marginal,
ChainEnsemble.predictive_logp) against the double twin of every chain and scipy's weighted logsumexp over them.  Every
chain holds its own assignment, hyper-parameters and alpha; the held-out rows are drawn apart from the training rows.
The gates are derived in tests/chains_marginal_helpers.py: gate_c = E_{r,c} + 1e-6 max(1, |want_c|) for a chain's row,
max_c gate_c + 1e-6 max(1, |want_mix|) for mix."""
import os
import re
import time

import numpy as np
import pytest
import torch
from scipy.special import logsumexp

import common_amd
from oracle import oracle as orc
from tests import chains_marginal_helpers as M
from tests import smc_helpers as H
from tests.gpu_helpers import audit, make_feature, recarray_of

pytestmark = pytest.mark.gpu

NICH1 = [(orc.NICH, 0)]
MIX = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 5), (orc.NICH, 0)]
WIDE = [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 33), (orc.NICH, 0), (M.NOOP, 0)]
N_TRAIN = 400


def full_and_empty(K):
    """one chain with every slot full beside one chain with no row assigned (the prior predictive)"""
    return [np.arange(N_TRAIN) % K, np.full(N_TRAIN, -1)]


# name: (specs, K, chains, held-out rows, build_twin's keywords) -- what each shape is there for is in the issue's words
CASES = {
    "nich_k40": (NICH1, 40, 3, 700, {}),                    # K no multiple of a batch or 64, rows no multiple of the block
    "nich_k1000": (NICH1, 1000, 2, 300, {}),                # many group tiles
    "mix_k64_masked": (MIX, 64, 5, 2000, dict(used=60, masked=(0, 1, 2, 3))),
    "wide_k300_big_counts": (WIDE, 300, 3, 513, dict(used=290, big_counts=True)),   # the beyond-the-table forms
    "bb40_k16": ([(orc.BB, 0)] * 40, 16, 2, 257, {}),       # more features than a lane can keep
    # tables too tall for one tile: the third dd column's stay in global memory (the plan stages the nich column after it)
    "dd120x3_k40": ([(orc.DD, 120)] * 3 + NICH1, 40, 2, 130, {}),
    "k1": (MIX, 1, 1, 1, {}),
    "full_and_empty": (MIX, 24, 2, 300, dict(assignments=full_and_empty(24))),
    "nich_k8_70_chains": (NICH1, 8, 70, 65, {}),            # few rows: a slice a chain, 70 parts merged per row
    # several chains in a workgroup's slice, the last slice short (SEVERAL_A_SLICE below says how many on this device):
    # the chain loop, the tile staged again for the next chain, the (M, S) pair carried from chain to chain
    "nich_k8_71_chains_4100_rows": (NICH1, 8, 71, 4100, {}),
    "mix_k16_9_chains_33000_rows": (MIX, 16, 9, 33000, dict(used=14, masked=(1, 3))),
}
SEVERAL_A_SLICE = ["nich_k8_71_chains_4100_rows", "mix_k16_9_chains_33000_rows"]
_cache = {}


def slice_cut(nchains, view_rows):
    """(chains a slice, slices) of a call: route_chains_marginal (common_amd/csrc/route_calls.hpp, held to its rule by
    tests/cxx/test_route_calls.cpp) and the launcher's cut, restated for the device the suite runs on -- a view below four
    workgroups of 256 rows a compute unit is filled up with slices, at most one a chain"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks, want = max(1, -(-view_rows // 256)), 4 * max(1, cus)
    slices = 1 if blocks >= want else min(nchains, 1024, -(-want // blocks))
    per = -(-nchains // slices)
    return per, -(-nchains // per)


@pytest.mark.parametrize("name", SEVERAL_A_SLICE)
def test_these_shapes_put_several_chains_in_a_slice_and_leave_the_last_one_short(gpu_ctx, name):
    """what the shapes are there for holds on the device the suite runs on (256 compute units: 2 chains a slice, 36 and 5
    slices, the last with one chain)"""
    _, _, nchains, nheld, _ = CASES[name]
    per, slices = slice_cut(nchains, nheld)
    assert per >= 2 and slices >= 2 and nchains % per != 0, (per, slices)


def case(ctx, name):
    """the twin is computed once per case and shared; the device side is built for each test"""
    specs, K, nchains, nheld, kw = CASES[name]
    if name not in _cache:
        twin = M.build_twin(specs, K, nchains, N_TRAIN, nheld, seed=sum(map(ord, name)), **kw)
        rows = np.arange(nheld)
        _cache[name] = (twin, twin.all_chains(rows))
    twin, (want, gate) = _cache[name]
    return M.EnsembleCase(ctx, twin), want, gate


def weights_with_a_hole(nchains, seed):
    """random finite log weights, one of them -inf (none with a single chain)"""
    rng = np.random.default_rng(seed)
    logw = rng.uniform(-6.0, 3.0, nchains)
    if nchains > 1:
        logw[int(rng.integers(nchains))] = -np.inf
    return logw


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_rows_and_mix_against_the_twin(gpu_ctx, name):
    c, want, gate = case(gpu_ctx, name)
    nchains = c.twin.nchains
    for tag, logw in (("equal", None), ("weighted", weights_with_a_hole(nchains, 7))):
        mix, per = c.ens.predictive_logp(c.view, weights=logw, per_chain=True)
        alone = c.ens.predictive_logp(c.view, weights=logw)
        torch.cuda.synchronize()
        mix, per, alone = mix.cpu().numpy().astype(np.float64), per.cpu().numpy().astype(np.float64), alone.cpu().numpy()
        r_chain = float(np.max(np.abs(per - want) / gate))
        want_mix, gate_mix = c.twin.mix(want, gate, logw)
        r_mix = float(np.max(np.abs(mix - want_mix) / gate_mix))
        print("%s %s: max |chain_logp - want| / gate = %.3f, max |mix - want| / gate = %.3f" % (name, tag, r_chain, r_mix))
        audit("chains_marginal_chain_" + name, r_chain, 1.0)
        audit("chains_marginal_mix_%s_%s" % (tag, name), r_mix, 1.0)
        assert np.array_equal(alone, mix.astype(np.float32))          # (with or without the per-chain output)


@pytest.mark.parametrize("name", ["mix_k64_masked", "nich_k8_70_chains", "wide_k300_big_counts"] + SEVERAL_A_SLICE)
def test_one_hot_weights_give_the_chains_row_bit_for_bit(gpu_ctx, name):
    c, _, _ = case(gpu_ctx, name)
    n = c.twin.nchains
    for pick in sorted({0, 1, n // 2, n - 1}):            # (0 and 1: both places of a two-chain slice; n - 1: the last slice)
        logw = np.full(n, -np.inf)
        logw[pick] = -2.75
        mix, per = c.ens.predictive_logp(c.view, weights=logw, per_chain=True)
        assert torch.equal(mix, per[pick]), (name, pick)


@pytest.mark.parametrize("name", ["mix_k64_masked", "nich_k8_70_chains", "nich_k1000"] + SEVERAL_A_SLICE)
def test_row_ranges_give_the_whole_calls_bits_and_a_call_repeats_them(gpu_ctx, name):
    c, _, _ = case(gpu_ctx, name)
    n = int(c.view.nrows)
    logw = weights_with_a_hole(c.twin.nchains, 3)
    whole = [a.clone() for a in c.ens.predictive_logp(c.view, weights=logw, per_chain=True)]
    again = c.ens.predictive_logp(c.view, weights=logw, per_chain=True)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
    cuts = sorted({0, 1, min(n, 33), n // 3 + 7, n})
    for a, b in zip(cuts[:-1], cuts[1:]):
        mix, per = c.ens.predictive_logp(c.view, weights=logw, per_chain=True, row0=a, nrows=b - a)
        assert torch.equal(whole[0][a:b], mix) and torch.equal(whole[1][:, a:b], per), (name, a, b)


def test_features_and_given_are_the_restricted_and_the_conditional_density(gpu_ctx):
    """features= is the twin over those features alone.  given= the others is the model-averaged conditional density of a
    dd(5) label: over the label's five values it sums to one.  Each cond_v is within err_v = gate_mix(all, v) +
    gate_mix(given) of the truth and sum_v exp(cond_v) = 1 there, so the sum moves by at most sum_v exp(cond_v) (e^err_v
    - 1) <= 1.01 max_v err_v (err_v ~ 1e-5) -- inside the sum of the five values' gates."""
    specs = [(orc.DD, 5), (orc.BB, 0), (orc.GP, 0), (orc.NICH, 0)]
    twin = M.build_twin(specs, 24, 4, N_TRAIN, 600, seed=41, used=20)
    c = M.EnsembleCase(gpu_ctx, twin)
    rows, others = np.arange(600), [1, 2, 3]
    logw = weights_with_a_hole(4, 5)
    for feats in ([0], [1, 3], [0, 2, 3]):
        want, gate = twin.all_chains(rows, feats=feats)
        want_mix, gate_mix = twin.mix(want, gate, logw)
        mix, per = c.ens.predictive_logp(c.view, weights=logw, features=feats, per_chain=True)
        audit("chains_marginal_features_chain", np.max(np.abs(per.cpu().numpy() - want) / gate), 1.0)
        audit("chains_marginal_features_mix", np.max(np.abs(mix.cpu().numpy() - want_mix) / gate_mix), 1.0)
    w_sub, g_sub = twin.all_chains(rows, feats=others)
    wm_sub, gm_sub = twin.mix(w_sub, g_sub, logw)
    total, err = np.zeros(600), np.zeros(600)
    for v in range(5):
        twin.held[0]["values"] = np.full(600, v, dtype=np.int32)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(twin.held))
        w_all, g_all = twin.all_chains(rows)
        wm_all, gm_all = twin.mix(w_all, g_all, logw)
        cond = c.ens.predictive_logp(view, weights=logw, given=others).cpu().numpy().astype(np.float64)
        audit("chains_marginal_given", np.max(np.abs(cond - (wm_all - wm_sub)) / (gm_all + gm_sub)), 1.0)
        total += np.exp(cond)
        err = np.maximum(err, gm_all + gm_sub)
    audit("chains_marginal_given_sums_to_one", np.max(np.abs(total - 1.0) / (1.01 * err)), 1.0)


@pytest.mark.parametrize("name", ["bb", "nich"])
def test_the_partitions_of_five_rows_average_to_the_exact_predictive_of_the_sixth(gpu_ctx, name):
    """52 chains, one per set partition of five rows, weighted by the partitions' exact posterior: mix of the sixth row is
    log p(x_1..6) - log p(x_1..5) from the enumeration over set partitions -- a route that shares no code with the
    kernel.  Bound: max_c gate_c + 1e-6 max(1, |want|), plus the enumeration's own float64 rounding (sums of 52 and 203
    terms: < 1e-13) and the 1.3e-8 by which the float suff-stats the device holds move the answer
    (tests/test_chains_marginal_cpu.py has the identity itself to 1e-10): 2e-8 for both."""
    twin, logw, exact = M.partition_twin(H.six_row_datasets()[name][0], 1.0)
    c = M.EnsembleCase(gpu_ctx, twin)
    _, gate = twin.all_chains(np.arange(1))
    got = float(c.ens.predictive_logp(c.view, weights=logw).cpu().numpy()[0])
    bound = float(gate.max()) + 1e-6 * max(1.0, abs(exact)) + 2e-8
    print("partitions %s: mix %.9f, exact %.9f, |diff| / bound = %.3f" % (name, got, exact, abs(got - exact) / bound))
    audit("chains_marginal_partitions_" + name, abs(got - exact) / bound, 1.0)
    # the same weights on the device
    got_dev = c.ens.predictive_logp(c.view, weights=torch.from_numpy(logw).to(gpu_ctx.torch_device))
    assert float(got_dev.cpu().numpy()[0]) == got


SWEEP_SPECS = [(orc.BB, 0), (orc.GP, 0), (orc.NICH, 0)]


def seated(gpu_ctx, seed=31):
    feats, _, view = H.data(gpu_ctx, SWEEP_SPECS, 120, 8, seed)
    ens = H.ensemble(gpu_ctx, feats, 8, 6, alpha=1.25)
    ens.seat(view, seed=17)
    return ens, view


def test_the_ensemble_is_read_only(gpu_ctx):
    """the bits of every member (and z, logw) are the same before and after, and a sweep on the training view that
    follows gives the z and the tables it gives without the call -- the held-out view's gp column reaches further than
    the training view's, so the members' count tables are rebuilt for it and again for the sweep"""
    held_feats = [make_feature(f, 77, 6, np.random.default_rng(8), d) for f, d in SWEEP_SPECS]
    held_feats[1]["values"] = (held_feats[1]["values"] + 40).astype(np.uint32)
    held = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(held_feats))
    ens, view = seated(gpu_ctx)
    before = H.ensemble_bits(ens)
    ens.predictive_logp(held, per_chain=True)
    ens.predictive_logp(held, weights=np.log(np.arange(1.0, 7.0)), features=[1, 2], given=[2])
    assert H.ensemble_bits(ens) == before
    ens.sweep(view, 2, seed=9, sweep=1)
    torch.cuda.synchronize()
    with_call = H.ensemble_bits(ens)
    plain, view2 = seated(gpu_ctx)
    plain.sweep(view2, 2, seed=9, sweep=1)
    torch.cuda.synchronize()
    assert H.ensemble_bits(plain) == with_call


def test_the_particle_filters_weights_go_straight_in(gpu_ctx):
    """after ens.smc the weighted particles predict: mix equals numpy's logsumexp of the per-chain rows plus the
    normalised log weights.  The per-chain rows are the device's own L rounded to float (each moves by <= 2^-24 |L_c|,
    and a chain far below the mix carries no weight), mix is rounded once more, the weights are normalised in double on
    both sides: within 1e-6 max(1, |want|), the reduction's share of the mix gate."""
    feats, _, view = H.data(gpu_ctx, H.C3_SMALL, 48, 8, 77)
    ens = H.ensemble(gpu_ctx, feats, 8, 16)
    res = ens.smc(view, seed=5)
    assert np.isfinite(res.log_evidence)
    _, _, held = H.data(gpu_ctx, H.C3_SMALL, 90, 8, 78)
    mix, per = ens.predictive_logp(held, weights=ens.logw, per_chain=True)
    logw = ens.logw.cpu().numpy()
    want = logsumexp(per.cpu().numpy().astype(np.float64) + M.normalised(logw, 16)[:, None], axis=0)
    audit("chains_marginal_smc_handover", np.max(np.abs(mix.cpu().numpy() - want) / (1e-6 * np.maximum(1.0, np.abs(want)))), 1.0)
    assert bool(torch.isfinite(mix).all())


def test_no_finite_weight_is_nan_and_the_chain_rows_stay(gpu_ctx):
    c, want, gate = case(gpu_ctx, "nich_k40")
    mix, per = c.ens.predictive_logp(c.view, weights=np.full(3, -np.inf), per_chain=True)
    assert bool(torch.isnan(mix).all())
    assert np.all(np.abs(per.cpu().numpy() - want) <= gate)


def test_bad_arguments(gpu_ctx):
    twin = M.build_twin([(orc.NICH, 0), (orc.BB, 0)], 8, 3, N_TRAIN, 100, seed=1)
    c = M.EnsembleCase(gpu_ctx, twin)
    dev, lib, ens, view = gpu_ctx.torch_device, gpu_ctx.lib, c.ens, c.view
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "microscopes_hip.h")) as fh:
        einval = int(re.search(r"MSC_EINVAL\s*=\s*(-?\d+)", fh.read()).group(1))
    mix = torch.full((100,), 7.0, dtype=torch.float32, device=dev)
    per = torch.full((3, 100), 7.0, dtype=torch.float32, device=dev)
    u32 = lambda *v: (common_amd._lib.C.c_uint32 * len(v))(*v)          # noqa: E731

    def call(h=ens._h, v=view._h, cols=None, row0=0, nrows=100, feats=None, nf=0, flags=0, m=mix.data_ptr(),
             p=per.data_ptr(), ld=100):
        return lib.msc_chains_score_marginal(h, v, cols, row0, nrows, feats, nf, None, flags, m, p, ld)
    def refused(rc):
        """MSC_EINVAL, and neither output touched"""
        assert rc == einval, rc
        torch.cuda.synchronize()
        assert bool((mix == 7.0).all()) and bool((per == 7.0).all())
    refused(call(h=None))                                                 # null arguments
    refused(call(v=None))
    refused(call(m=None, p=None))                                         # both outputs null
    refused(call(ld=99))                                                  # ld_logp < nrows with a per-chain output
    refused(call(feats=u32(1, 0), nf=2))                                  # not ascending
    refused(call(feats=u32(0, 0), nf=2))                                  # ... not strictly
    refused(call(feats=u32(0, 2), nf=2))                                  # outside the state
    refused(call(row0=50, nrows=51, ld=100))                              # rows outside the view
    rec3 = np.zeros(100, dtype=[("f0", np.float32), ("f1", np.bool_), ("f2", np.float32, (3,))])
    view3 = common_amd.DataView.from_recarray(gpu_ctx, rec3)
    refused(call(v=view3._h, cols=u32(2, 1)))                             # three elements a value do not fit the nich feature
    refused(call(cols=u32(0, 9)))                                         # a column outside the view
    refused(call(flags=1))
    zt = torch.zeros(100, dtype=torch.int32, device=dev)                  # member 1 between step_begin and commit_reduce
    ens.states[1].sweep_step_begin(view, zt, seed=3, sweep=0)
    refused(call())
    assert "state 1" in lib.msc_last_error().decode()                    # (the member is named)
    ens.states[1].commit_reduce()
    assert call(v=view3._h) == 0                                          # (that view's first two columns do fit)
    assert call(p=None, ld=0) == 0 and call(m=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mix).all()) and bool(torch.isfinite(per).all())
    # the binding's own checks come before any device call
    for kw in (dict(weights=np.zeros(3, dtype=np.float32)), dict(weights=np.zeros(4)), dict(features=[2]), dict(features=[]),
               dict(features=[0, 0]), dict(features=[0], given=[1]), dict(given=[5]), dict(row0=-1), dict(row0=50, nrows=51),
               dict(out=torch.empty(99, dtype=torch.float32, device=dev))):
        with pytest.raises(ValueError):
            ens.predictive_logp(view, **kw)
    assert ens.predictive_logp(view, nrows=0).numel() == 0


def test_members_whose_count_tables_differ_are_refused(gpu_ctx):
    """one tile plan serves every chain: a member whose own column bounds give its gp table other rows than member 0's
    is MSC_EINVAL, named, with nothing written; with the bounds gone the call runs"""
    twin = M.build_twin([(orc.GP, 0), (orc.NICH, 0)], 8, 3, N_TRAIN, 100, seed=2)
    c = M.EnsembleCase(gpu_ctx, twin)
    out = torch.full((100,), 7.0, dtype=torch.float32, device=gpu_ctx.torch_device)
    c.ens.states[2].set_col_bounds([int(twin.held[0]["values"].max()) + 40])
    with pytest.raises(common_amd._lib.MicroscopesHipError) as err:
        c.ens.predictive_logp(c.view, out=out)
    assert "state 2" in str(err.value) and "feature 0" in str(err.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    c.ens.states[2].set_col_bounds(None)
    want, gate = twin.all_chains(np.arange(100))
    want_mix, gate_mix = twin.mix(want, gate)
    assert np.all(np.abs(c.ens.predictive_logp(c.view, out=out).cpu().numpy() - want_mix) <= gate_mix)


def test_faster_than_the_loop_over_the_states(gpu_ctx):
    """128 chains, one nich column, K = 64, 2048 held-out rows: one ens.predictive_logp against what callers had -- 128
    State.predictive_logp calls, a stack and torch.logsumexp.  Medians of 7 device-synchronised wall times each, warmed
    up; the only bar is faster."""
    nchains, K, n = 128, 64, 2048
    rng = np.random.default_rng(6)
    train, held = make_feature(orc.NICH, 1000, K, rng), make_feature(orc.NICH, n, K, rng)
    view_t = common_amd.DataView.from_recarray(gpu_ctx, recarray_of([train]))
    view_h = common_amd.DataView.from_recarray(gpu_ctx, recarray_of([held]))
    ens = common_amd.ChainEnsemble(gpu_ctx, NICH1, K, nchains, hps=[train["hp"]])
    ens.assign(view_t, torch.from_numpy(rng.integers(0, K, (nchains, 1000)).astype(np.int32)))
    lw = torch.full((nchains, 1), -float(np.log(nchains)), dtype=torch.float32, device=gpu_ctx.torch_device)
    out = torch.empty(n, dtype=torch.float32, device=gpu_ctx.torch_device)

    def fused():
        return ens.predictive_logp(view_h, out=out)

    def loop():
        return torch.logsumexp(torch.stack([st.predictive_logp(view_h) for st in ens.states]) + lw, dim=0)

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
    print("128 chains x 2048 rows, nich K = 64: ens.predictive_logp %.3f ms, the loop over the states %.3f ms (x %.1f)"
          % (t_fused, t_loop, t_loop / t_fused))
    # both routes answer the same question (each side within a gate of the truth: 1e-4 is far outside both)
    assert float((fused() - loop()).abs().max()) < 1e-4 * float(loop().abs().max().clamp(min=1.0))
    assert t_fused < t_loop, (t_fused, t_loop)
