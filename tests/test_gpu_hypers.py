"""GPU: every place of the device code that READS a hyperparameter block, under blocks that tell its fields apart.

The parity tests elsewhere run on make_feature's defaults -- alpha = beta = 1, alphas all one, mu = 0 with kappa = sigmasq
= nu = 1, psi = I -- under which swapped fields, a rotated alphas index, a sign error on mu, a dropped kappa mu mu^T or
nu sigmasq or ln det psi term, and one feature reading another's block all pass.  Hyperparameters enter device code in
few places (prepare_group's plain and leave-one-out tables, k_dm_prepare, the own-group terms of the leave-one-out, sweep
and marginal kernels, k_gp_large_fix, k_niw_prepare / k_niw_score_data, k_score_data, the predictive prepare kernels, the
sequential sweep beyond its tables, the host's packing of the blocks); after them the tile, role-split, lane-row and
fused kernels read prepared tables only.  So: one test per consumer at the smallest shape that reaches it, on
gpu_helpers.distinct_hp (tests/test_hypers_cpu.py shows on the twin alone that these values discriminate), against the
oracle's double twin under the standing gates: TOL for one feature, TOL * sum_f max(1, |score_f|) for a sum of features
(test_gpu_fuzz.py's).  The scoring, score_data, beyond-the-tables and sequential tests run on edge_assignment's state (an
empty group, a singleton, an unassigned row); the sweep cases keep test_gpu_sweep._run's assignment (two empty groups)
and the marginal case test_gpu_marginal.Case's (empty groups, a singleton, unassigned rows in the leave-one-out call),
so that their checks are exactly the ones those files make."""
import numpy as np
import pytest
import torch
from scipy import stats

import common_amd
from oracle import oracle as orc
from tests.gpu_helpers import (MIXED, TOL, audit, crp_prior_matrix, distinct_hp, edge_assignment, load_state, make_feature,
                               recarray_of, rel_err, state_from_assignment)
from tests.test_gpu_marginal import Case, check_case
from tests.test_gpu_predictive import (P_GATE, check_replay, draws_of_group, entry_u24, group_state, inverse_cdf,
                                       pooled_chi2)
from tests.test_gpu_sequential import _run_and_replay
from tests.test_gpu_sweep import _check_agreement, _run, nich1_kernel  # noqa: F401  (nich1_kernel: a fixture)

pytestmark = pytest.mark.gpu

N, K, ALPHA = 256, 8, 1.7
SINGLE = [(orc.BB, 0), (orc.BBNC, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 5), (orc.DD, 128), (orc.DM, 4), (orc.NICH, 0),
          (orc.NIW, 3), (orc.NIW, 20), (orc.NIW, 40), (orc.NIW, 100)]


def _name(spec):
    return "%s%s" % (orc.FAMILY_NAMES[spec[0]], spec[1] or "")


def mixed_hp(j, family, dim, shared_nu=False):
    """feature j of a state on distinct_hp(.., i=j); shared_nu: the second nich feature (j = 7) takes the first's nu and
    keeps its own mu, kappa and sigmasq -- the two then share a c1 block (abi.cpp groups nich features by nu)"""
    hp = distinct_hp(family, dim, j)
    if shared_nu and family == orc.NICH and j == 7:
        hp["nu"] = distinct_hp(orc.NICH, 0, 6)["nu"]
    return hp


def _features(specs, n, k, rng, hp_of, small_dm=False):
    feats = [make_feature(f, n, k, rng, d, hp=hp_of(j, f, d)) for j, (f, d) in enumerate(specs)]
    if small_dm:      # (row totals of at most ~10: the dm tables are staged whole, what the lane <-> row kernel needs)
        feats = [dict(f, values=(f["values"] // 5).astype(np.int32)) if f["family"] == orc.DM else f for f in feats]
    return feats


def _state(gpu_ctx, feats, k, z, alpha=ALPHA):
    fs = state_from_assignment(feats, k, z)
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], k)
    load_state(st, fs)
    counts = np.bincount(z[z >= 0], minlength=k)
    st.set_group_counts(counts.astype(np.uint32))
    st.set_alpha(alpha)
    return fs, view, st, counts


def _twin(feats, fs, z=None):
    """-> (sum over the features, sum_f max(1, |score_f|)) of the double twin"""
    parts = [F.score_matrix(ss64, f["values"], z) for f, (F, ss64, _) in zip(feats, fs)]
    return sum(parts), sum(np.maximum(1.0, np.abs(p)) for p in parts)


def _check(name, got, want, mag=None):
    """print the figure, then hold it to the gate: TOL on rel_err for one feature, TOL on |got - want| / max(sum_f
    max(1, |score_f|), |want|) for a sum (mag given)"""
    got = np.asarray(got, dtype=np.float64)
    err = rel_err(got, want) if mag is None else np.abs(got - want) / np.maximum(mag, np.abs(want))
    worst = float(np.nanmax(np.where(np.isfinite(err), err, np.inf))) if err.size else 0.0
    print("%s: max err %.3g (gate %.1g)" % (name, worst, TOL))
    if mag is None:
        assert worst <= TOL, (name, worst)
    else:
        audit("hypers." + name, worst, TOL)


def _check_all_outputs(gpu_ctx, name, feats, k, z, single):
    """plain, leave-one-out, leave-one-out + prior, score_data of every group -- against the twin"""
    fs, view, st, counts = _state(gpu_ctx, feats, k, z)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    want, mag = _twin(feats, fs)
    _check(name + ".plain", st.score_value(view).cpu().numpy(), want, None if single else mag)
    want, mag = _twin(feats, fs, z)
    _check(name + ".loo", st.score_value(view, z=zt).cpu().numpy(), want, None if single else mag)
    _check(name + ".loo_prior", st.score_value(view, z=zt, crp_prior=True).cpu().numpy(),
           want + crp_prior_matrix(counts, ALPHA, z), None if single else mag)
    sd = st.score_data().cpu().numpy()
    for i, (F, ss64, _) in enumerate(fs):
        _check("%s.score_data" % name, sd[i], F.score_data_all(ss64))
    return st, view


@pytest.mark.parametrize("spec", SINGLE, ids=_name)
def test_single_feature_scores_and_score_data(gpu_ctx, spec):
    """prepare_group's tables and leave-one-out tables (bb, gp, bnb, dd, nich), k_dm_prepare, k_niw_prepare with a dense
    psi and mu != 0 (dimensions 3, 20, 40, 100: the register kernel, the one- and two-block f64 kernels, the wide one),
    k_score_data / k_niw_score_data (bbnc's prior part, niw's 0.5 nu ln det psi)"""
    fam, dim = spec
    rng = np.random.default_rng(4000 + 10 * fam + dim)
    feats = _features([spec], N, K, rng, lambda j, f, d: distinct_hp(f, d))
    _check_all_outputs(gpu_ctx, _name(spec), feats, K, edge_assignment(N, K, rng), single=True)


@pytest.mark.parametrize("k", [8, 300])
@pytest.mark.parametrize("shared_nu", [False, True], ids=["nu_all_different", "two_nich_share_nu"])
def test_several_features_each_on_its_own_block(gpu_ctx, shared_nu, k):
    """the offsets into the state's packed hyperparameter buffer (a feature reading its neighbour's block moves its scores
    far beyond the gate: test_hypers_cpu.py) and the host's grouping of nich features into blocks by nu"""
    n = 300
    rng = np.random.default_rng(50 + k)
    feats = _features(MIXED, n, k, rng, lambda j, f, d: mixed_hp(j, f, d, shared_nu))
    _check_all_outputs(gpu_ctx, "mixed_k%d%s" % (k, "_shared_nu" if shared_nu else ""), feats, k, edge_assignment(n, k, rng),
                       single=False)


def test_several_features_on_the_lane_row_kernel(gpu_ctx, monkeypatch):
    """the same state on k_score_tail_rows (512 rows, 40 groups, the kernel forced from 256 rows on; dm counts small enough
    for its staged tables).  The niw feature has a kernel of its own that runs after the scalar pass and is the last one
    named, so the kernel's name is asserted on the list without it and the whole list is checked as well."""
    monkeypatch.setenv("MSC_TAIL_MIN_ROWS", "256")
    n, k = 512, 40
    for specs in (MIXED[:-1], MIXED):
        rng = np.random.default_rng(77)
        feats = _features(specs, n, k, rng, lambda j, f, d: mixed_hp(j, f, d), small_dm=True)
        st, view = _check_all_outputs(gpu_ctx, "mixed_lane_row_%d" % len(specs), feats, k, edge_assignment(n, k, rng), single=False)
        if specs is not MIXED:
            st.score_value(view)
            assert gpu_ctx.last_kernel("score").startswith("k_score_tail_rows<"), gpu_ctx.last_kernel("score")


PLANTED = [0, 31, 32, 1000, 65535]


@pytest.mark.parametrize("fam", [orc.GP, orc.BNB, orc.DM], ids=["gp", "bnb", "dm"])
def test_counts_beyond_the_tables(gpu_ctx, fam):
    """k_gp_large_fix and the HEAVY own-group branches (gp_loo, bnb_score, dm_score_direct): values at and beyond the
    exact tables' ends -- in ordinary groups, in the singleton (row 3) and on the unassigned row (row 5)"""
    dim = 4 if fam == orc.DM else 0
    rng = np.random.default_rng(600 + fam)
    f = _features([(fam, dim)], N, K, rng, lambda j, ff, d: distinct_hp(ff, d))[0]
    if fam == orc.DM:
        f["values"][[0, 3, 5], 2] += np.array([1024, 3000, 70000], dtype=np.int32)      # the category's count and the total
        f["values"][1, 0] += 600                                                     # the total alone
        f["values"][1, 1] += 600
        assert (f["values"][[0, 1, 3, 5]].sum(1) >= 1024).all()
    else:
        f["values"][[0, 1, 2, 4, 6]] = np.array(PLANTED, dtype=np.uint32)
        f["values"][3], f["values"][5] = 1000, 65535
    z = edge_assignment(N, K, rng)
    fs, view, st, _ = _state(gpu_ctx, [f], K, z)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    name = "beyond_tables_" + orc.FAMILY_NAMES[fam]
    _check(name + ".plain", st.score_value(view).cpu().numpy(), _twin([f], fs)[0])
    _check(name + ".loo", st.score_value(view, z=zt).cpu().numpy(), _twin([f], fs, z)[0])


def _sweep_case(gpu_ctx, specs, n, k, seed, hp_of):
    got, want, scores, _ = _run(gpu_ctx, specs, n, k, seed=seed, sweep_idx=2, hp_of=hp_of)
    print("sweep %s K=%d: agreement %.4f" % ([_name(s) for s in specs], k, (got == want).mean()))
    _check_agreement(got, want, scores, seed, 2, 0.98)


@pytest.mark.parametrize("k", [7, 300])
def test_sweep_single_nich(gpu_ctx, k, nich1_kernel):  # noqa: F811
    """the own-group term of k_sweep_nich1 / k_sweep_nich1_t reads the block itself (nich_loo_core)"""
    _sweep_case(gpu_ctx, [(orc.NICH, 0)], 1000, k, 800 + k, lambda j, f, d: distinct_hp(f, d))


@pytest.mark.parametrize("k", [40, 300])
def test_sweep_mixed_features(gpu_ctx, k):
    """the own-group term of the tile sweep kernels (K <= 256) and of the materialising path beyond, a block per feature"""
    _sweep_case(gpu_ctx, MIXED[:-1], 1000, k, 820 + k, mixed_hp)


@pytest.mark.parametrize("dim,k", [(3, 5), (20, 12)])
def test_sweep_niw(gpu_ctx, dim, k):
    """niw 3 at five groups: the fused small-niw sweep; niw 20: k_niw_prepare's tables under the materialising sweep"""
    _sweep_case(gpu_ctx, [(orc.NIW, dim)], 1000, k, 840 + dim, lambda j, f, d: distinct_hp(f, d))


def test_marginal_with_z(gpu_ctx):
    """msc_score_marginal's own-group term (kernels_marginal.hip) on the mixed list, 40 groups, leave-one-out"""
    c = Case(gpu_ctx, MIXED, 2000, 40, seed=31, alpha=ALPHA, used=36, hp_of=mixed_hp)
    check_case(c, "hypers_mixed")
    check_case(c, "hypers_mixed", z=c.loo_z())


def test_sequential_sweep_beyond_the_tables(gpu_ctx):
    """the sequential sweep evaluates counts beyond its tables from the block (gp_eval_large on hp[0], hp[1]; bnb_score):
    one replay of the chain in double, gp and bnb columns holding such counts"""
    n, k, alpha = 600, 12, 1.3
    rng = np.random.default_rng(93)
    specs = [(orc.GP, 0), (orc.BNB, 0), (orc.NICH, 0)]
    feats = _features(specs, n, k, rng, lambda j, f, d: distinct_hp(f, d, j))
    for f in feats[:2]:
        f["values"][::37] = rng.integers(1024, 3000, len(f["values"][::37])).astype(np.uint32)
    z = edge_assignment(n, k, rng)
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = common_amd.State(gpu_ctx, specs, k)
    Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
    for i, F in enumerate(Fs):
        st.set_hp(i, F.hp)
    st.set_alpha(alpha)
    st.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device))
    s = dict(view=view, st=st, z=z, alpha=alpha, K=k, N=n, rfeats=[(F, f["values"], None) for F, f in zip(Fs, feats)])
    _run_and_replay(gpu_ctx, s, seed=17, sweep=4)


NDRAW = 1 << 17


@pytest.mark.parametrize("spec", [(orc.GP, 0), (orc.BNB, 0), (orc.NICH, 0), (orc.NIW, 3)], ids=_name)
def test_predictive_of_a_populated_and_of_an_empty_group(gpu_ctx, spec):
    """k_pred_prepare / the niw predictive prepare: 2^17 draws from group 0 (posterior predictive) and from group 1, which
    holds no row (the PRIOR predictive: the block alone), against the closed forms"""
    fam, dim = spec
    h = distinct_hp(fam, dim)
    f, (F, ss64, _), st = group_state(gpu_ctx, fam, dim, 2, 6, 131 + fam, hp=h, empty=1)
    assert ss64["count"][0] == 6 and ss64["count"][1] == 0
    view = common_amd.DataView.from_recarray(gpu_ctx, np.zeros(NDRAW, dtype=[("f0", f["np_dtype"])]))
    for g in (0, 1):
        x = draws_of_group(gpu_ctx, st, view, g, NDRAW).astype(np.float64)
        cnt = float(ss64["count"][g])
        if fam == orc.GP:
            theta = 1.0 / (h["inv_beta"] + cnt)
            ps = [pooled_chi2(x, stats.nbinom(h["alpha"] + float(ss64["sum"][g]), 1.0 / (1.0 + theta)).pmf)]
        elif fam == orc.BNB:
            ps = [pooled_chi2(x, stats.betanbinom(h["r"], h["alpha"] + h["r"] * cnt, h["beta"] + float(ss64["sum"][g])).pmf)]
        elif fam == orc.NICH:
            mean, ctv = float(ss64["mean"][g]), float(ss64["count_times_variance"][g])
            kn, nun = h["kappa"] + cnt, h["nu"] + cnt
            mun = (h["kappa"] * h["mu"] + cnt * mean) / kn
            s2 = (h["nu"] * h["sigmasq"] + ctv + cnt * h["kappa"] * (h["mu"] - mean) ** 2 / kn) / nun
            ps = [stats.kstest(x, stats.t(nun, mun, np.sqrt(s2 * (kn + 1) / kn)).cdf).pvalue]
        else:
            sx, sxx = ss64["sum_x"][g].astype(np.float64), ss64["sum_xxT"][g].astype(np.float64).reshape(dim, dim)
            kn, nun = h["kappa"] + cnt, h["nu"] + cnt
            mun = (h["kappa"] * h["mu"] + sx) / kn
            psin = h["psi"] + sxx + h["kappa"] * np.outer(h["mu"], h["mu"]) - kn * np.outer(mun, mun)
            dof = nun - dim + 1
            sigma = psin * (kn + 1) / (kn * dof)
            a = np.random.default_rng(dim).normal(size=dim)
            ps = [stats.kstest(x[:, i], stats.t(dof, mun[i], np.sqrt(sigma[i, i])).cdf).pvalue for i in range(dim)]
            ps.append(stats.kstest(x @ a, stats.t(dof, a @ mun, np.sqrt(a @ sigma @ a)).cdf).pvalue)
        print("%s group %d (count %d): p = %s" % (_name(spec), g, cnt, ["%.3g" % p for p in ps]))
        for p in ps:
            audit("pred_gpu_hypers_p", -p, -P_GATE)


def test_one_uniform_draws_of_bb_and_dd_replay(gpu_ctx):
    """the one-uniform draws read the block as alpha + heads over alpha + beta + n and alphas[v] + counts[v]: replayed"""
    n, k, seed, sweep = 1024, 4, 11, 5
    rng = np.random.default_rng(3)
    feats = _features([(orc.BB, 0), (orc.DD, 7)], n, k, rng, lambda j, f, d: distinct_hp(f, d, j))
    z = rng.integers(0, k - 1, n).astype(np.int32)                  # the last group: empty, drawn from below
    fs, view, st, _ = _state(gpu_ctx, feats, k, z)
    zd = z.copy()
    zd[::5] = k - 1                                                 # a fifth of the rows draw from the empty group's prior
    out, groups = st.sample_predictive(view, z=torch.from_numpy(zd).to(gpu_ctx.torch_device), seed=seed, sweep=sweep)
    assert np.array_equal(groups.cpu().numpy(), zd)
    for i, (F, ss64, _) in enumerate(fs):
        u = np.array([entry_u24(seed, sweep, r, i) for r in range(n)])
        if F.family == orc.BB:
            a, b = feats[i]["hp"]["alpha"], feats[i]["hp"]["beta"]
            p1 = (a + ss64["heads"].astype(np.float64)) / (a + b + ss64["heads"] + ss64["tails"])
            probs = np.stack([1 - p1, p1], 1)
        else:
            probs = np.asarray(feats[i]["hp"]["alphas"], np.float64)[None, :] + ss64["counts"].astype(np.float64)
        want, near = inverse_cdf(probs[zd], u)
        check_replay("hypers_fam%d" % F.family, out[i].cpu().numpy().astype(np.int64), want, near)
