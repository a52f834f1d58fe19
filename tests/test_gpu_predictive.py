"""GPU: posterior predictive sampling (msc_sample_predictive / State.sample_predictive / State.impute).  The one-uniform
draws (bb, bbnc, dd, the group draw) are replayed exactly in numpy with the oracle's Philox words under the counter layout
the header documents; the rejection families are held to their predictive distributions with goodness-of-fit tests at
fixed seeds; imputation, reproducibility, the untouched state and the errors are checked directly."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

import common_amd
from common_amd import _lib as L
from oracle import oracle as orc
from tests.gpu_helpers import (audit, crp_prior_matrix, load_state, make_feature, oracle_scores, recarray_of,
                               state_from_assignment)

pytestmark = pytest.mark.gpu

P_GATE = 1e-4          # goodness of fit at a fixed seed: a correct sampler passes with room to spare
STEP_EPS = 1e-6        # a draw may differ from the replay only where its uniform lies this close to a CDF step (f32 rounding)


def setup(ctx, specs, N, K, seed, masked=None):
    rng = np.random.default_rng(seed)
    feats = [make_feature(fam, N, K, rng, dim=dim) for fam, dim in specs]
    z = rng.integers(0, K, N).astype(np.int32)
    fs = state_from_assignment(feats, K, z)
    st = common_amd.State(ctx, [(fam, dim) for fam, dim in specs], K)
    load_state(st, fs)
    st.set_group_counts(np.bincount(z, minlength=K).astype(np.uint32))
    st.set_alpha(1.3)
    arr = recarray_of(feats)
    if masked is not None:
        mask = np.zeros(N, dtype=[("f%d" % i, np.bool_, np.dtype(f["np_dtype"]).shape) for i, f in enumerate(feats)])
        for i, f in enumerate(feats):
            m = rng.random(N) < masked
            mask["f%d" % i] = m if np.dtype(f["np_dtype"]).shape == () else np.repeat(m[:, None], f["dim"], 1)
        arr = np.ma.masked_array(arr, mask=mask)
    view = common_amd.DataView.from_recarray(ctx, arr)
    return feats, fs, st, view, z, arr


def entry_u24(seed, sweep, row, feature):
    w = orc.philox([seed & 0xffffffff, seed >> 32],
                   [row & 0xffffffff, row >> 32, sweep & 0xffffffff, 0x80000000 | (feature & 0x7fff) << 16])
    return (int(w[0]) >> 8) / 16777216.0


def inverse_cdf(probs, u):
    """smallest v with u < CDF(v), and how close u lies to a step"""
    cdf = np.cumsum(probs, axis=1)
    cdf /= cdf[:, -1:]
    v = np.minimum((u[:, None] >= cdf).sum(1), probs.shape[1] - 1)
    near = np.abs(cdf - u[:, None]).min(1)
    return v, near


def check_replay(name, got, want, near):
    bad = got != want
    audit("pred_replay_mismatch_frac_" + name, bad.mean(), 1e-3)
    assert np.all(near[bad] < STEP_EPS), (name, near[bad])


def test_one_uniform_draws_replay_exactly(gpu_ctx):
    N, K, seed, sweep = 4096, 16, 11, 5
    feats, fs, st, view, z, _ = setup(gpu_ctx, [(orc.BB, 0), (orc.BBNC, 0), (orc.DD, 7)], N, K, 3)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    out, groups = st.sample_predictive(view, z=zt, seed=seed, sweep=sweep)
    assert np.array_equal(groups.cpu().numpy(), z)
    rows = np.arange(N)
    for f, (F, ss64, ss32) in enumerate(fs):
        u = np.array([entry_u24(seed, sweep, r, f) for r in rows])
        if F.family == orc.BB:
            a, b = feats[f]["hp"]["alpha"], feats[f]["hp"]["beta"]
            p1 = (a + ss64["heads"].astype(np.float64)) / (a + b + ss64["heads"] + ss64["tails"])
            probs = np.stack([1 - p1, p1], 1)
        elif F.family == orc.BBNC:
            p1 = ss32["p"].astype(np.float64)
            probs = np.stack([1 - p1, p1], 1)
        else:
            probs = np.asarray(feats[f]["hp"]["alphas"], np.float32).astype(np.float64)[None, :] + ss64["counts"].astype(np.float64)
        want, near = inverse_cdf(probs[z], u)
        got = out[f].cpu().numpy().astype(np.int64)
        check_replay("fam%d" % F.family, got, want, near)


def test_group_draw_is_the_sweeps_draw_of_an_unassigned_row_under_its_own_key(gpu_ctx):
    N, K, seed, sweep = 4096, 32, 21, 3
    feats, fs, st, view, z, _ = setup(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0), (orc.DD, 5)], N, K, 8)
    out, groups = st.sample_predictive(view, seed=seed, sweep=sweep)
    g = groups.cpu().numpy()
    assert g.min() >= 0 and g.max() < K
    scores = oracle_scores(feats, fs) + crp_prior_matrix(np.bincount(z, minlength=K), 1.3)
    probs = np.exp(scores - scores.max(1, keepdims=True))
    key = seed ^ L.PRED_GROUP_KEY
    u = np.array([orc.uniform01(key, sweep, r) for r in range(N)], dtype=np.float64)
    want, near = inverse_cdf(probs, u)
    check_replay("group", g, want, near)
    # ... and not the draw a sweep with the same (seed, sweep) makes
    u_sweep = np.array([orc.uniform01(seed, sweep, r) for r in range(N)], dtype=np.float64)
    assert not np.array_equal(u, u_sweep)
    assert (inverse_cdf(probs, u_sweep)[0] == g).mean() < 0.9


def group_state(ctx, family, dim, K, n_per, seed, hp=None, empty=0):
    """K groups of n_per rows each; the last `empty` of them hold no row (their draws are the prior predictive's)"""
    rng = np.random.default_rng(seed)
    f = make_feature(family, (K - empty) * n_per, K, rng, dim=dim, hp=hp)
    z = np.repeat(np.arange(K - empty), n_per).astype(np.int32)
    fs = state_from_assignment([f], K, z)
    st = common_amd.State(ctx, [(family, dim)], K)
    load_state(st, fs)
    return f, fs[0], st


def draws_of_group(ctx, st, view, k, n, seed=99):
    zt = torch.full((n,), k, dtype=torch.int32, device=ctx.torch_device)
    out, _ = st.sample_predictive(view, z=zt, seed=seed, sweep=k, nrows=n)
    return out[0].cpu().numpy()


def pooled_chi2(x, pmf, min_expected=20.0):
    hi = int(x.max())
    ks = np.arange(hi + 1)
    obs = np.bincount(x.astype(np.int64), minlength=hi + 1).astype(np.float64)
    exp = pmf(ks) * x.size
    exp[-1] += max(0.0, x.size - exp.sum())
    co, ce, ao, ae = [], [], 0.0, 0.0
    for o, e in zip(obs, exp):
        ao, ae = ao + o, ae + e
        if ae >= min_expected:
            co.append(ao); ce.append(ae); ao = ae = 0.0
    co[-1] += ao; ce[-1] += ae
    co, ce = np.array(co), np.array(ce)
    return stats.chisquare(co, ce * co.sum() / ce.sum()).pvalue


@pytest.mark.parametrize("family", [orc.GP, orc.BNB])
def test_count_families_follow_their_predictive(gpu_ctx, family):
    K, n = 3, 1 << 20
    f, (F, ss64, _), st = group_state(gpu_ctx, family, 0, K, 6, 31)
    vals = np.zeros(n, dtype=[("f0", f["np_dtype"])])
    view = common_amd.DataView.from_recarray(gpu_ctx, vals)
    for k in range(K):
        x = draws_of_group(gpu_ctx, st, view, k, n)
        h = f["hp"]
        if family == orc.GP:
            a = h["alpha"] + float(ss64["sum"][k])
            theta = 1.0 / (h["inv_beta"] + float(ss64["count"][k]))
            pmf = stats.nbinom(a, 1.0 / (1.0 + theta)).pmf
        else:
            r = h["r"]
            pmf = stats.betanbinom(r, h["alpha"] + r * float(ss64["count"][k]), h["beta"] + float(ss64["sum"][k])).pmf
        audit("pred_gpu_chi2_p", -pooled_chi2(x, pmf), -P_GATE)


def test_nich_follows_its_student_t(gpu_ctx):
    K, n = 3, 1 << 20
    f, (F, ss64, _), st = group_state(gpu_ctx, orc.NICH, 0, K, 5, 41)
    view = common_amd.DataView.from_recarray(gpu_ctx, np.zeros(n, dtype=[("f0", np.float32)]))
    h = f["hp"]
    for k in range(K):
        x = draws_of_group(gpu_ctx, st, view, k, n).astype(np.float64)
        cnt, mean, ctv = float(ss64["count"][k]), float(ss64["mean"][k]), float(ss64["count_times_variance"][k])
        kn, nun = h["kappa"] + cnt, h["nu"] + cnt
        mun = (h["kappa"] * h["mu"] + cnt * mean) / kn
        s2 = (h["nu"] * h["sigmasq"] + ctv + cnt * h["kappa"] * (h["mu"] - mean) ** 2 / kn) / nun
        audit("pred_gpu_ks_p", -stats.kstest(x, stats.t(nun, mun, np.sqrt(s2 * (kn + 1) / kn)).cdf).pvalue, -P_GATE)


@pytest.mark.parametrize("dim", [3, 32, 128])      # (128: the widest niw, 65 KiB of LDS a workgroup, the largest factor)
def test_niw_moments_marginals_and_projection(gpu_ctx, dim):
    K, n = 2, (1 << 18) if dim <= 32 else (1 << 16)
    f, (F, ss64, _), st = group_state(gpu_ctx, orc.NIW, dim, K, 2 * dim, 51 + dim)
    view = common_amd.DataView.from_recarray(gpu_ctx, np.zeros(n, dtype=[("f0", np.float32, (dim,))]))
    h = f["hp"]
    rng = np.random.default_rng(dim)
    for k in range(K):
        x = draws_of_group(gpu_ctx, st, view, k, n).astype(np.float64)
        cnt = float(ss64["count"][k])
        sx, sxx = ss64["sum_x"][k].astype(np.float64), ss64["sum_xxT"][k].astype(np.float64).reshape(dim, dim)
        mu0, psi = np.asarray(h["mu"], np.float64), np.asarray(h["psi"], np.float64).reshape(dim, dim)
        kn, nun = h["kappa"] + cnt, h["nu"] + cnt
        mun = (h["kappa"] * mu0 + sx) / kn
        psin = psi + sxx + h["kappa"] * np.outer(mu0, mu0) - kn * np.outer(mun, mun)
        dof = nun - dim + 1
        sigma = psin * (kn + 1) / (kn * dof)
        cov = sigma * dof / (dof - 2)
        sd = np.sqrt(np.diag(cov))
        audit("pred_niw_mean_z", (np.abs(x.mean(0) - mun) / (sd / np.sqrt(n))).max(), 6.0)
        audit("pred_niw_cov_rel", (np.abs(np.cov(x.T) - cov) / np.outer(sd, sd)).max(), 0.05)
        for i in (0, dim - 1):
            audit("pred_gpu_ks_p", -stats.kstest(x[:, i], stats.t(dof, mun[i], np.sqrt(sigma[i, i])).cdf).pvalue, -P_GATE)
        a = rng.normal(size=dim)
        audit("pred_gpu_ks_p", -stats.kstest(x @ a, stats.t(dof, a @ mun, np.sqrt(a @ sigma @ a)).cdf).pvalue, -P_GATE)


SPECS = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 6), (orc.NICH, 0), (orc.BNB, 0), (orc.NIW, 3)]


def test_impute_keeps_observed_entries_and_draws_masked_ones(gpu_ctx):
    N, K = 3000, 8
    feats, fs, st, view, z, arr = setup(gpu_ctx, SPECS, N, K, 61, masked=0.25)
    # one niw row with a single masked element: drawn whole
    arr.mask["f5"][7] = [False, True, False]
    arr.mask["f5"][8] = [False, False, False]
    view = common_amd.DataView.from_recarray(gpu_ctx, arr)
    out, groups = st.impute(view, seed=4, sweep=1)
    assert groups.cpu().numpy().min() >= 0
    for f, feat in enumerate(feats):
        got = out[f].cpu().numpy()
        m = np.ma.getmaskarray(arr)["f%d" % f]
        obs = ~(m if m.ndim == 1 else m.any(1))
        want = np.asarray(arr.data["f%d" % f])
        assert np.array_equal(got[obs].view(np.uint8), want[obs].astype(got.dtype).view(np.uint8)), f
        if feat["family"] == orc.NIW:
            assert not np.any(got[7][[0, 2]] == want[7][[0, 2]])
    # without masked_only every entry is drawn
    full, _ = st.sample_predictive(view, seed=4, sweep=1)
    assert (full[3].cpu().numpy() != arr.data["f3"]).mean() > 0.99


def test_rows_out_of_range_and_features_not_asked_for_are_left_alone(gpu_ctx):
    N, K = 1000, 8
    feats, fs, st, view, z, _ = setup(gpu_ctx, SPECS, N, K, 71)
    zz = z.copy()
    zz[::7], zz[3::7] = -1, K
    zt = torch.from_numpy(zz).to(gpu_ctx.torch_device)
    dev = gpu_ctx.torch_device
    pre = {1: torch.full((N,), 0xABCDEF, dtype=torch.uint32, device=dev),
           3: torch.full((N,), 12345.0, dtype=torch.float32, device=dev),
           5: torch.full((N, 3), -7.0, dtype=torch.float32, device=dev)}
    out, groups = st.sample_predictive(view, z=zt, seed=1, sweep=2, features=[1, 3, 5], out=pre)
    assert sorted(out) == [1, 3, 5]
    skip = (zz < 0) | (zz >= K)
    g = groups.cpu().numpy()
    assert np.all(g[skip] == -1) and np.array_equal(g[~skip], zz[~skip])
    assert np.all(out[1].cpu().numpy()[skip] == 0xABCDEF) and np.all(out[3].cpu().numpy()[skip] == 12345.0)
    assert np.all(out[5].cpu().numpy()[skip] == -7.0) and np.all(out[3].cpu().numpy()[~skip] != 12345.0)
    # NULL outputs at the C level: feature 0 only, the others are not touched
    o0 = torch.full((N,), 9, dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * len(SPECS))(o0.data_ptr())
    L.check(gpu_ctx.lib.msc_sample_predictive(st._h, view._h, None, 0, N, 0, C.c_void_p(zt.data_ptr()), None, 0, 1, 2,
                                              ptrs))
    torch.cuda.synchronize()
    assert set(np.unique(o0.cpu().numpy()[~skip])) <= {0, 1} and np.all(o0.cpu().numpy()[skip] == 9)


def _all(out):
    return {f: t.cpu().numpy().copy() for f, t in out.items()}


def test_draws_are_reproducible_and_independent_of_the_row_split(gpu_ctx):
    N, K = 2000, 8
    feats, fs, st, view, z, _ = setup(gpu_ctx, SPECS, N, K, 81, masked=0.2)
    a, ga = st.impute(view, seed=5, sweep=9)
    a, ga = _all(a), ga.cpu().numpy()
    b, gb = st.impute(view, seed=5, sweep=9)
    assert np.array_equal(ga, gb.cpu().numpy())
    for f in a:
        assert np.array_equal(a[f].view(np.uint8), b[f].cpu().numpy().view(np.uint8))
    h = N // 2 + 13
    lo, glo = st.impute(view, seed=5, sweep=9, row0=0, nrows=h)
    lo, glo = _all(lo), glo.cpu().numpy()
    hi, ghi = st.impute(view, seed=5, sweep=9, row0=h, nrows=N - h, row_id0=h)
    assert np.array_equal(np.concatenate([glo, ghi.cpu().numpy()]), ga)
    for f in a:
        both = np.concatenate([lo[f], hi[f].cpu().numpy()])
        assert np.array_equal(both.view(np.uint8), a[f].view(np.uint8)), f
    for kw in (dict(seed=6, sweep=9), dict(seed=5, sweep=10)):
        c, gc = st.sample_predictive(view, **kw)
        d0, _ = st.sample_predictive(view, seed=5, sweep=9)
        assert (c[3].cpu().numpy() != d0[3].cpu().numpy()).mean() > 0.99


def snapshot(st, view, z):
    ss = [st.get_ss(f).tobytes() for f in range(len(st.features))]
    cnt = st.get_group_counts().tobytes()
    sd = st.score_data().cpu().numpy().tobytes()
    zt = torch.from_numpy(z).to(st.ctx.torch_device)
    st.sweep_step(view, zt, seed=3, sweep=0)
    after = [st.get_ss(f).tobytes() for f in range(len(st.features))]
    return ss, cnt, sd, zt.cpu().numpy().tobytes(), after


def test_state_is_left_untouched(gpu_ctx):
    N, K = 2000, 16
    _, _, st1, view1, z, _ = setup(gpu_ctx, SPECS, N, K, 91, masked=0.2)
    _, _, st2, view2, _, _ = setup(gpu_ctx, SPECS, N, K, 91, masked=0.2)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    st2.sweep_assign(view2, zt.clone(), seed=3, sweep=0)     # (the device's sweep counter pair is in use)
    st1.sweep_assign(view1, zt.clone(), seed=3, sweep=0)
    st2.impute(view2, seed=8, sweep=0)
    st2.sample_predictive(view2, z=zt, seed=8, sweep=1)
    assert snapshot(st1, view1, z) == snapshot(st2, view2, z)


def test_errors(gpu_ctx):
    N, K = 500, 8
    rng = np.random.default_rng(5)
    feats = [make_feature(orc.NICH, N, K, rng), make_feature(orc.DM, N, K, rng, dim=4)]
    z = rng.integers(0, K, N).astype(np.int32)
    fs = state_from_assignment(feats, K, z)
    st = common_amd.State(gpu_ctx, [(orc.NICH, 0), (orc.DM, 4)], K)
    load_state(st, fs)
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    before = [st.get_ss(f).tobytes() for f in range(2)]
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        st.sample_predictive(view, seed=1, sweep=0)
    assert e.value.code == -4
    o = torch.zeros((N, 4), dtype=torch.int32, device=gpu_ctx.torch_device)
    ptrs = (C.c_void_p * 2)(None, o.data_ptr())
    rc = gpu_ctx.lib.msc_sample_predictive(st._h, view._h, None, 0, N, 0, None, None, 0, 1, 0, ptrs)
    assert rc == -4 and [st.get_ss(f).tobytes() for f in range(2)] == before
    out, _ = st.sample_predictive(view, seed=1, sweep=0, features=[0])       # dm not asked for: fine
    assert out[0].shape == (N,)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    with pytest.raises(ValueError):
        st.sample_predictive(view, z=zt.to(torch.int64), features=[0])
    with pytest.raises(ValueError):
        st.sample_predictive(view, features=[0], out={0: torch.zeros(N, dtype=torch.float64, device=gpu_ctx.torch_device)})
    with pytest.raises(ValueError):
        st.sample_predictive(view, features=[0], nrows=N + 1)
    rc = gpu_ctx.lib.msc_sample_predictive(st._h, view._h, None, 0, N, 0, None, None, 0x2, 1, 0, (C.c_void_p * 2)())
    assert rc == -1
    st2 = common_amd.State(gpu_ctx, [(orc.NICH, 0)], K)
    load_state(st2, fs[:1])
    st2.set_group_counts(np.bincount(z, minlength=K).astype(np.uint32))
    st2.sweep_step_begin(view, zt.clone(), seed=1, sweep=0)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        st2.sample_predictive(view, seed=1, sweep=0)
    assert e.value.code == -1
    st2.commit_reduce()
    st2.sample_predictive(view, seed=1, sweep=0)
