"""Grid hyper-parameter inference on the device (msc_hp_grid_*, State.hp_grid / crp_grid / hp_gibbs): every grid point's
marginal likelihood against the oracle's double twin, the CRP grid against score_assignment, the draw against a numpy
recomputation and against the softmax, the installation of the chosen point against set_hp / set_alpha through whole
sweeps, determinism, and the argument checks."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.gpu_helpers import audit, make_feature, recarray_of

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
FAMILIES = [(orc.BB, 0), (orc.BBNC, 0), (orc.BNB, 0), (orc.GP, 0), (orc.NICH, 0), (orc.DD, 5), (orc.DM, 4)]


def _records(family, dim, K, rng, empty):
    """random float suff-stats of K groups (slots in `empty` hold no data) and the group counts that go with them"""
    import common_amd
    rec = np.zeros(K, dtype=common_amd.ss_dtype(family, dim))
    n = rng.integers(1, 60, K).astype(np.uint32)
    n[empty] = 0
    if family in (orc.BB, orc.BBNC):
        h = rng.binomial(n, rng.uniform(0.05, 0.95, K)).astype(np.uint32)
        rec["heads"], rec["tails"] = h, n - h
        if family == orc.BBNC:
            rec["p"] = rng.uniform(0.02, 0.98, K).astype(np.float32)
            rec["p"][np.flatnonzero(empty)[:1]] = 7.0   # not a probability: never read while its slot is not counted
    elif family in (orc.GP, orc.BNB):
        rec["count"] = n
        rec["sum"] = rng.poisson(4.0 * n).astype(np.uint32)
        if family == orc.GP:
            rec["log_prod"] = (rng.uniform(0.0, 3.0, K) * n).astype(np.float32)
    elif family == orc.NICH:
        rec["count"] = n
        rec["mean"] = rng.normal(0, 3, K).astype(np.float32)
        rec["count_times_variance"] = (rng.uniform(0.1, 4.0, K) * n).astype(np.float32)
        rec["mean"][empty] = 0
        rec["count_times_variance"][empty] = 0
    elif family == orc.DD:
        c = np.array([rng.multinomial(int(k), np.ones(dim) / dim) for k in n], dtype=np.uint32).reshape(K, dim)
        rec["counts"], rec["count_sum"] = c, c.sum(1)
    elif family == orc.DM:
        c = rng.integers(0, 9, (K, dim)).astype(np.uint32)
        c[empty] = 0
        rec["counts"] = c
        rec["ratio"] = np.where(n > 0, rng.uniform(-5, 5, K), 0).astype(np.float32)
    return rec, n


def _ss64(family, dim, rec):
    ss = np.zeros(rec.shape[0], dtype=orc.ss_dtype(family, dim, "f64"))
    for name in rec.dtype.names:
        ss[name] = rec[name]
    return ss


def _random_blocks(family, dim, G, rng):
    if family in (orc.BB, orc.BBNC):
        return rng.uniform(0.1, 10, (G, 2)).astype(np.float32)
    if family == orc.GP:
        return rng.uniform(0.1, 10, (G, 2)).astype(np.float32)
    if family == orc.BNB:
        b = rng.uniform(0.1, 10, (G, 3)).astype(np.float32)
        b[:, 2] = rng.integers(1, 8, G)
        return b
    if family == orc.NICH:
        return np.stack([rng.uniform(-2, 2, G), rng.uniform(0.5, 4, G), rng.uniform(0.1, 10, G),
                         rng.uniform(1, 8, G)], 1).astype(np.float32)
    return rng.uniform(0.2, 5, (G, dim)).astype(np.float32)


def _default_blocks(family, dim, rng):
    from common_amd import hypers, models
    desc = {orc.BB: models.bb, orc.BBNC: models.bbnc, orc.BNB: models.bnb, orc.GP: models.gp,
            orc.NICH: models.nich}.get(family)
    if desc is None:                                 # dd / dm have no default grid: 10 000 random points
        return _random_blocks(family, dim, 10000, rng)
    cur = {orc.BNB: {"alpha": 1., "beta": 1., "r": 3}, orc.NICH: {"mu": 0.5, "kappa": 2., "sigmasq": 1., "nu": 3.}}
    return hypers.grid_blocks(desc, cur.get(family))


def _check_grid(F, dim, blocks, ss64, counted, dev, name, rng):
    pts = np.arange(blocks.shape[0])
    if pts.size > 600:
        pts = np.sort(rng.choice(pts, 600, replace=False))
    worst = 0.0
    for g in pts:
        per = orc.Family(F, blocks[g], dim, "f64").score_data_all(ss64[counted]) if counted.any() else np.zeros(0)
        want = float(per.sum())
        gate = 1e-8 * (np.abs(per).sum() + 1.0)
        worst = max(worst, abs(dev[g] - want) / gate)
        audit(name, abs(dev[g] - want), gate)
    return worst


@pytest.mark.parametrize("family,dim", FAMILIES)
@pytest.mark.parametrize("K", [1, 37, 256, 1000])
def test_grid_scores_match_the_double_twin(gpu_ctx, family, dim, K):
    import common_amd
    rng = np.random.default_rng(1000 * family + K)
    empty = rng.random(K) < 0.3
    if K > 1:
        empty[0] = True                              # (bbnc: the invalid p sits in slot 0)
    rec, n = _records(family, dim, K, rng, empty)
    st = common_amd.State(gpu_ctx, [(family, dim)], K)
    st.set_ss(0, rec)
    st.set_group_counts(n)
    ss64 = _ss64(family, dim, rec)
    for G, blocks in ((1, _random_blocks(family, dim, 1, rng)), (97, _random_blocks(family, dim, 97, rng)),
                      (10000, _default_blocks(family, dim, rng))):
        grid = st.hp_grid(0, blocks)
        dev = grid.scores().cpu().numpy()
        _check_grid(family, dim, blocks, ss64, n > 0, dev, "hp_grid.score_data_sum", rng)
        # a caller's mask: some empty slots counted, some occupied ones not, slot 0 (bbnc's invalid p) excluded
        mask = rng.random(K) < 0.6
        mask[0] = False
        mdev = grid.scores(slots=torch.from_numpy(mask.astype(np.uint8)).to(gpu_ctx.torch_device)).cpu().numpy()
        assert np.all(np.isfinite(mdev))
        _check_grid(family, dim, blocks, ss64, mask, mdev, "hp_grid.score_data_sum_masked", rng)
        grid.close()
    st.close()


@pytest.mark.parametrize("family,dim", FAMILIES)
def test_current_hp_point_equals_the_summed_score_data(gpu_ctx, family, dim):
    import common_amd
    K = 256
    rng = np.random.default_rng(7 + family)
    empty = rng.random(K) < 0.2
    rec, n = _records(family, dim, K, rng, empty)
    st = common_amd.State(gpu_ctx, [(family, dim)], K)
    blocks = _random_blocks(family, dim, 5, rng)
    st.set_hp(0, blocks[3])
    st.set_ss(0, rec)
    st.set_group_counts(n)
    sd = st.score_data().cpu().numpy()[0].astype(np.float64)
    got = st.hp_grid(0, blocks).scores().cpu().numpy()[3]
    want = sd[n > 0].sum()
    audit("hp_grid.vs_score_data_float", abs(got - want), 1e-6 * np.maximum(1.0, np.abs(sd[n > 0])).sum())


def test_crp_grid_matches_score_assignment(gpu_ctx):
    import common_amd
    K = 300
    rng = np.random.default_rng(3)
    n = rng.integers(0, 40, K).astype(np.uint32)
    n[rng.random(K) < 0.3] = 0
    st = common_amd.State(gpu_ctx, [(orc.BB, 0)], K)
    st.set_group_counts(n)
    alphas = np.logspace(-2, 2, 100).astype(np.float32)
    dev = st.crp_grid(alphas).scores().cpu().numpy()
    z = np.repeat(np.arange(K), n)
    for a, d in zip(alphas, dev):
        want = orc.score_assignment(z, float(a))
        audit("hp_grid.crp_score_assignment", abs(d - want) / max(1.0, abs(want)), 1e-8)


def _mixed_state(gpu_ctx, K=64, seed=5):
    import common_amd
    from common_amd import models
    rng = np.random.default_rng(seed)
    specs = [(orc.BB, 0, models.bb), (orc.GP, 0, models.gp), (orc.NICH, 0, models.nich), (orc.DD, 4, models.dd(4))]
    st = common_amd.State(gpu_ctx, [(f, d) for f, d, _ in specs], K)
    empty = rng.random(K) < 0.25
    n = None
    for i, (f, d, _) in enumerate(specs):
        rec, n = _records(f, d, K, rng, empty)
        st.set_ss(i, rec)
    st.set_group_counts(n)
    return st, [desc for _, _, desc in specs], rng


def test_draw_follows_the_cdf_of_the_downloaded_scores(gpu_ctx):
    from common_amd import hypers
    st, descs, rng = _mixed_state(gpu_ctx)
    gb = hypers.FeatureHpGibbs(st, descs, grids=[None, None, None, [{"alphas": list(a)} for a in
                                                                      rng.uniform(0.3, 3, (50, 4))]],
                               cluster_grid=np.logspace(-1, 1, 40))
    grids = gb._grids
    feats = gb.features + [len(st.features)]                   # the alpha grid's stream is 2^64 - 1 - nfeatures
    for sweep in range(6):
        chosen, scores = st.hp_gibbs(grids, seed=11, sweep=sweep, want_scores=True)
        for g, k, s, f in zip(grids, chosen, scores, feats):
            s = s.cpu().numpy()
            lik = g.scores().cpu().numpy()
            assert np.array_equal(s, lik + (g.logprior if g.logprior is not None else 0.0))
            p = np.exp(s - s.max())
            cdf = np.cumsum(p)
            dart = orc.uniform01(11, sweep, U64 - f) * cdf[-1]
            want = int(np.argmax(cdf > dart))
            if want != int(k):                               # only where the dart lies on a CDF step between them
                lo, hi = min(want, int(k)), max(want, int(k))
                audit("hp_grid.draw_cdf_step", np.abs(cdf[lo:hi] - dart).min() / cdf[-1], 1e-6)


def test_draw_frequencies_follow_the_softmax(gpu_ctx):
    import common_amd
    K = 4
    st = common_amd.State(gpu_ctx, [(orc.BB, 0)], K)
    rec = np.zeros(K, dtype=common_amd.ss_dtype(orc.BB, 0))
    rec["heads"], rec["tails"] = [3, 1, 0, 5], [2, 4, 0, 1]
    st.set_ss(0, rec)
    st.set_group_counts(rec["heads"] + rec["tails"])
    blocks = np.array([[1.0, 1.0], [2.0, 0.5], [0.7, 1.6]], dtype=np.float32)
    grid = st.hp_grid(0, blocks, logprior=np.array([0.0, -0.4, 0.3]))
    s = grid.scores().cpu().numpy() + grid.logprior
    p = np.exp(s - s.max())
    p /= p.sum()
    counts = np.zeros(3)
    for seed in range(2000):
        counts[int(st.hp_gibbs([grid], seed=seed, sweep=1)[0])] += 1
    e = 2000 * p
    chi2 = float(((counts - e) ** 2 / e).sum())
    pval = math.exp(-chi2 / 2)                                 # (chi-square with 2 degrees of freedom)
    assert pval > 1e-4, (counts, e, chi2)


@pytest.mark.parametrize("graph", [False, True])
def test_installed_point_equals_set_hp_through_sweeps(gpu_ctx, graph, monkeypatch):
    import common_amd
    from common_amd import hypers, models
    monkeypatch.setenv("MSC_SWEEP_GRAPH", "1" if graph else "0")
    N, K = 3000, 32
    rng = np.random.default_rng(21)
    specs = [(orc.BB, 0, models.bb), (orc.GP, 0, models.gp), (orc.NICH, 0, models.nich), (orc.DD, 3, models.dd(3))]
    feats = [make_feature(f, N, K, rng, d) for f, d, _ in specs]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    z0 = rng.integers(0, K - 4, N).astype(np.int32)
    pair = []
    for _ in range(2):
        st = common_amd.State(gpu_ctx, [(f, d) for f, d, _ in specs], K)
        st.set_alpha(1.0)
        z = torch.from_numpy(z0).to(gpu_ctx.torch_device)
        st.accumulate(view, z)
        pair.append((st, z))
    (a, za), (b, zb) = pair
    gb = hypers.FeatureHpGibbs(a, [d for _, _, d in specs],
                               grids=[None, None, None, [{"alphas": list(x)} for x in rng.uniform(0.3, 3, (20, 3))]],
                               cluster_grid=np.logspace(-1, 1, 30))
    chosen = a.hp_gibbs(gb._grids, seed=4, sweep=0)
    for g, k in zip(gb._grids[:-1], chosen[:-1]):
        assert np.array_equal(a.get_hp(g.feature).view(np.uint32), g.blocks[k].view(np.uint32))
        b.set_hp(g.feature, g.blocks[k])
    b.set_alpha(float(gb._grids[-1].blocks[chosen[-1], 0]))
    # alpha reaches the CRP prior the same way
    sa = a.score_value(view, nrows=64, crp_prior=True).cpu().numpy()
    sb = b.score_value(view, nrows=64, crp_prior=True).cpu().numpy()
    assert np.array_equal(sa, sb)
    for sweep in range(3):
        a.sweep_step(view, za, seed=9, sweep=sweep)
        b.sweep_step(view, zb, seed=9, sweep=sweep)
        assert torch.equal(za, zb)
    assert np.array_equal(a.get_group_counts(), b.get_group_counts())
    for f in range(len(specs)):
        ra, rb = a.get_ss(f), b.get_ss(f)
        for name in ra.dtype.names:
            assert np.array_equal(ra[name], rb[name]), (f, name)


def test_scores_are_deterministic(gpu_ctx):
    st, descs, rng = _mixed_state(gpu_ctx, K=1000, seed=8)
    from common_amd import hypers
    gb = hypers.FeatureHpGibbs(st, descs, cluster_grid=np.logspace(-1, 1, 50))
    for g in gb._grids:
        x, y = g.scores().cpu().numpy(), g.scores().cpu().numpy()
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    _, s1 = st.hp_gibbs(gb._grids, seed=2, sweep=3, want_scores=True)
    _, s2 = st.hp_gibbs(gb._grids, seed=2, sweep=3, want_scores=True)
    for x, y in zip(s1, s2):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))


def test_argument_errors(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    st = common_amd.State(gpu_ctx, [(orc.BB, 0), (orc.NIW, 2)], 8)
    with pytest.raises(MicroscopesHipError) as e:
        st.hp_grid(1, np.ones((3, 8), np.float32))
    assert e.value.code == -4                                  # MSC_EUNSUPPORTED
    for bad in (np.ones((3, 3), np.float32), np.ones((0, 2), np.float32)):
        with pytest.raises(MicroscopesHipError) as e:
            st.hp_grid(0, bad)
        assert e.value.code == -1                              # MSC_EINVAL
    with pytest.raises(MicroscopesHipError) as e:
        st.crp_grid([1.0, 0.0])
    assert e.value.code == -1


def test_refused_inside_a_sharded_step(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    N, K = 500, 8
    rng = np.random.default_rng(2)
    feats = [make_feature(orc.BB, N, K, rng)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = common_amd.State(gpu_ctx, [(orc.BB, 0)], K)
    st.set_alpha(1.0)
    z = torch.from_numpy(rng.integers(0, K, N).astype(np.int32)).to(gpu_ctx.torch_device)
    st.accumulate(view, z)
    grid = st.hp_grid(0, np.ones((4, 2), np.float32))
    st.sweep_step_begin(view, z, seed=1, sweep=0)
    for call in (lambda: grid.scores(), lambda: st.hp_gibbs([grid], 1, 0)):
        with pytest.raises(MicroscopesHipError) as e:
            call()
        assert e.value.code == -1
    st.commit_reduce()
    assert st.hp_gibbs([grid], 1, 0)[0] < 4
