"""GPU: the blocked Gibbs sampler on a state of one niw feature (dim <= 32) -- the exact sampler of the Dirichlet-process
Gaussian mixture.  The assignment replayed in double from the drawn tables and matrices, the device's draws against
the Normal-Inverse-Wishart posterior and against the host build of the same header, the exact posterior of six rows,
determinism, the shard rule and the call sequence, and the error cases."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import blocked_niw_helpers as bh
from tests import seq_helpers as sh
from tests.gpu_helpers import distinct_hp, make_feature, recarray_of
from tests.test_gpu_blocked import _check_assign

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bh.build_host(tmp_path_factory.mktemp("blocked_niw_gpu"))


def _state(gpu_ctx, d, K, hp=None, alpha=1.3):
    import common_amd
    st = common_amd.State(gpu_ctx, [(orc.NIW, d)], K)
    st.set_hp(0, distinct_hp(orc.NIW, d) if hp is None else hp)
    st.set_alpha(alpha)
    return st


def _setup(gpu_ctx, d, N, K, seed, alpha=1.3, masked=False, empty=2, hp=None, shift=0.0, assigned=True, all_masked_row=None):
    """one niw column, a view, a state accumulated from z on the device, and the replay's values and row mask"""
    import common_amd
    rng = np.random.default_rng(seed)
    f = make_feature(orc.NIW, N, max(K, 2), rng, d)
    f["values"] = (f["values"] + np.float32(shift)).astype(np.float32)
    data = recarray_of([f])
    row_mask = np.zeros(N, dtype=bool)
    if masked:
        mask = np.zeros(N, dtype=[("f0", np.bool_, (d,))])
        row_mask = rng.random(N) < 0.2
        mask["f0"][row_mask, rng.integers(0, d, row_mask.sum())] = True       # one masked element hides the row
        if all_masked_row is not None:
            mask["f0"][all_masked_row, :] = True
            row_mask[all_masked_row] = True
        data = np.ma.masked_array(data, mask=mask)
    view = common_amd.DataView.from_recarray(gpu_ctx, data)
    st = _state(gpu_ctx, d, K, hp, alpha)
    z = rng.integers(0, max(1, K - empty), N).astype(np.int32) if assigned else np.full(N, -1, dtype=np.int32)
    st.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device))
    return dict(view=view, st=st, z=z, K=K, N=N, d=d, values=f["values"], row_mask=row_mask, alpha=alpha)


def _scores(st, d, values, row_mask, rows):
    """s[r, k] = log pi_k + c_k - |V_k (x_r - mu_k)|^2 / 2 in float64 from blocked_tables() and blocked_niw_params(); a
    row with a masked element: log pi_k alone"""
    tabs, par = st.blocked_tables(), st.blocked_niw_params()
    assert tabs[0].shape[0] == 1
    for t in list(tabs.values()) + list(par.values()):
        assert bool(torch.isfinite(t).all())
    logw = tabs["logw"].cpu().numpy().astype(np.float64)
    c = tabs[0][0].cpu().numpy().astype(np.float64)
    mean, V = par["mean"].cpu().numpy(), bh.unpack(par["whiten"].cpu().numpy(), d)
    assert mean.dtype == np.float64 and mean.shape == (len(logw), d)
    x = values[rows].astype(np.float64)
    y = np.einsum("kij,rkj->rki", V, x[:, None, :] - mean[None, :, :])
    s = logw[None, :] + c[None, :] - 0.5 * (y ** 2).sum(2)
    return np.where(row_mask[rows][:, None], logw[None, :], s), logw


def _draw_assign_replay(gpu_ctx, s, seed, sweep, row0=0, nrows=None, row_id0=None):
    st, view = s["st"], s["view"]
    n = s["N"] - row0 if nrows is None else nrows
    rid0 = row0 if row_id0 is None else row_id0
    st.blocked_draw(seed, sweep)
    zt = torch.full((n + 37,), -5, dtype=torch.int32, device=gpu_ctx.torch_device)
    st.blocked_assign(view, zt, seed, sweep, row0=row0, nrows=n, row_id0=row_id0)
    got = zt.cpu().numpy()
    assert (got[n:] == -5).all()                             # lanes without a row store nothing
    got = got[:n]
    assert ((got >= 0) & (got < s["K"])).all()
    rows = np.arange(row0, row0 + n)
    sc, logw = _scores(st, s["d"], s["values"], s["row_mask"], rows)
    n_off = _check_assign(sc, got, seed, sweep, rid0 + np.arange(n))
    return got, logw, n_off


@pytest.mark.parametrize("d", [2, 3, 16, 17, 32])
def test_assign_replay_across_dimensions(gpu_ctx, d):
    s = _setup(gpu_ctx, d, 1999, 48, seed=300 + d)
    _draw_assign_replay(gpu_ctx, s, seed=11 + d, sweep=2)


@pytest.mark.parametrize("K,d", [(1, 3), (2, 3), (7, 3), (64, 3), (65, 3), (257, 3), (65, 17)])
def test_assign_replay_across_slot_counts(gpu_ctx, K, d):
    s = _setup(gpu_ctx, d, 1999, K, seed=400 + K + d, empty=min(2, K - 1))
    _draw_assign_replay(gpu_ctx, s, seed=5 + K, sweep=1)


def test_assign_replay_row_offsets_and_masked_rows(gpu_ctx):
    s = _setup(gpu_ctx, 3, 1999, 48, seed=9, masked=True)
    assert 0.1 < s["row_mask"].mean() < 0.3
    _draw_assign_replay(gpu_ctx, s, seed=21, sweep=7, row0=300, nrows=1201, row_id0=50000)


def test_a_row_with_a_masked_element_draws_from_the_weights(gpu_ctx):
    s = _setup(gpu_ctx, 17, 1999, 48, seed=19, masked=True, all_masked_row=777)
    got, logw, _ = _draw_assign_replay(gpu_ctx, s, seed=8, sweep=3)
    w = np.exp(logw)
    cdf = np.cumsum(w / w.sum())
    for r in [777] + list(np.nonzero(s["row_mask"])[0][:20]):
        u = orc.uniform01(8, 3, int(r))
        want = int(orc.sample_discrete(orc.scores_to_probs(logw), u))
        assert got[r] == want or abs(cdf[min(got[r], want)] - u) < 1e-5, r


@pytest.mark.parametrize("d", [3, 32])
def test_assign_replay_far_from_the_origin(gpu_ctx, d):
    """centres near 1000 with unit spread: a subtraction or a contraction done in float would move probabilities by 1e-4
    and more.  Every slot draws from a prior centred there (sums of squares near 1e6 a row do not fit a float table)"""
    hp = distinct_hp(orc.NIW, d)
    hp = dict(hp, mu=np.asarray(hp["mu"]) + 1000.0)
    s = _setup(gpu_ctx, d, 1999, 48, seed=70 + d, hp=hp, shift=1000.0, assigned=False)
    assert abs(float(np.median(s["values"])) - 1000.0) < 5.0
    got, _, _ = _draw_assign_replay(gpu_ctx, s, seed=13, sweep=5)
    assert len(np.unique(got)) > 1


# ---- the draws ---------------------------------------------------------------------------------------------------------
def _identical_slots(gpu_ctx, d, n, K=4096, seed=123, sweep=4):
    import common_amd
    st = _state(gpu_ctx, d, K, alpha=1.0)
    _, sx, sxx = bh.members(d, n)
    rec = np.zeros(K, dtype=common_amd.ss_dtype(orc.NIW, d))
    rec["count"], rec["sum_x"], rec["sum_xxT"] = n, sx, sxx
    st.set_ss(0, rec)
    st.set_group_counts(np.full(K, n, dtype=np.uint32))
    st.blocked_draw(seed, sweep)
    par = st.blocked_niw_params()
    c = st.blocked_tables()[0][0].cpu().numpy()
    return st, par["mean"].cpu().numpy(), par["whiten"].cpu().numpy(), c, sx, sxx


@pytest.mark.parametrize("d,n", [(3, 0), (3, 500), (17, 500)])
def test_device_draws_follow_the_posterior(gpu_ctx, d, n):
    _, mean, whiten, c, sx, sxx = _identical_slots(gpu_ctx, d, n)
    hpb = bh.hp_block(distinct_hp(orc.NIW, d), d)
    kn, nun, mun, Psin = bh.posterior(hpb, d, n, sx, sxx)
    bh.check_draws(mean, whiten, c, d, kn, nun, mun, Psin)
    assert len(np.unique(whiten[:, 0])) == whiten.shape[0]   # every slot its own stream


@pytest.mark.parametrize("d", [3, 17, 32])
def test_device_against_the_host_header(gpu_ctx, host, d):
    """three slots (the last one empty) with the suff-stats the device holds: the device's mean and whiten against the host
    compiler's build of the same header, within 1e-6 of the slot's largest |V| entry"""
    s = _setup(gpu_ctx, d, 400, 3, seed=50 + d, empty=1)
    st = s["st"]
    seed, sweep = 77, 9
    st.blocked_draw(seed, sweep)
    par = st.blocked_niw_params()
    mean, whiten = par["mean"].cpu().numpy(), par["whiten"].cpu().numpy()
    c = st.blocked_tables()[0][0].cpu().numpy()
    rec = st.get_ss(0)
    assert list(rec["count"]) == list(np.bincount(s["z"], minlength=3)) and rec["count"][2] == 0 and rec["count"][0] > d
    hpb = bh.hp_block(distinct_hp(orc.NIW, d), d)
    worst = 0.0
    for k in range(3):
        sx, sxx = np.ascontiguousarray(rec["sum_x"][k]), np.ascontiguousarray(rec["sum_xxT"][k])
        hm, hw, _, hc = bh.host_draws(host, hpb, d, int(rec["count"][k]), sx, sxx, 1, seed=seed, sweep=sweep, slot0=k)
        scale = np.abs(hw[0]).max()
        err = max(np.abs(mean[k] - hm[0]).max(), np.abs(whiten[k] - hw[0]).max()) / scale
        worst = max(worst, err)
        assert abs(float(c[k]) - float(hc[0])) <= 1e-5 * max(1.0, abs(float(hc[0])))
    print("blocked niw d=%d: device against host header, largest |difference| / max|V| = %.3g" % (d, worst))
    assert worst <= 1e-6, worst


# ---- the chain ---------------------------------------------------------------------------------------------------------
def test_exact_posterior_of_six_rows(gpu_ctx):
    """N = 6, d = 2, K = 32, alpha = 1: 5e4 blocked sweeps from z = -1 visit the 203 partitions with the exact posterior's
    frequencies (truncation bound 4 N exp(-(K - 1) / alpha) = 8e-13).  The posterior puts 0.123 on its best partition and
    more than 1e-4 on 184 of the 203: it tells samplers apart (the batched chain sits at TV 0.25 and more)"""
    import common_amd
    dev = gpu_ctx.torch_device
    N, K, alpha, per_call, calls = 6, 32, 1.0, 10000, 5
    X = np.array([[0.2, 0.1], [-0.4, 0.3], [0.1, -0.2], [2.5, 2.0], [2.9, 2.4], [5.0, -1.0]], dtype=np.float32)
    hp = distinct_hp(orc.NIW, 2)
    F = orc.Family(orc.NIW, hp, 2, "f64")
    parts, p = sh.exact_posterior([(F, X)], alpha)
    assert len(parts) == 203 and abs(p.max() - 0.123) < 1e-3 and int((p > 1e-4).sum()) == 184
    f = dict(family=orc.NIW, dim=2, hp=hp, values=X, np_dtype=np.dtype((np.float32, (2,))))
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of([f]))
    st = _state(gpu_ctx, 2, K, alpha=alpha)
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
    print("exact posterior niw d=2: blocked TV %.4f KL %.5f" % (tv, kl))
    assert tv <= 0.05 and kl <= 0.01, (tv, kl)


# ---- determinism and sequencing ------------------------------------------------------------------------------------------
def _bits(st):
    out = {k: t.cpu().numpy().view(np.uint32).copy() for k, t in st.blocked_tables().items()}
    out.update({k: t.cpu().numpy().view(np.uint64).copy() for k, t in st.blocked_niw_params().items()})
    return out


def test_equal_tables_draw_equal_parameters_and_shards_assign_the_same(gpu_ctx):
    dev = gpu_ctx.torch_device
    a = _setup(gpu_ctx, 17, 1999, 48, seed=71, masked=True)
    b = _setup(gpu_ctx, 17, 1999, 48, seed=71, masked=True)
    a["st"].blocked_draw(31, 6)
    b["st"].blocked_draw(31, 6)
    ta, tb = _bits(a["st"]), _bits(b["st"])
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    b["st"].blocked_draw(31, 7)                              # another (seed, sweep) gives other parameters
    tb = _bits(b["st"])
    assert not np.array_equal(ta["logw"], tb["logw"]) and not np.array_equal(ta["whiten"], tb["whiten"])
    N = a["N"]
    whole = torch.full((N,), -1, dtype=torch.int32, device=dev)
    parts = torch.full((N,), -1, dtype=torch.int32, device=dev)
    a["st"].blocked_assign(a["view"], whole, 31, 6)
    h = N // 2                                               # (999: the second part starts in the middle of a wave's rows)
    a["st"].blocked_assign(a["view"], parts[:h], 31, 6, row0=0, nrows=h, row_id0=0)
    a["st"].blocked_assign(a["view"], parts[h:], 31, 6, row0=h, nrows=N - h, row_id0=h)
    assert np.array_equal(whole.cpu().numpy(), parts.cpu().numpy())
    assert len(np.unique(whole.cpu().numpy())) > 4


def test_sweep_blocked_is_draw_assign_accumulate(gpu_ctx):
    dev = gpu_ctx.torch_device
    a = _setup(gpu_ctx, 3, 1500, 50, seed=61)
    b = _setup(gpu_ctx, 3, 1500, 50, seed=61)
    za, zb = torch.from_numpy(a["z"].copy()).to(dev), torch.from_numpy(b["z"].copy()).to(dev)
    trace = torch.empty(2 * 1500, dtype=torch.int32, device=dev)
    a["st"].sweep_blocked(a["view"], za, 17, 4, nsweeps=2, trace=trace)
    by_hand = []
    for i in range(2):
        b["st"].blocked_draw(17, 4 + i)
        b["st"].blocked_assign(b["view"], zb, 17, 4 + i)
        by_hand.append(zb.cpu().numpy().copy())
        b["st"].accumulate(b["view"], zb, reset=True)
    assert np.array_equal(trace.cpu().numpy().reshape(2, 1500), np.stack(by_hand))
    assert not np.array_equal(by_hand[0], by_hand[1]) and not np.array_equal(by_hand[0], a["z"])
    assert np.array_equal(za.cpu().numpy(), zb.cpu().numpy())
    assert np.array_equal(a["st"].get_group_counts(), b["st"].get_group_counts())
    assert np.array_equal(a["st"].get_group_counts(), np.bincount(by_hand[1], minlength=50).astype(np.uint32))
    ra, rb = a["st"].get_ss(0), b["st"].get_ss(0)
    for name in ra.dtype.names:
        assert np.array_equal(ra[name], rb[name]), name
    ta, tb = _bits(a["st"]), _bits(b["st"])
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k


# ---- errors ------------------------------------------------------------------------------------------------------------
def _raises(code, call):
    import common_amd
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        call()
    assert e.value.code == code
    return str(e.value)


def test_errors(gpu_ctx):
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, 3, 500, 20, seed=91)
    st, view = s["st"], s["view"]
    zt = torch.from_numpy(s["z"].copy()).to(dev)
    assign = lambda: st.blocked_assign(view, zt.clone(), 1, 0)
    _raises(-1, assign)                                      # before any draw
    st.blocked_draw(1, 0)
    assign()
    st.accumulate(view, zt, reset=True)
    _raises(-1, assign)                                      # the draw is stale: the tables changed
    st.blocked_draw(1, 0)
    st.set_hp(0, distinct_hp(orc.NIW, 3, i=1))
    _raises(-1, assign)
    st.blocked_draw(1, 1)
    assign()
    # split-merge and the sequential sweep refuse the state as they always did
    msg = _raises(-4, lambda: st.split_merge(view, zt, 1, 0))
    assert "split-merge takes bb, gp, bnb, dd, nich and noop features" in msg
    _raises(-4, lambda: st.sweep_sequential(view, zt, 1, 0))
    with pytest.raises(ValueError):
        st.blocked_niw_params(1)
    with pytest.raises(ValueError):
        st.blocked_niw_params(-1)
    gpu_ctx.synchronize()


def test_dimension_beyond_32_is_refused(gpu_ctx):
    s = _setup(gpu_ctx, 33, 64, 4, seed=33)
    st, view = s["st"], s["view"]
    zt = torch.from_numpy(s["z"].copy()).to(gpu_ctx.torch_device)
    for call in (lambda: st.blocked_draw(1, 0), lambda: st.blocked_tables(), lambda: st.blocked_niw_params(),
                 lambda: st.blocked_assign(view, zt, 1, 0), lambda: st.sweep_blocked(view, zt, 1, 0)):
        assert "the blocked sweep takes a niw feature of dimension at most 32" in _raises(-4, call)


def test_params_of_a_state_without_niw(gpu_ctx):
    import common_amd
    st = common_amd.State(gpu_ctx, [(orc.NICH, 0)], 8)
    _raises(-1, lambda: st.blocked_niw_params())
