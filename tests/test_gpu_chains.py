"""GPU: many sequential chains in one launch (msc_chains_sweep, common_amd.ChainEnsemble) -- every chain against a twin
State run with State.sweep_sequential (the same bits), grids beyond the compute units, calls that span launches, orders,
the thinned trace and the occupied counts, the pooled chains against the exact posterior, the z-matrix hand-over, errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]


def _data(gpu_ctx, specs, N, K, seed, mask_col=None):
    """seeded features and their view; mask_col: that column has a fifth of its entries masked"""
    import common_amd
    rng = np.random.default_rng(seed)
    feats = [make_feature(f, N, max(min(K, 6), 2), rng, d) for f, d in specs]
    data = recarray_of(feats)
    if mask_col is not None:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in data.dtype.names])
        mask["f%d" % mask_col] = rng.random(N) < 0.2
        data = np.ma.masked_array(data, mask=mask)
    return feats, common_amd.DataView.from_recarray(gpu_ctx, data)


def _ensemble(gpu_ctx, feats, K, nchains, alpha=1.0):
    import common_amd
    return common_amd.ChainEnsemble(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K, nchains, alpha=alpha,
                                    hps=[f["hp"] for f in feats])


def _state_bits(st):
    """everything a sweep leaves in a state, as bytes: the group counts and every feature's suff-stats"""
    return [st.get_group_counts().tobytes()] + [st.get_ss(i).tobytes() for i in range(len(st.features))]


def _install(st, start):
    cnt, ss = start
    st.set_group_counts(cnt)
    for i, rec in enumerate(ss):
        st.set_ss(i, rec)


def _pin_start(ens):
    """accumulate adds its double sums with atomics, in an order that varies from run to run, so two states built by two
    accumulate calls may differ in the last bits of a sum.  The start is therefore pinned: every chain's tables are read
    back and installed again (the records, from which the additive sums are rebuilt element by element), and a twin is
    given the same records -> [(group counts, [suff-stats of every feature])] per chain"""
    starts = []
    for st in ens.states:
        starts.append((st.get_group_counts(), [st.get_ss(i) for i in range(len(st.features))]))
        _install(st, starts[-1])
    return starts


def _twin(gpu_ctx, feats, K, alpha, view, z0, start, seed, nsweeps, sweep=0, order=None):
    """a fresh State given the chain's start and run alone with State.sweep_sequential -> (z, full trace, state bits)"""
    import common_amd
    dev = gpu_ctx.torch_device
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    for i, f in enumerate(feats):
        st.set_hp(i, f["hp"])
    st.set_alpha(alpha)
    _install(st, start)
    zt = torch.from_numpy(np.ascontiguousarray(z0, dtype=np.int32)).to(dev)
    n = len(z0)
    trace = torch.full((max(nsweeps, 1) * n,), -7, dtype=torch.int32, device=dev)
    ot = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    st.sweep_sequential(view, zt, seed, sweep, nsweeps=nsweeps, order=ot, trace=trace)
    out = zt.cpu().numpy(), trace.cpu().numpy().reshape(-1, n)[:nsweeps], _state_bits(st)
    st.close()
    return out


def _check_chain(gpu_ctx, ens, c, feats, K, alpha, view, z0, start, seed, nsweeps, trace=None, every=1, order=None,
                 sweep=0):
    """chain c of the ensemble against its twin: integers equal, floats equal as bits"""
    z, tr, bits = _twin(gpu_ctx, feats, K, alpha, view, z0, start, seed, nsweeps, sweep=sweep, order=order)
    assert np.array_equal(ens.z[c].cpu().numpy(), z), c
    if trace is not None:
        assert np.array_equal(trace[c], tr[every - 1::every][:trace.shape[1]]), c
    assert _state_bits(ens.states[c]) == bits, c


@pytest.mark.parametrize("K", [8, 300])
def test_chain_is_the_single_chain_call_bit_for_bit(gpu_ctx, K):
    """K = 8: the sliced score path (K below the block); K = 300: the strided one"""
    N, nchains, nsweeps = 37, 5, 3
    feats, view = _data(gpu_ctx, C3_SMALL, N, K, seed=400 + K, mask_col=2)
    rng = np.random.default_rng(K)
    z0 = rng.integers(0, K - 2, (nchains, N)).astype(np.int32)
    z0[3] = -1                                           # one chain starts unassigned: its first sweep seats it
    alphas = [1.3, 1.3, 0.4, 1.3, 1.3]
    seeds = [11, 4, 1 << 40, 11, 97]
    ens = _ensemble(gpu_ctx, feats, K, nchains, alpha=alphas)
    ens.assign(view, z0)
    starts = _pin_start(ens)
    trace = ens.sweep(view, nsweeps, seeds, sweep=5, trace_every=1)
    assert tuple(trace.shape) == (nchains, nsweeps, N)
    tr = trace.cpu().numpy()
    gpu_ctx.synchronize()
    for c in range(nchains):
        _check_chain(gpu_ctx, ens, c, feats, K, alphas[c], view, z0[c], starts[c], seeds[c], nsweeps, trace=tr, sweep=5)
    assert ((tr >= 0) & (tr < K)).all()
    ens.close()


def test_more_chains_than_compute_units(gpu_ctx):
    N, K, nchains, nsweeps = 6, 7, 300, 4
    feats, view = _data(gpu_ctx, [(orc.BB, 0), (orc.NICH, 0)], N, K, seed=7)
    z0 = np.random.default_rng(8).integers(0, K, (nchains, N)).astype(np.int32)
    ens = _ensemble(gpu_ctx, feats, K, nchains)
    ens.assign(view, z0)
    starts = _pin_start(ens)
    tr = ens.sweep(view, nsweeps, 1000, trace_every=1).cpu().numpy()      # (chain c's key: 1000 + c)
    gpu_ctx.synchronize()
    assert tr.shape == (nchains, nsweeps, N) and ((tr >= 0) & (tr < K)).all()
    for c in (0, 1, 255, 256, 299):
        _check_chain(gpu_ctx, ens, c, feats, K, 1.0, view, z0[c], starts[c], 1000 + c, nsweeps, trace=tr)
    ens.close()


def test_a_call_that_spans_launches(gpu_ctx):
    """40 sweeps of 64 rows are 2560 visits a chain; a launch takes about 1200 at this shape (one nich column, K = 16)"""
    N, K, nchains = 64, 16, 3
    feats, view = _data(gpu_ctx, [(orc.NICH, 0)], N, K, seed=21)
    z0 = np.random.default_rng(22).integers(0, K - 3, (nchains, N)).astype(np.int32)
    seeds = [3, 30, 300]
    ens = _ensemble(gpu_ctx, feats, K, nchains)
    ens.assign(view, z0)
    starts = _pin_start(ens)
    tr = ens.sweep(view, 40, seeds, trace_every=1).cpu().numpy()
    for c in range(nchains):
        _check_chain(gpu_ctx, ens, c, feats, K, 1.0, view, z0[c], starts[c], seeds[c], 40, trace=tr)
    z_one, bits_one = ens.z.cpu().numpy(), [_state_bits(st) for st in ens.states]
    ens.assign(view, z0)
    for st, start in zip(ens.states, starts):
        _install(st, start)
    ta = ens.sweep(view, 20, seeds, sweep=0, trace_every=1).cpu().numpy()
    tb = ens.sweep(view, 20, seeds, sweep=20, trace_every=1).cpu().numpy()
    assert np.array_equal(np.concatenate([ta, tb], axis=1), tr)
    assert np.array_equal(ens.z.cpu().numpy(), z_one)
    assert [_state_bits(st) for st in ens.states] == bits_one
    ens.close()


def test_orders_and_thinning(gpu_ctx):
    N, K, nchains, nsweeps = 29, 12, 4, 7
    feats, view = _data(gpu_ctx, [(orc.BB, 0), (orc.NICH, 0), (orc.GP, 0)], N, K, seed=31)
    rng = np.random.default_rng(32)
    z0 = rng.integers(0, K - 4, (nchains, N)).astype(np.int32)
    dev = gpu_ctx.torch_device
    ens = _ensemble(gpu_ctx, feats, K, nchains)
    # one permutation for all chains
    shared = rng.permutation(N).astype(np.int32)
    ens.assign(view, z0)
    starts = _pin_start(ens)
    trace, occ = ens.sweep(view, 2, 50, order=torch.from_numpy(shared).to(dev), trace_every=1, want_occupied=True)
    tr, occ = trace.cpu().numpy(), occ.cpu().numpy()
    for c in range(nchains):
        _check_chain(gpu_ctx, ens, c, feats, K, 1.0, view, z0[c], starts[c], 50 + c, 2, trace=tr, order=shared)
        assert occ[c, -1] == int((ens.states[c].get_group_counts() > 0).sum()) == len(np.unique(tr[c, -1])), c
    # one permutation per chain; every second sweep traced; the occupied counts
    own = np.stack([rng.permutation(N) for _ in range(nchains)]).astype(np.int32)
    ens.assign(view, z0)
    starts = _pin_start(ens)
    trace, occ = ens.sweep(view, nsweeps, 60, order=torch.from_numpy(own).to(dev), trace_every=2, want_occupied=True)
    tr, occ = trace.cpu().numpy(), occ.cpu().numpy()
    assert tr.shape == (nchains, 3, N) and occ.shape == (nchains, 3)
    for c in range(nchains):
        _check_chain(gpu_ctx, ens, c, feats, K, 1.0, view, z0[c], starts[c], 60 + c, nsweeps, trace=tr, every=2, order=own[c])
        for j in range(3):
            assert occ[c, j] == len(np.unique(tr[c, j])), (c, j)
    ens.close()


def test_pooled_chains_reach_the_exact_posterior(gpu_ctx):
    """N = 6, K = 7, alpha = 1: 250 chains seated from all-unassigned, 800 sweeps each, every sweep traced -- 2e5 samples,
    the sample count and the gates of test_gpu_sequential.py::test_exact_posterior_of_six_rows (TV <= 0.05, KL <= 0.01;
    independent sampling noise alone gives TV ~ 0.013 over the 203 partitions)"""
    rng = np.random.default_rng(2024)
    N, K, alpha, nchains, nsweeps = 6, 7, 1.0, 250, 800
    datasets = {
        "bb3": [make_feature(orc.BB, N, 2, rng) for _ in range(3)],
        "nich_bb": [make_feature(orc.NICH, N, 2, rng), make_feature(orc.BB, N, 2, rng)],
    }
    datasets["nich_bb"][0]["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    import common_amd
    for name, feats in datasets.items():
        Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
        parts, p = sh.exact_posterior([(F, f["values"]) for F, f in zip(Fs, feats)], alpha)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
        ens = common_amd.ChainEnsemble(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K, nchains, alpha=alpha,
                                       hps=[F.hp for F in Fs])
        ens.seat(view)
        trace = ens.sweep(view, nsweeps, 77, trace_every=1)
        freq = sh.partition_frequencies(trace.cpu().numpy().reshape(-1, N), parts)
        tv, kl = sh.tv_kl(freq, p)
        print("exact posterior %s: %d pooled chains x %d sweeps TV %.4f KL %.5f" % (name, nchains, nsweeps, tv, kl))
        ens.close()
        assert tv <= 0.05 and kl <= 0.01, (name, tv, kl)


def test_into_the_zmatrix(gpu_ctx):
    import common_amd
    N, K, nchains, nsweeps = 40, 10, 8, 5
    feats, view = _data(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], N, K, seed=61)
    ens = _ensemble(gpu_ctx, feats, K, nchains)
    ens.seat(view)
    zm = common_amd.ZMatrix(gpu_ctx, N, K)
    trace = ens.sweep(view, nsweeps, 5, zmatrix=zm)
    assert zm.nsamples == nchains * nsweeps == 40
    got = zm.result().cpu().numpy()
    want = common_amd.query.zmatrix(trace.cpu().numpy().reshape(-1, N))
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    zm.close()
    ens.close()


def _create(lib, states):
    hs = (C.c_void_p * len(states))(*[st._h.value for st in states])
    h = C.c_void_p()
    return lib.msc_chains_create(hs, len(states), C.byref(h)), h


def test_errors(gpu_ctx):
    import common_amd
    lib = gpu_ctx.lib
    spec = [(orc.NICH, 0), (orc.BB, 0)]
    a, b = common_amd.State(gpu_ctx, spec, 8), common_amd.State(gpu_ctx, spec, 8)
    for states, word in (([a, b, a], "state 2"), ([a, common_amd.State(gpu_ctx, spec, 9)], "state 1"),
                         ([a, b, common_amd.State(gpu_ctx, [(orc.NICH, 0), (orc.GP, 0)], 8)], "state 2"),
                         ([a, common_amd.State(gpu_ctx, spec[:1], 8)], "state 1")):
        rc, _ = _create(lib, states)
        assert rc == -1 and word in lib.msc_last_error().decode(), (word, lib.msc_last_error())
    rc, _ = _create(lib, [])
    assert rc == -1
    other = common_amd.Context(device=0)                   # a second context on the device
    foreign = common_amd.State(other, spec, 8)
    rc, _ = _create(lib, [a, foreign])
    assert rc == -1 and "state 1" in lib.msc_last_error().decode()
    foreign.close()
    other.close()
    for bad in ((orc.NIW, 3), (orc.DM, 4), (orc.BBNC, 0)):
        with pytest.raises(common_amd.MicroscopesHipError) as e:
            common_amd.ChainEnsemble(gpu_ctx, [bad, (orc.NICH, 0)], 8, 2)
        assert e.value.code == -4
    # a member state cannot be destroyed while the handle lives
    rc, h = _create(lib, [a, b])
    assert rc == 0
    n = C.c_uint32()
    assert lib.msc_chains_size(h, C.byref(n)) == 0 and n.value == 2
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        a.close()
    assert e.value.code == -1 and "msc_chains" in str(e.value) and a._h
    assert lib.msc_chains_destroy(h) == 0
    a.close()
    b.close()
    assert a._h is None

    # the sweep's own arguments
    N, K, nchains = 20, 8, 3
    feats, view = _data(gpu_ctx, spec, N, K, seed=71)
    ens = _ensemble(gpu_ctx, feats, K, nchains)
    z0 = np.random.default_rng(72).integers(0, K, (nchains, N)).astype(np.int32)
    ens.assign(view, z0)
    seeds = (C.c_uint64 * nchains)(1, 2, 3)
    trace = torch.empty((nchains, 2, N), dtype=torch.int32, device=gpu_ctx.torch_device)
    zp, tp = C.c_void_p(ens.z.data_ptr()), C.c_void_p(trace.data_ptr())
    assert lib.msc_chains_sweep(ens._h, view._h, None, 0, N, 0, zp, N - 1, None, 0, 2, seeds, 0, 1, None, None) == -1
    assert lib.msc_chains_sweep(ens._h, view._h, None, 0, N, 0, zp, N, None, 0, 2, seeds, 0, 0, tp, None) == -1
    assert "trace_every" in lib.msc_last_error().decode()
    with pytest.raises(ValueError):
        ens.sweep(view, 2, 1, trace_every=0)
    with pytest.raises(ValueError):
        ens.sweep(view, 2, [1, 2])
    with pytest.raises(ValueError):
        ens.sweep(view, 2, 1, order=torch.arange(N, dtype=torch.int64, device=gpu_ctx.torch_device))
    with pytest.raises(ValueError):
        ens.sweep(view, 2, 1, order=torch.arange(N - 1, dtype=torch.int32, device=gpu_ctx.torch_device))
    with pytest.raises(ValueError):
        ens.sweep(view, 2, 1, order=torch.arange(N, dtype=torch.int32))
    with pytest.raises(ValueError):
        ens.sweep(view, 1 << 32, 1)
    with pytest.raises(ValueError):
        ens.assign(view, z0.astype(np.int64))
    # nothing above ran a visit, and nsweeps = 0 runs none either: z and the tables are as assign() left them
    bits = [_state_bits(st) for st in ens.states]
    assert ens.sweep(view, 0, 1) is None
    assert tuple(ens.sweep(view, 0, 1, trace_every=1).shape) == (nchains, 0, N)
    gpu_ctx.synchronize()
    assert np.array_equal(ens.z.cpu().numpy(), z0) and [_state_bits(st) for st in ens.states] == bits
    # close: the handle, then the states; a second close is harmless
    states = list(ens.states)
    ens.close()
    assert all(st._h is None for st in states) and ens.states == []
    ens.close()
    with pytest.raises(ValueError):
        ens.sweep(view, 1, 1)
