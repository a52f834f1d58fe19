"""GPU: the sweep at a temperature (msc_chains_sweep_tempered, ChainEnsemble.sweep(beta=)) and its drivers
(ChainEnsemble.run_tempered, ChainEnsemble.ais) -- beta = 1 against the untempered call bit for bit; beta = 0 blind to the
data; mixed temperatures against the double replay of a chain at a temperature (tests/temper_helpers.TemperedReplay);
calls cut into launches and temperatures changed on the device; run_tempered against its calls made by hand; every rung
of a replica-exchange run against its exact tempered posterior over the partitions of six rows; annealed importance
sampling against the exact evidence; a temperature that is none through the device error word; the arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests import smc_helpers as H
from tests import temper_helpers as TH

pytestmark = pytest.mark.gpu

K6, ALPHA6 = 7, 1.0


def _assigned(ens, view, z0):
    """assign z0 and pin the start (accumulate's atomics order their double sums differently from run to run, so the
    records are read back and installed again) -> the per-chain records, for a twin"""
    ens.assign(view, z0)
    starts = []
    for st in ens.states:
        starts.append((st.get_group_counts(), [st.get_ss(i) for i in range(len(st.features))]))
        _install(st, starts[-1])
    return starts


def _install(st, start):
    cnt, ss = start
    st.set_group_counts(cnt)
    for i, rec in enumerate(ss):
        st.set_ss(i, rec)


def _twin_of(gpu_ctx, feats, K, nchains, view, z0, starts, alpha=1.0):
    twin = H.ensemble(gpu_ctx, feats, K, nchains, alpha=alpha)
    twin.assign(view, z0)
    for st, start in zip(twin.states, starts):
        _install(st, start)
    return twin


def _dev(gpu_ctx, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu_ctx.torch_device)


def _replay_chain(rfeats, K, alpha, z_start, beta32, traces, seed, sweep0, order=None):
    """the chain's sweeps replayed in double at the chain's float32 temperature, joining the device's draws: every visit
    where the two disagree is held to Replay.visit's own tolerance there -> how many such visits"""
    n = len(z_start)
    rp = TH.TemperedReplay(rfeats, K, alpha, z_start, float(np.float32(beta32)))
    offs = np.arange(n) if order is None else np.asarray(order)
    n_off = 0
    for k, tr in enumerate(traces):
        n_off += rp.sweep(offs, seed, sweep0 + k, offs, got=tr[offs])
        assert np.array_equal(rp.z, tr), k
    return n_off


# ---- 1. beta = 1 is the untempered call, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("start", ["assigned", "seated"])
@pytest.mark.parametrize("K", [8, 300])
def test_beta_one_is_the_untempered_call_bit_for_bit(gpu_ctx, K, start):
    """K = 8: the sliced scoring path (nq > 1); K = 300: K >= the block.  z, trace, occupied and every table."""
    N, nchains, nsweeps = 300, 5, 3
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=500 + K, mask_col=2)
    seeds = [11, 4, 1 << 40, 12, 97]
    ens = H.ensemble(gpu_ctx, feats, K, nchains, alpha=1.3)
    if start == "assigned":
        z0 = np.random.default_rng(K).integers(0, K - 2, (nchains, N)).astype(np.int32)
        z0[3, ::7] = -1
        starts = _assigned(ens, view, z0)
        twin = _twin_of(gpu_ctx, feats, K, nchains, view, z0, starts, alpha=1.3)
    else:
        twin = H.ensemble(gpu_ctx, feats, K, nchains, alpha=1.3)
        ens.seat(view)
        twin.seat(view)
    ones = torch.ones(nchains, dtype=torch.float32, device=gpu_ctx.torch_device)
    tr_a, occ_a = ens.sweep(view, nsweeps, seeds, sweep=5, trace_every=1, want_occupied=True, beta=ones)
    tr_b, occ_b = twin.sweep(view, nsweeps, seeds, sweep=5, trace_every=1, want_occupied=True)
    assert tuple(tr_a.shape) == (nchains, nsweeps, N) and tuple(occ_a.shape) == (nchains, nsweeps)
    assert tr_a.cpu().numpy().tobytes() == tr_b.cpu().numpy().tobytes()
    assert occ_a.cpu().numpy().tobytes() == occ_b.cpu().numpy().tobytes()
    assert H.ensemble_bits(ens) == H.ensemble_bits(twin)
    assert len(np.unique(tr_a.cpu().numpy()[:, -1])) > 1                  # (the chains moved)
    # a float and a list of floats are made into the same tensor
    ens.sweep(view, 1, seeds, sweep=9, beta=1.0)
    twin.sweep(view, 1, seeds, sweep=9, beta=[1.0] * nchains)
    assert H.ensemble_bits(ens) == H.ensemble_bits(twin)
    gpu_ctx.synchronize()
    ens.close()
    twin.close()


# ---- 2. beta = 0 reads no feature ---------------------------------------------------------------------------------------------
def test_beta_zero_reads_no_feature(gpu_ctx):
    """two views of one shape with different values, the same keys, from seat(): the same traces; chain 0 is the CRP
    chain of the double replay.  -0.0f is 0 too."""
    N, K, nchains, nsweeps = 300, 8, 4, 2
    feats_a, _, view_a = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=71, mask_col=2)
    feats_b, _, view_b = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=72, mask_col=1)
    assert any(not np.array_equal(a["values"], b["values"]) for a, b in zip(feats_a, feats_b))
    traces = []
    for feats, view, zero in ((feats_a, view_a, 0.0), (feats_b, view_b, -0.0)):
        ens = H.ensemble(gpu_ctx, feats_a, K, nchains, alpha=1.3)        # (one set of hyper-parameters: they are not read)
        ens.seat(view)
        tr = ens.sweep(view, nsweeps, 31, sweep=2, trace_every=1, beta=np.full(nchains, zero, dtype=np.float32))
        traces.append(tr.cpu().numpy())
        assert np.array_equal(traces[-1][:, -1], ens.z.cpu().numpy())
        # the row still joined its group's suff-stats: the counts are those of z
        for c, st in enumerate(ens.states):
            assert np.array_equal(st.get_group_counts(), np.bincount(traces[-1][c, -1], minlength=K))
        gpu_ctx.synchronize()
        ens.close()
    assert traces[0].tobytes() == traces[1].tobytes()
    assert ((traces[0] >= 0) & (traces[0] < K)).all() and len(np.unique(traces[0][0, -1])) > 1
    n_off = _replay_chain(H.replay_features(feats_a, [None, None, None, None]), K, 1.3, np.full(N, -1, np.int32), 0.0,
                          traces[0][0], 31, 2)
    print("beta = 0: %d of %d visits off the replay's draw" % (n_off, nsweeps * N))
    assert n_off <= max(3, 0.005 * nsweeps * N), n_off


# ---- 3. mixed temperatures against the double replay ---------------------------------------------------------------------------
MIXED = {
    "K24": dict(betas=(1.0, 0.5, 0.25, 0.0, 1.7, 2.0 / 3.0), N=400, K=24, nsweeps=2, ordered=True),
    "K300": dict(betas=(0.5, 1.7), N=300, K=300, nsweeps=1, ordered=False),
}


@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_temperatures_against_the_replay(gpu_ctx, case):
    """every chain's trace replayed by TemperedReplay at that chain's float32 beta with got= the device's draws: at most
    max(3, 0.005 visits) visits a chain where the two disagree, each already held to Replay.visit's own tolerance"""
    c = MIXED[case]
    N, K, nsweeps, nchains = c["N"], c["K"], c["nsweeps"], len(c["betas"])
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=600 + K, mask_col=2)
    rfeats = H.replay_features(feats, masks)
    rng = np.random.default_rng(K)
    z0 = rng.integers(0, min(K, 12) - 2, (nchains, N)).astype(np.int32)
    z0[1, ::5] = -1
    ens = H.ensemble(gpu_ctx, feats, K, nchains, alpha=1.3)
    ens.assign(view, z0)
    beta32 = np.asarray(c["betas"], dtype=np.float32)
    order = None
    if c["ordered"]:                                  # an order of its own for half the chains, ascending for the rest
        order = np.tile(np.arange(N, dtype=np.int32), (nchains, 1))
        for ch in range(0, nchains, 2):
            order[ch] = rng.permutation(N)
    seeds = [100 + 7 * ch for ch in range(nchains)]
    tr = ens.sweep(view, nsweeps, seeds, sweep=3, trace_every=1, beta=_dev(gpu_ctx, beta32, np.float32),
                   order=None if order is None else _dev(gpu_ctx, order, np.int32)).cpu().numpy()
    assert np.array_equal(tr[:, -1], ens.z.cpu().numpy())
    gpu_ctx.synchronize()
    ens.close()
    for ch in range(nchains):
        n_off = _replay_chain(rfeats, K, 1.3, z0[ch], beta32[ch], tr[ch], seeds[ch], 3,
                              None if order is None else order[ch])
        print("%s chain %d beta %.4f: %d of %d visits off the replay's draw" % (case, ch, beta32[ch], n_off, nsweeps * N))
        assert n_off <= max(3, 0.005 * nsweeps * N), (ch, n_off)


# ---- 4. a call cut into launches, and temperatures changed on the device -------------------------------------------------------
def test_calls_cut_into_launches_and_temperatures_swapped_on_the_device(gpu_ctx):
    N, K, nchains = 120, 12, 4
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=77, mask_col=2)
    rfeats = H.replay_features(feats, masks)
    z0 = np.random.default_rng(3).integers(0, K - 3, (nchains, N)).astype(np.int32)
    beta32 = np.asarray([1.0, 0.3, 0.0, 1.7], dtype=np.float32)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    starts = _assigned(ens, view, z0)
    twin = _twin_of(gpu_ctx, feats, K, nchains, view, z0, starts)
    bt = _dev(gpu_ctx, beta32, np.float32)
    tr = ens.sweep(view, 4, 900, sweep=6, trace_every=1, beta=bt).cpu().numpy()
    parts = [twin.sweep(view, 1, 900, sweep=6 + k, trace_every=1, beta=bt).cpu().numpy() for k in range(4)]
    assert tr.tobytes() == np.concatenate(parts, axis=1).tobytes()
    assert H.ensemble_bits(ens) == H.ensemble_bits(twin)
    # chains 1 and 3 swap their temperatures by torch ops on the device, between two calls and with no wait in between
    z_mid = ens.z.cpu().numpy()
    first = ens.sweep(view, 1, 900, sweep=10, trace_every=1, beta=bt)
    idx = torch.tensor([0, 3, 2, 1], device=gpu_ctx.torch_device)
    bt.copy_(bt[idx])
    second = ens.sweep(view, 1, 900, sweep=11, trace_every=1, beta=bt)
    first, second = first.cpu().numpy(), second.cpu().numpy()
    swapped = beta32[[0, 3, 2, 1]]
    assert bt.cpu().numpy().tobytes() == swapped.tobytes()
    for ch in range(nchains):
        n_off = _replay_chain(rfeats, K, 1.0, z_mid[ch], beta32[ch], first[ch], 900 + ch, 10)
        n_off += _replay_chain(rfeats, K, 1.0, first[ch, -1], swapped[ch], second[ch], 900 + ch, 11)
        assert n_off <= max(3, 0.005 * 2 * N), (ch, n_off)
    # ... and the swap is seen: at its old temperature chain 1's second sweep is another one
    twin.sweep(view, 1, 900, sweep=10, beta=_dev(gpu_ctx, beta32, np.float32))
    old = twin.sweep(view, 1, 900, sweep=11, trace_every=1, beta=_dev(gpu_ctx, beta32, np.float32)).cpu().numpy()
    assert np.array_equal(old[0], second[0]) and np.array_equal(old[2], second[2])
    assert not np.array_equal(old[1], second[1]) and not np.array_equal(old[3], second[3])
    gpu_ctx.synchronize()
    ens.close()
    twin.close()


# ---- 5. run_tempered is its calls -------------------------------------------------------------------------------------------------
def test_run_tempered_is_its_calls(gpu_ctx):
    import common_amd
    from common_amd import tempering as T
    N, K, R, nl = 40, 10, 4, 2
    nchains, dev = R * nl, gpu_ctx.torch_device
    feats, masks, view = H.data(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], N, K, seed=55)
    betas = T.ladder(R, "linear")
    z0 = np.random.default_rng(9).integers(0, 4, (nchains, N)).astype(np.int32)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    starts = _assigned(ens, view, z0)
    hand, nine = (_twin_of(gpu_ctx, feats, K, nchains, view, z0, starts) for _ in range(2))
    seed, sweep0, niters, every = 321, 4, 6, 2
    res = ens.run_tempered(view, niters, seed, betas, sweep=sweep0, trace_every=every)
    assert isinstance(res, T.TemperedResult)
    # the four calls by hand
    beta = _dev(gpu_ctx, np.tile(betas, nl), np.float32)
    rung = _dev(gpu_ctx, np.tile(np.arange(R), nl), np.int32)
    prop, acc = (torch.zeros((nl, R - 1), dtype=torch.int32, device=dev) for _ in range(2))
    joint = torch.empty((nchains, len(feats) + 3), dtype=torch.float64, device=dev)
    trace = torch.empty((nchains, niters // every, N), dtype=torch.int32, device=dev)
    rungs = torch.empty((nchains, niters // every), dtype=torch.int32, device=dev)
    for i in range(niters):
        s = sweep0 + i
        hand.sweep(view, 1, seed, sweep=s, beta=beta)
        hand.score_joint(out=joint)
        if (i + 1) % every == 0:
            trace[:, (i + 1) // every - 1].copy_(hand.z)
            rungs[:, (i + 1) // every - 1].copy_(rung)
        hand.exchange(joint, beta, rung, R, parity=s, seed=T.exchange_key(seed), sweep=s, counters=(prop, acc))
    for name, want in (("trace", trace), ("rungs", rungs), ("beta", beta), ("rung", rung), ("proposed", prop),
                       ("accepted", acc), ("joint", joint)):
        got = getattr(res, name)
        assert got.dtype == want.dtype and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), name
    assert ens.z.cpu().numpy().tobytes() == hand.z.cpu().numpy().tobytes()
    assert int(res.proposed.sum()) == nl * sum(1 for i in range(niters) for j in range(R - 1) if j % 2 == (sweep0 + i) % 2)
    assert int(res.accepted.sum()) > 0 and not np.array_equal(res.rung.cpu().numpy(), np.tile(np.arange(R), nl))
    # a continued run is the long run
    before = [t.clone() for t in (res.beta, res.rung, res.proposed, res.accepted)]
    more = ens.run_tempered(view, 3, seed, betas, sweep=sweep0 + niters, trace_every=1, state=res)
    for a, b in zip(before, (res.beta, res.rung, res.proposed, res.accepted)):
        assert torch.equal(a, b)                                       # (the earlier result is left as it was)
    whole = nine.run_tempered(view, 9, seed, betas, sweep=sweep0, trace_every=1)
    for name in ("beta", "rung", "proposed", "accepted", "joint"):
        assert getattr(more, name).cpu().numpy().tobytes() == getattr(whole, name).cpu().numpy().tobytes(), name
    assert more.trace.cpu().numpy().tobytes() == whole.trace[:, 6:].contiguous().cpu().numpy().tobytes()
    assert more.rungs.cpu().numpy().tobytes() == whole.rungs[:, 6:].contiguous().cpu().numpy().tobytes()
    assert H.ensemble_bits(ens) == H.ensemble_bits(nine)
    # the z-matrix takes the cold samples
    zm_a, zm_b = common_amd.ZMatrix(gpu_ctx, N, K), common_amd.ZMatrix(gpu_ctx, N, K)
    r2 = ens.run_tempered(view, 4, seed, betas, sweep=40, zmatrix=zm_a)
    assert tuple(r2.trace.shape) == (nchains, 4, N)                     # (trace_every defaulted to 1)
    cold = T.cold_samples(r2.trace, r2.rungs)
    assert tuple(cold.shape) == (nl * 4, N)                             # (one chain a ladder holds rung 0 at any time)
    zm_b.add(cold)
    assert zm_a.nsamples == zm_b.nsamples == nl * 4
    counts = zm_a.counts().cpu().numpy()
    assert counts.tobytes() == zm_b.counts().cpu().numpy().tobytes() and counts[0, 0] == nl * 4
    with pytest.raises(ValueError):
        ens.run_tempered(view, 1, seed, T.ladder(3))                    # 8 chains are no ladders of 3
    gpu_ctx.synchronize()
    for e in (zm_a, zm_b, ens, hand, nine):
        e.close()


# ---- 6. the sampler reaches every rung's exact target -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_rows():
    out = {}
    for name, feats in H.six_row_datasets().items():
        rfeats = H.replay_features(feats)
        out[name] = (feats, TH.PartitionTable(rfeats, ALPHA6), H.exact_log_evidence(rfeats, ALPHA6))
    return out


def _six_row_ensemble(gpu_ctx, feats, nchains):
    import common_amd
    view = common_amd.DataView.from_recarray(gpu_ctx, H.recarray_of(feats))
    return view, H.ensemble(gpu_ctx, feats, K6, nchains, alpha=ALPHA6)


@pytest.mark.parametrize("name", sorted(TH.LADDERS))
def test_replica_exchange_reaches_every_rungs_exact_target(gpu_ctx, six_rows, name):
    """64 ladders, 1 000 iterations after 100 of burn-in: per rung, the partitions of the samples taken under that rung
    against the exact pi_beta at the float32 beta: TV <= 0.05 and KL <= 0.01 (temper_helpers' gates), on ladders whose
    rungs' targets are >= 0.10 apart, so a sweep that ignored beta could not pass.
    The numpy sampler replica_exchange_np, run on the CPU at exactly these sizes with seeds 7, 8 and 9, gave per-rung TV
    0.014 - 0.020 and KL 0.0014 - 0.0018 on both datasets and acceptance 0.72 - 0.82: the gates leave 2.5 x room over
    the sampling noise."""
    feats, table, _ = six_rows[name]
    betas = TH.LADDERS[name]
    R, nl, burn, niters = len(betas), 64, 100, 1000
    sep = TH.rung_separation(table, betas)
    assert sep >= TH.MIN_RUNG_TV, (name, sep)
    view, ens = _six_row_ensemble(gpu_ctx, feats, nl * R)
    ens.seat(view)
    warm = ens.run_tempered(view, burn, 4100, betas, sweep=0)
    res = ens.run_tempered(view, niters, 4100, betas, sweep=burn, trace_every=1, state=warm)
    trace, rungs = res.trace.cpu().numpy(), res.rungs.cpu().numpy()
    prop = res.proposed.cpu().numpy().astype(np.int64) - warm.proposed.cpu().numpy()
    acc = res.accepted.cpu().numpy().astype(np.int64) - warm.accepted.cpu().numpy()
    gpu_ctx.synchronize()
    ens.close()
    assert trace.shape == (nl * R, niters, 6) and rungs.shape == (nl * R, niters)
    assert (rungs == 0).sum() == nl * niters
    for j, b in enumerate(betas):
        freq = sh.partition_frequencies(trace[rungs == j], table.parts)
        tv, kl = sh.tv_kl(freq, table.posterior(np.float32(b)))
        print("%s rung %d beta %.4f: TV %.4f KL %.5f" % (name, j, b, tv, kl))
        assert tv <= TH.GATE_TV and kl <= TH.GATE_KL, (name, j, tv, kl)
    rate = acc.sum(0) / prop.sum(0)
    print("%s: smallest exact TV between two rungs %.3f, acceptance %s" % (name, sep, rate))
    assert np.all((rate > 0) & (rate < 1)), rate
    held = np.stack([(rungs == j).any(1) for j in range(R)], 1)
    assert held.all(), np.argwhere(~held)[:5]


# ---- 7. AIS gives the exact evidence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TH.LADDERS))
def test_annealed_importance_sampling_gives_the_exact_evidence(gpu_ctx, six_rows, name):
    """1 024 chains, 33 linear temperatures, one sweep each: |log_evidence - exact| <= 5 se + 1e-4, the gate of
    tests/test_temper_cpu.py, which ais_np passed on the CPU at T = 9, 17 and 33"""
    from common_amd import tempering as T
    feats, _, exact = six_rows[name]
    view, ens = _six_row_ensemble(gpu_ctx, feats, 1024)
    r = ens.ais(view, np.linspace(0.0, 1.0, 33), 7700, sweeps_per_temp=1)
    assert isinstance(r, T.AISResult)
    se = H.evidence_se(r.weights)
    print("AIS %s: exact %.5f, estimate %.5f, se %.5f, t %.2f, ess %.1f" % (name, exact, r.log_evidence, se,
                                                                           (r.log_evidence - exact) / se, r.ess))
    assert r.log_weights.shape == (1024,) and np.isfinite(r.log_weights).all()
    assert r.log_weights.tobytes() == ens.logw.cpu().numpy().tobytes()
    assert abs(r.weights.sum() - 1.0) < 1e-12 and 1.0 <= r.ess <= 1024.0
    assert abs(r.log_evidence - exact) <= 5 * se + 1e-4, (name, r.log_evidence, exact, se)
    assert r.truncated is False                                          # K = 7 > N = 6
    gpu_ctx.synchronize()
    ens.close()


def test_ais_reports_truncation(gpu_ctx):
    """K = 2 slots for six rows under alpha = 1: some chain ends some sweep with both occupied"""
    import common_amd
    feats = H.six_row_datasets()["bb"]
    view = common_amd.DataView.from_recarray(gpu_ctx, H.recarray_of(feats))
    ens = H.ensemble(gpu_ctx, feats, 2, 8, alpha=1.0)
    r = ens.ais(view, [0.0, 0.5, 1.0], 5)
    assert r.truncated is True and np.isfinite(r.log_evidence)
    gpu_ctx.synchronize()
    ens.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_a_temperature_that_is_none_stops_its_chain_alone(gpu_ctx):
    """NaN at chain 1, -0.5 at chain 3: the kernel leaves those two chains as they were and reports them through the
    device error word -- nothing faults; the next call raises, the one after is clean"""
    import common_amd
    N, K, nchains = 60, 8, 5
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=88, mask_col=2)
    z0 = np.random.default_rng(4).integers(0, K - 2, (nchains, N)).astype(np.int32)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    _assigned(ens, view, z0)
    before = H.ensemble_bits(ens)
    beta = _dev(gpu_ctx, [1.0, float("nan"), 0.5, -0.5, 0.0], np.float32)
    tr = ens.sweep(view, 2, 50, sweep=1, trace_every=1, beta=beta)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()                                             # the next library call: it waits, then reads the word
    assert e.value.code == -6 and "msc_chains_sweep_tempered" in str(e.value)
    assert "detail of the first: 1]" in str(e.value) or "detail of the first: 3]" in str(e.value)
    ens.score_joint()                                                     # (reported once: the call after it is clean)
    gpu_ctx.synchronize()
    after = H.ensemble_bits(ens)
    zb = np.frombuffer(before[0], dtype=np.int32).reshape(nchains, N)
    za = np.frombuffer(after[0], dtype=np.int32).reshape(nchains, N)
    for c in range(nchains):
        if c in (1, 3):
            assert np.array_equal(za[c], zb[c]) and after[2][c] == before[2][c], c
        else:
            assert not np.array_equal(za[c], zb[c]) and after[2][c] != before[2][c], c
            assert np.array_equal(tr[c, -1].cpu().numpy(), za[c])
    ens.sweep(view, 1, 50, sweep=3, beta=1.0)                             # the ensemble goes on
    gpu_ctx.synchronize()
    ens.close()


def test_arguments(gpu_ctx):
    import common_amd
    lib, dev = gpu_ctx.lib, gpu_ctx.torch_device
    N, K, nchains = 30, 6, 3
    feats, masks, view = H.data(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], N, K, seed=21)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    ens.assign(view, np.random.default_rng(1).integers(0, K, (nchains, N)).astype(np.int32))
    ens.sweep(view, 1, 8)
    gpu_ctx.synchronize()
    before = H.ensemble_bits(ens)
    seeds = (C.c_uint64 * nchains)(8, 9, 10)
    beta = torch.ones(nchains, dtype=torch.float32, device=dev)

    def raw(beta_ptr, nsweeps=1, nrows=N, trace_every=0, occupied=None):
        return lib.msc_chains_sweep_tempered(ens._h, view._h, None, 0, nrows, 0, C.c_void_p(ens.z.data_ptr()),
                                             int(ens.z.stride(0)), None, 0, nsweeps, seeds, 1, beta_ptr, trace_every, None,
                                             occupied)

    assert raw(None) == -1 and "beta_dev" in lib.msc_last_error().decode()            # MSC_EINVAL, nothing launched
    assert raw(None, nsweeps=0) == 0 and raw(None, nrows=0) == 0                       # no visit to make: no beta needed
    occ = torch.zeros((nchains, 1), dtype=torch.int32, device=dev)
    assert raw(C.c_void_p(beta.data_ptr()), trace_every=0, occupied=C.c_void_p(occ.data_ptr())) == -1
    assert raw(C.c_void_p(beta.data_ptr()), nrows=N + 1) == -1                         # what msc_chains_sweep refuses
    gpu_ctx.synchronize()
    assert H.ensemble_bits(ens) == before
    for bad in (torch.ones(nchains, dtype=torch.float64, device=dev), torch.ones(nchains + 1, dtype=torch.float32, device=dev),
                torch.ones(nchains - 1, dtype=torch.float32, device=dev), torch.ones((nchains, 1), dtype=torch.float32, device=dev),
                torch.ones(nchains, dtype=torch.float32), [1.0] * (nchains + 1), np.ones((2, nchains), dtype=np.float32)):
        with pytest.raises(ValueError):
            ens.sweep(view, 1, 8, beta=bad)
    gpu_ctx.synchronize()
    assert H.ensemble_bits(ens) == before
    assert raw(C.c_void_p(beta.data_ptr())) == 0                                       # a good call goes through
    gpu_ctx.synchronize()
    assert H.ensemble_bits(ens) != before
    ens.close()
