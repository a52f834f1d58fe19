"""GPU: the particle filter over rows (msc_chains_visit, msc_chains_clone, ChainEnsemble.visit / clone / smc) -- a visit's
log predictive against the double replay driven by the device's own draws, with z and the tables the bits a plain sweep
leaves; calls cut anywhere; grids beyond the compute units; clones that are their ancestors bit for bit; the evidence
against the exact log p(X) of six rows, without and with resampling; the driver's bookkeeping; errors.

Figures of the run this was written against (one MI355X) are printed by every test before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests import smc_helpers as H

pytestmark = pytest.mark.gpu

ALPHAS = (1.3, 0.4, 2.0)


def _order(gpu_ctx, N, seed):
    o = np.random.default_rng(seed).permutation(N).astype(np.int32)
    return o, torch.from_numpy(o).to(gpu_ctx.torch_device)


def _check_increments(name, c, rp, order, z_c, logp_c):
    """the visits of one pass of chain c against the replay -> (sum of the wants, sum of the gates, saw every slot full)"""
    wants, gates, full = H.replay_pass(rp, order, z_c)
    err = np.abs(logp_c.astype(np.float64) - wants)
    print("%s chain %d: max |inc - want| / gate = %.3f" % (name, c, float(np.max(err / gates))))
    assert np.all(err <= gates), (name, c, err / gates)
    return wants.sum(), gates.sum(), full


# ---- (V1) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 300])
def test_v1_increments_and_bits(gpu_ctx, K):
    """K = 8: the sliced score path, and the slots fill, so visits with no empty slot (e = -inf) are among them; K = 300:
    the strided path.  A seating pass, then a pass over the assigned rows (the leave-first branch)."""
    N, seeds = 37, [11, 4, 1 << 40]
    # (data seed 444: on the replay's own draws two of the three chains fill all 8 slots for dozens of visits)
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed={8: 444, 300: 700}[K], mask_col=2)
    rfeats = H.replay_features(feats, masks)
    order, order_dev = _order(gpu_ctx, N, K)
    ens, twin = (H.ensemble(gpu_ctx, feats, K, 3, alpha=list(ALPHAS)) for _ in range(2))
    ens.seat(view)
    twin.seat(view)
    replays = [sh.Replay(rfeats, K, a, np.full(N, -1, np.int32)) for a in ALPHAS]
    any_full = False
    for sweep in (0, 1):
        logp = ens.visit(view, 0, N, seeds, sweep=sweep, order=order_dev, want_logp=True)
        twin.sweep(view, 1, seeds, sweep=sweep, order=order_dev)
        # the new outputs move no draw: z and every state's bits are the plain sweep's
        z = ens.z.cpu().numpy()
        assert np.array_equal(z, twin.z.cpu().numpy()), sweep
        assert [H.state_bits(st) for st in ens.states] == [H.state_bits(st) for st in twin.states], sweep
        assert ((z >= 0) & (z < K)).all()
        logp, logw = logp.cpu().numpy(), ens.logw.cpu().numpy()
        assert logp.dtype == np.float32 and logp.shape == (3, N) and np.isfinite(logp).all()
        for c in range(3):
            want, gate, full = _check_increments("V1 K=%d sweep %d" % (K, sweep), c, replays[c], order, z[c], logp[c])
            any_full |= full
            print("   logw %.6f, want %.6f, gate %.2e" % (logw[c], want, gate))
            assert abs(logw[c] - want) <= gate, (c, logw[c], want, gate)
        ens.logw.zero_()
    if K == 8:
        assert any_full, "no visit found every slot occupied: the truncated branch was not exercised"
    ens.close()
    twin.close()


# ---- (V2) ------------------------------------------------------------------------------------------------------------------
def test_v2_cuts_do_not_show(gpu_ctx):
    """one call, two calls ([0, 5) and [5, 37)) and 37 one-position calls: the same bytes everywhere"""
    N, K, seeds = 37, 8, [11, 4, 1 << 40]
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=408, mask_col=2)
    order, order_dev = _order(gpu_ctx, N, 8)
    ens = H.ensemble(gpu_ctx, feats, K, 3, alpha=list(ALPHAS))
    results = []
    for cuts in ([(0, N)], [(0, 5), (5, N - 5)], [(p, 1) for p in range(N)]):
        ens.seat(view)
        logp = torch.full((3, N), float("nan"), dtype=torch.float32, device=gpu_ctx.torch_device)
        for pos0, npos in cuts:
            part = ens.visit(view, pos0, npos, seeds, order=order_dev, want_logp=True)
            made = ~torch.isnan(part)
            assert made[:, pos0:pos0 + npos].all() and int(made.sum()) == 3 * npos      # untouched positions stay NaN
            logp = torch.where(made, part, logp)
        results.append((logp.cpu().numpy().tobytes(),) + H.ensemble_bits(ens))
    assert results[0] == results[1], "two calls differ from one"
    assert results[0] == results[2], "one-position calls differ from one call"
    ens.close()


# ---- (V3) ------------------------------------------------------------------------------------------------------------------
def test_v3_more_chains_than_compute_units(gpu_ctx):
    N, K, nchains = 6, 7, 300
    feats, masks, view = H.data(gpu_ctx, [(orc.BB, 0), (orc.NICH, 0)], N, K, seed=7)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    ens.seat(view)
    logp = ens.visit(view, 0, N, 1000, want_logp=True).cpu().numpy()          # (chain c's key: 1000 + c)
    z, logw = ens.z.cpu().numpy(), ens.logw.cpu().numpy()
    assert ((z >= 0) & (z < K)).all() and np.isfinite(logp).all()
    one = H.ensemble(gpu_ctx, feats, K, 1)
    for c in (0, 255, 256, 299):
        one.seat(view)
        lp1 = one.visit(view, 0, N, [1000 + c], want_logp=True).cpu().numpy()
        assert np.array_equal(one.z.cpu().numpy()[0], z[c]), c
        assert lp1[0].tobytes() == logp[c].tobytes() and one.logw.cpu().numpy().tobytes() == logw[c:c + 1].tobytes(), c
        assert H.state_bits(one.states[0]) == H.state_bits(ens.states[c]), c
    one.close()
    ens.close()


# ---- (C1) ------------------------------------------------------------------------------------------------------------------
def test_c1_clone(gpu_ctx):
    N, K = 37, 16
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=416, mask_col=2)
    ens = H.ensemble(gpu_ctx, feats, K, 4)
    lib = gpu_ctx.lib
    ens.seat(view)
    ens.visit(view, 0, N, [21, 22, 23, 24])
    z = ens.z.cpu().numpy()
    assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[2], z[3])     # distinct keys: distinct particles
    before = H.ensemble_bits(ens)

    def raw(anc):
        return lib.msc_chains_clone(ens._h, (C.c_uint32 * 4)(*anc), C.c_void_p(ens.z.data_ptr()), int(ens.z.stride(0)), N)

    # refused, with every chain's bits unchanged: a source that is itself overwritten; an entry that is no chain
    for bad in ([1, 0, 2, 3], [0, 4, 2, 3]):
        assert raw(bad) == -1
        with pytest.raises(ValueError):
            ens.clone(bad)
        assert H.ensemble_bits(ens) == before
    # the identity changes nothing
    assert raw([0, 1, 2, 3]) == 0
    ens.clone([0, 1, 2, 3])
    assert H.ensemble_bits(ens) == before
    # chains 1 and 3 become 0 and 2
    ens.clone([0, 0, 2, 2])
    z = ens.z.cpu().numpy()
    assert z.tobytes() == np.stack([np.frombuffer(before[0], np.int32).reshape(4, N)[a] for a in (0, 0, 2, 2)]).tobytes()
    bits = [H.state_bits(st) for st in ens.states]
    assert bits[0] == before[2][0] and bits[2] == before[2][2]                   # the sources are as they were
    assert bits[1] == bits[0] and bits[3] == bits[2]
    assert ens.logw.cpu().numpy().tobytes() == before[1]                         # the weights are the caller's
    # a clone's rebuilt tables are its ancestor's: continued under equal keys, the pairs stay identical
    ens.logw.zero_()
    logp = ens.visit(view, 0, N, [5, 5, 9, 9], sweep=1, want_logp=True).cpu().numpy()
    z, logw, bits = ens.z.cpu().numpy(), ens.logw.cpu().numpy(), [H.state_bits(st) for st in ens.states]
    for a, b in ((0, 1), (2, 3)):
        assert np.array_equal(z[a], z[b]) and logp[a].tobytes() == logp[b].tobytes() and logw[a] == logw[b], (a, b)
        assert bits[a] == bits[b], (a, b)
    assert not np.array_equal(z[0], z[2])
    # ... and without the read-back of the states in between (the rebuild is then the next visit's alone)
    ens.clone([0, 0, 0, 0])
    ens.visit(view, 0, N, [7, 7, 7, 7], sweep=2)
    z, bits = ens.z.cpu().numpy(), [H.state_bits(st) for st in ens.states]
    assert all(np.array_equal(z[0], z[c]) and bits[0] == bits[c] for c in (1, 2, 3))
    ens.close()


# ---- (E1), (E2) ------------------------------------------------------------------------------------------------------------
N6, K6, ALPHA6 = 6, 8, 1.0


@pytest.fixture(scope="module")
def six_rows():
    """{name: (features, exact log p(X))} of the two six-row datasets, computed once"""
    return {name: (feats, H.exact_log_evidence(H.replay_features(feats), ALPHA6))
            for name, feats in H.six_row_datasets().items()}


def _six_row_ensemble(gpu_ctx, feats, P):
    import common_amd
    view = common_amd.DataView.from_recarray(gpu_ctx, H.recarray_of(feats))
    return view, H.ensemble(gpu_ctx, feats, K6, P, alpha=ALPHA6)


@pytest.mark.parametrize("name", ["bb", "nich"])
def test_e1_evidence_without_resampling(gpu_ctx, six_rows, name):
    """512 particles, ess_threshold = 0: |log_evidence - exact| <= 5 se + 1e-4, se = std(P w) / sqrt(P) (delta method; the
    1e-4 covers the float scores).  tests/test_smc_cpu.py holds the same filter over the double replay to this gate."""
    feats, exact = six_rows[name]
    view, ens = _six_row_ensemble(gpu_ctx, feats, 512)
    r = ens.smc(view, 2024, ess_threshold=0.0)
    se = H.evidence_se(r.weights)
    print("E1 %s: exact %.5f, estimate %.5f, se %.5f, t %.2f" % (name, exact, r.log_evidence, se,
                                                                  (r.log_evidence - exact) / se))
    assert r.resampled_at == [] and r.ancestors == [] and len(r.ess) == N6
    assert r.truncated is False
    assert abs(r.log_evidence - exact) <= 5 * se + 1e-4
    ens.close()


@pytest.mark.parametrize("name", ["bb", "nich"])
def test_e2_evidence_with_resampling_is_unbiased(gpu_ctx, six_rows, name):
    """16 independent runs of 64 particles, resampled after every 2 rows: the mean of exp(log_evidence - exact) is 1
    within 5 of its standard errors.  A run that forgets to reset the weights, to add log_mean_exp at a checkpoint or
    to clone the tables misses this by orders of magnitude."""
    feats, exact = six_rows[name]
    view, ens = _six_row_ensemble(gpu_ctx, feats, 64)
    logz = []
    for run in range(16):
        r = ens.smc(view, 5000 + 100 * run, block=2, ess_threshold=float("inf"))
        assert r.resampled_at == [2, 4] and len(r.ess) == 3 and not r.truncated
        logz.append(r.log_evidence)
    ratio = np.exp(np.array(logz) - exact)
    sem = ratio.std(ddof=1) / math.sqrt(len(ratio))
    print("E2 %s: mean ratio %.5f, sem %.5f, t %.2f" % (name, ratio.mean(), sem, (ratio.mean() - 1) / sem))
    assert abs(ratio.mean() - 1.0) <= 5 * sem
    ens.close()


# ---- (E3) ------------------------------------------------------------------------------------------------------------------
def test_e3_adaptive_bookkeeping(gpu_ctx):
    import common_amd
    N, K, P = 37, 12, 32
    feats, masks, view = H.data(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0), (orc.GP, 0)], N, K, seed=61)
    order, order_dev = _order(gpu_ctx, N, 62)
    ens = H.ensemble(gpu_ctx, feats, K, P)
    # resampled exactly where the reported ESS is below the threshold (the default block here is one row)
    r = ens.smc(view, 300, order=order_dev, ess_threshold=0.5)
    assert len(r.ess) == N and len(r.ancestors) == len(r.resampled_at)
    assert r.resampled_at == [i + 1 for i, e in enumerate(r.ess[:-1]) if e < 0.5 * P]
    print("E3: %d of %d checkpoints resampled, log evidence %.4f" % (len(r.resampled_at), N - 1, r.log_evidence))
    assert 0 < len(r.resampled_at) < N - 1
    for a in r.ancestors:
        assert a.dtype == np.uint32 and np.array_equal(a[a], a)
    assert np.isfinite(r.log_evidence) and abs(r.weights.sum() - 1.0) < 1e-12
    # never resampling: the weights are what a plain visit of all rows leaves
    r0 = ens.smc(view, 300, order=order_dev, ess_threshold=0.0)
    ens.seat(view)
    ens.visit(view, 0, N, 300, order=order_dev)
    assert r0.log_weights.tobytes() == ens.logw.cpu().numpy().tobytes() and r0.resampled_at == []
    # a final resampling leaves equally weighted particles whose tables are those of their z rows
    rf = ens.smc(view, 300, order=order_dev, ess_threshold=0.5, final_resample=True)
    assert rf.resampled_at[-1] == N and rf.resampled_at[:-1] == r.resampled_at and rf.log_evidence == r.log_evidence
    assert np.array_equal(rf.log_weights, np.zeros(P)) and ens.logw.cpu().numpy().tobytes() == np.zeros(P).tobytes()
    ref = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    for i, f in enumerate(feats):
        ref.set_hp(i, f["hp"])
    for c in range(P):
        ref.accumulate(view, ens.z[c])
        assert np.array_equal(ens.states[c].get_group_counts(), ref.get_group_counts()), c
        for i in range(len(feats)):
            got, want = ens.states[c].get_ss(i), ref.get_ss(i)
            for field in got.dtype.names:
                x, y = got[field].astype(np.float64), want[field].astype(np.float64)
                if np.issubdtype(got.dtype[field].base, np.integer):
                    assert np.array_equal(x, y), (c, i, field)
                else:
                    assert np.all(np.abs(x - y) <= 1e-6 * np.maximum(1.0, np.abs(y))), (c, i, field)
    ref.close()
    # ... and the chains go on from them
    zm = common_amd.ZMatrix(gpu_ctx, N, K)
    zm.add(ens.z)
    ens.sweep(view, 2, 301, zmatrix=zm)
    assert zm.nsamples == 3 * P
    z = ens.z.cpu().numpy()
    assert ((z >= 0) & (z < K)).all()
    zm.close()
    ens.close()


# ---- (X) -------------------------------------------------------------------------------------------------------------------
def test_x_errors_change_nothing(gpu_ctx):
    N, K = 9, 5
    feats, masks, view = H.data(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], N, K, seed=71)
    ens = H.ensemble(gpu_ctx, feats, K, 2)
    with pytest.raises(ValueError):
        ens.visit(view, 0, N, 1)                                   # before assign() / seat()
    with pytest.raises(ValueError):
        ens.clone([0, 0])
    ens.seat(view)
    ens.visit(view, 0, 4, 1)
    before = H.ensemble_bits(ens)
    lib, dev = gpu_ctx.lib, gpu_ctx.torch_device
    seeds = (C.c_uint64 * 2)(1, 2)
    logp = torch.full((2, N), 7.0, dtype=torch.float32, device=dev)

    def raw(pos0, npos, ld_logp):
        return lib.msc_chains_visit(ens._h, view._h, None, 0, N, 0, C.c_void_p(ens.z.data_ptr()), int(ens.z.stride(0)), None,
                                    0, pos0, npos, seeds, 0, C.c_void_p(ens.logw.data_ptr()), C.c_void_p(logp.data_ptr()),
                                    ld_logp)

    assert raw(4, N - 3, N) == -1                                  # pos0 + npos > nrows
    assert raw(N + 1, 0, N) == -1
    assert raw(4, 2, N - 1) == -1                                  # ld_logp < nrows
    assert raw(4, 0, N) == 0                                       # no position: nothing touched
    for args in ((4, N - 3), (-1, 2), (0, -1)):
        with pytest.raises(ValueError):
            ens.visit(view, *args, seed=1)
    assert H.ensemble_bits(ens) == before and bool((logp == 7.0).all())
    ens.visit(view, 4, N - 4, 1)                                   # the ensemble still works
    z = ens.z.cpu().numpy()
    assert ((z >= 0) & (z < K)).all()
    ens.close()
    for call in (lambda: ens.visit(view, 0, N, 1), lambda: ens.clone([0, 1]), lambda: ens.smc(view, 1)):
        with pytest.raises(ValueError):
            call()
