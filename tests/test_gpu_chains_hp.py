"""GPU: the slice step of every chain of an ensemble in one launch (msc_chains_hp_slice, ChainEnsemble.hp_slice / run,
hypers.EnsembleHpSlice) -- held bit for bit against the loop of State.hp_slice calls it replaces, on a twin ensemble of
equal contents: the installed values, the evaluation counts, every hp block and alpha; and, as the probe of the score and
CRP tables the call rebuilds, the float32 log predictives of a visit of every row afterwards and the tables it leaves."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import smc_helpers as H
from tests.gpu_helpers import random_hp

pytestmark = pytest.mark.gpu

MIX = [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 5), (orc.NICH, 0)]
NICH1 = [(orc.NICH, 0)]


def _descs(specs):
    from common_amd import models
    by = {orc.BB: models.bb, orc.GP: models.gp, orc.BNB: models.bnb, orc.NICH: models.nich}
    return [models.dd(d) if f == orc.DD else by[f] for f, d in specs]


def _nich_all():
    """all four nich coordinates (the descriptor's defaults slice two)"""
    from common_amd.scalar_functions import log_exponential, log_normal
    return {"mu": (log_normal(0.0, 4.0), 1.0), "kappa": (log_exponential(1.0), 1.0),
            "sigmasq": (log_exponential(1.0), 1.0), "nu": (log_exponential(0.5), 2.0)}


def _coords(ens, specs, hparams=None):
    from common_amd import hypers
    from common_amd.scalar_functions import log_exponential
    return hypers.EnsembleHpSlice(ens, _descs(specs), hparams=hparams, cparam={"alpha": (log_exponential(1.0), 1.0)}).coords


def _pair(gpu_ctx, specs, N, K, nchains, seed, z=None, same_chains=False):
    """two ensembles of equal contents whose chains differ from each other: each chain seated with its own key and swept
    twice (the sequential kernel: no atomics, so both ensembles hold the same bits), or started from z; then its own
    alpha and its own hp blocks.  same_chains: every chain the same key, alpha and blocks -> (A, B, view)"""
    feats, _, view = H.data(gpu_ctx, specs, N, K, seed)
    pair = []
    for _ in range(2):
        ens = H.ensemble(gpu_ctx, feats, K, nchains)
        if z is None:
            keys = [1000 + seed] * nchains if same_chains else 1000 + seed
            ens.seat(view, seed=keys)
            ens.sweep(view, 2, keys, sweep=1)
        else:
            ens.assign(view, torch.from_numpy(z))
        hrng = np.random.default_rng(seed + 1)
        for st in ens.states:
            if same_chains:
                hrng = np.random.default_rng(seed + 1)
            st.set_alpha(float(np.float32(hrng.uniform(0.5, 3.0))))
            for f, (fam, dim) in enumerate(specs):
                st.set_hp(f, random_hp(fam, dim, hrng))
        pair.append(ens)
    return pair[0], pair[1], view


def _loop(ens, coords, seed, sweep, slots=None):
    """the route the ensemble call replaces: State.hp_slice on every member, chain c under chain_seeds(seed)[c] and its
    own row of a per-chain mask"""
    from common_amd.chains import chain_seeds
    keys = chain_seeds(seed, ens.nchains)
    vals, evs = [], []
    for c, st in enumerate(ens.states):
        m = slots if slots is None or slots.dim() == 1 else slots[c]
        v, e = st.hp_slice(coords, keys[c], sweep, slots=m)
        vals.append(v)
        evs.append(e)
    return np.stack(vals), np.stack(evs)


def _hp_bits(ens):
    return [[st.get_hp(f).tobytes() for f in range(len(st.features))] + [np.float32(st.get_alpha()).tobytes()]
            for st in ens.states]


def _same_step(A, B, coords, seed, sweep, slots=None):
    va, ea = A.hp_slice(coords, seed, sweep=sweep, slots=slots)
    vb, eb = _loop(B, coords, seed, sweep, slots=slots)
    assert va.dtype == np.float32 and ea.dtype == np.uint32 and va.shape == ea.shape == (A.nchains, len(coords))
    assert va.tobytes() == vb.tobytes()
    assert ea.tobytes() == eb.tobytes()
    assert _hp_bits(A) == _hp_bits(B)
    return va, ea


def _same_tables(A, B, view, seed2):
    """a visit of every row by both: the float32 log predictives read the score and CRP tables the step rebuilt"""
    n = int(view.nrows)
    la = A.visit(view, 0, n, seed2, want_logp=True).cpu().numpy()
    lb = B.visit(view, 0, n, seed2, want_logp=True).cpu().numpy()
    assert not np.isnan(la).any()
    assert la.tobytes() == lb.tobytes()
    assert H.ensemble_bits(A) == H.ensemble_bits(B)


@pytest.mark.parametrize("K", [7, 300])
def test_mixed_columns_two_steps(gpu_ctx, K):
    A, B, view = _pair(gpu_ctx, MIX, 200, K, 5, seed=11 + K)
    coords = _coords(A, MIX)
    assert all(c["feature"] != 3 for c in coords) and coords[-1]["feature"] == "alpha"    # dd: no coordinate
    pre = _hp_bits(A)
    v0, _ = _same_step(A, B, coords, 31, 0)
    _same_tables(A, B, view, 77)
    v1, _ = _same_step(A, B, coords, 31, 1)
    _same_tables(A, B, view, 78)
    assert v0.tobytes() != v1.tobytes()
    post = _hp_bits(A)
    for c in range(5):
        assert post[c][3] == pre[c][3]                          # dd's block is nobody's coordinate
        assert all(post[c][f] != pre[c][f] for f in (0, 1, 2, 4, 5))
    assert len({tuple(p) for p in post}) == 5                   # the chains went their own ways
    A.close()
    B.close()


def test_more_workgroups_than_compute_units(gpu_ctx):
    A, B, view = _pair(gpu_ctx, NICH1, 64, 8, 300, seed=5)
    coords = _coords(A, NICH1, hparams=[_nich_all()])
    assert len(coords) == 5
    _same_step(A, B, coords, 9, 3)
    _same_tables(A, B, view, 10)
    A.close()
    B.close()


def test_spill_path_with_per_chain_pointers(gpu_ctx):
    N = K = 4200                                                # counted slots beyond the 4096 staged in LDS
    A, B, view = _pair(gpu_ctx, NICH1, N, K, 2, seed=6, z=np.arange(N, dtype=np.int32))
    coords = _coords(A, NICH1, hparams=[_nich_all()])
    _same_step(A, B, coords, [4, 40], 0)
    _same_tables(A, B, view, 12)
    A.close()
    B.close()


def test_masks_one_for_all_and_one_per_chain(gpu_ctx):
    K, nchains = 7, 4
    A, B, view = _pair(gpu_ctx, MIX, 200, K, nchains, seed=21)
    coords = _coords(A, MIX)
    rng = np.random.default_rng(3)
    one = torch.from_numpy((rng.random(K) < 0.6).astype(np.uint8)).to(gpu_ctx.torch_device)
    per = torch.from_numpy((rng.random((nchains, K)) < 0.6).astype(np.uint8)).to(gpu_ctx.torch_device)
    assert len({bytes(r) for r in per.cpu().numpy()}) > 1
    free = [st.get_hp(4).copy() for st in A.states]
    v_one, _ = _same_step(A, B, coords, 2, 0, slots=one)
    _same_tables(A, B, view, 13)
    v_per, _ = _same_step(A, B, coords, 2, 1, slots=per)
    _same_tables(A, B, view, 14)
    # the masks are read: a step from the same start under no mask installs other values
    C_, D_, _ = _pair(gpu_ctx, MIX, 200, K, nchains, seed=21)
    assert [st.get_hp(4).tobytes() for st in C_.states] == [h.tobytes() for h in free]
    v_none, _ = C_.hp_slice(coords, 2, sweep=0)
    assert v_none.tobytes() != v_one.tobytes()
    for e in (A, B, C_, D_):
        e.close()


def test_seeds(gpu_ctx):
    from common_amd.chains import chain_seeds
    A, B, view = _pair(gpu_ctx, NICH1, 64, 8, 3, seed=8)
    coords = _coords(A, NICH1, hparams=[_nich_all()])
    va, ea = A.hp_slice(coords, 50, sweep=2)                    # an int seed ...
    vb, eb = B.hp_slice(coords, chain_seeds(50, 3), sweep=2)    # ... is the explicit list; and the call repeats itself
    assert chain_seeds(50, 3) == [50, 51, 52]
    assert va.tobytes() == vb.tobytes() and ea.tobytes() == eb.tobytes() and _hp_bits(A) == _hp_bits(B)
    _same_tables(A, B, view, 15)
    A.close()
    B.close()
    # chains started identical end apart under different keys, together under equal ones
    S, T, _ = _pair(gpu_ctx, NICH1, 64, 8, 2, seed=8, same_chains=True)
    assert _hp_bits(S)[0] == _hp_bits(S)[1] and H.state_bits(S.states[0]) == H.state_bits(S.states[1])
    vs, _ = S.hp_slice(coords, [7, 8], sweep=0)
    vt, _ = T.hp_slice(coords, [7, 7], sweep=0)
    assert vs[0].tobytes() != vs[1].tobytes()
    assert vt[0].tobytes() == vt[1].tobytes() == vs[0].tobytes()
    S.close()
    T.close()


def test_non_finite_target_keeps_its_value_and_the_rest_is_installed(gpu_ctx):
    from common_amd import MicroscopesHipError
    A, B, view = _pair(gpu_ctx, MIX, 200, 7, 4, seed=30)
    bad = 2
    # nich mu under an exponential prior at mu = -1: the prior is -inf there (mu's support is every real)
    for ens in (A, B):
        hp = ens.states[bad].get_hp(4)
        hp[0] = -1.0
        ens.states[bad].set_hp(4, hp)
    coords = [c for c in _coords(A, MIX) if c["feature"] != 4]
    coords[2:2] = [{"feature": 4, "coord": 0, "width": 1.0, "prior": "exponential", "a": 1.0},
                   {"feature": 4, "coord": 2, "width": 1.0, "prior": "exponential", "a": 1.0}]
    pre = _hp_bits(A)
    with pytest.raises(MicroscopesHipError) as e:
        A.hp_slice(coords, 5, sweep=0)
    assert e.value.code == -1 and "chain %d" % bad in str(e.value) and "feature 4" in str(e.value)
    assert "coordinate 0" in str(e.value)
    from common_amd.chains import chain_seeds
    for c, st in enumerate(B.states):
        if c == bad:
            with pytest.raises(MicroscopesHipError):
                st.hp_slice(coords, chain_seeds(5, 4)[c], 0)
        else:
            st.hp_slice(coords, chain_seeds(5, 4)[c], 0)
    assert _hp_bits(A) == _hp_bits(B)
    post = _hp_bits(A)
    assert A.states[bad].get_hp(4)[0] == np.float32(-1.0)        # that entry of that chain is unchanged ...
    got = np.frombuffer(post[bad][4], np.float32)
    assert got[2] != np.frombuffer(pre[bad][4], np.float32)[2]   # ... its other entries are installed ...
    for c in range(4):                                           # ... and so is everything else, in every chain
        assert all(post[c][f] != pre[c][f] for f in (0, 1, 2, 5))
        assert post[c][4] != pre[c][4]
    _same_tables(A, B, view, 16)                                 # and the rebuild ran
    A.close()
    B.close()


def test_refusals(gpu_ctx):
    from common_amd import MicroscopesHipError
    A, B, view = _pair(gpu_ctx, MIX, 100, 7, 3, seed=40)
    coords = _coords(A, MIX)
    pre = _hp_bits(A)
    with pytest.raises(MicroscopesHipError) as e:
        A.hp_slice(coords + [{"feature": 3, "coord": 0, "width": 1.0}], 1)
    assert e.value.code == -4
    assert _hp_bits(A) == pre
    dev = gpu_ctx.torch_device
    with pytest.raises(ValueError):
        A.hp_slice(coords, [1, 2])                              # wrong seed count
    with pytest.raises(ValueError):
        A.hp_slice(coords, 1, slots=torch.ones((2, 7), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        A.hp_slice(coords, 1, slots=torch.ones(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        A.hp_slice(coords, 1, slots=torch.ones((3, 7), dtype=torch.int32, device=dev))
    assert _hp_bits(A) == pre
    _same_tables(A, B, view, 17)                                # nothing was left half done
    A.close()
    B.close()
    with pytest.raises(ValueError):
        A.hp_slice(coords, 1)                                   # closed


def test_run_is_the_calls_made_by_hand(gpu_ctx):
    import common_amd
    from common_amd import hypers
    from common_amd.scalar_functions import log_exponential
    A, B, view = _pair(gpu_ctx, MIX, 120, 7, 3, seed=50)
    n = int(view.nrows)
    cparam = {"alpha": (log_exponential(1.0), 1.0)}
    ha = hypers.EnsembleHpSlice(A, _descs(MIX), cparam=cparam)
    hb = hypers.EnsembleHpSlice(B, _descs(MIX), cparam=cparam)
    zm = common_amd.ZMatrix(gpu_ctx, n, 7)
    res = A.run(view, 3, 60, hp=ha, sweep=4, zmatrix=zm)
    trace, values = [], []
    for i in range(3):
        B.sweep(view, 1, 60, sweep=4 + i)
        trace.append(B.z.cpu().numpy().copy())
        out = hb.step(60, 4 + i)
        values.append(hb.last_values.copy())
        assert len(out) == 3 and set(out[0]) == {0, 1, 2, 4, "alpha"}
        for c in range(3):
            assert out[c]["alpha"] == B.states[c].get_alpha()
            assert np.float32(out[c][4]["sigmasq"]) == B.states[c].get_hp(4)[2]
    assert hb.last_evals.shape == (3, len(hb.coords)) and hb.last_evals.dtype == np.uint32
    assert res.trace.shape == (3, 3, n) and res.trace.dtype == torch.int32 and res.values.shape == (3, 3, len(ha.coords))
    assert res.trace.cpu().numpy().tobytes() == np.stack(trace, axis=1).tobytes()
    assert res.values.tobytes() == np.stack(values, axis=1).astype(np.float32).tobytes()
    assert H.ensemble_bits(A) == H.ensemble_bits(B) and _hp_bits(A) == _hp_bits(B)
    assert zm.nsamples == 9
    # thinned, and without an hp step: the sweeps alone
    r2 = A.run(view, 3, 61, sweep=9, trace_every=2)
    B.sweep(view, 2, 61, sweep=9)
    z1 = B.z.cpu().numpy().copy()
    B.sweep(view, 1, 61, sweep=11)
    assert r2.trace.shape == (3, 1, n) and r2.trace[:, 0].cpu().numpy().tobytes() == z1.tobytes()
    assert r2.values.shape == (3, 3, 0)
    assert H.ensemble_bits(A) == H.ensemble_bits(B)
    assert A.run(view, 2, 62, sweep=20).trace is None
    zm.close()
    A.close()
    B.close()
