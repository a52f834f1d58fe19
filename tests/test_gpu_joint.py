"""GPU: the log joint log p(X, z | hp, alpha) of a state and of every chain of an ensemble (msc_score_joint /
msc_chains_score_joint / msc_chains_keep_best, State.score_joint, ChainEnsemble.score_joint, chains.JointTracker).

The parts are held to the oracle's double twin fed the suff-stats downloaded from the device, with the gates of
tests/test_gpu_hp_grid.py (1e-8 (sum |per-slot term| + 1) for a sum of score_data, 1e-8 max(1, |want|) for
score_assignment); the total to the written-order sum of the downloaded parts, exactly; the ensemble's rows to the
single-state call, byte for byte; the tracker to a hand loop of the same calls, byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import smc_helpers as H
from tests.gpu_helpers import audit, distinct_hp, make_feature, random_hp, recarray_of
from tests.test_gpu_hp_grid import FAMILIES, _records, _ss64

pytestmark = pytest.mark.gpu

MIX = [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 7), (orc.NICH, 0)]
EXACT = [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 7), (orc.BB, 0)]     # integer statistics only


def _written_order(row):
    """(((a + d_0) + d_1) + ... + d_{F-1}) + p of a downloaded row, in double"""
    t = row[1]
    for d in row[2:-1]:
        t = t + d
    return t + row[-1]


def _held(st, f):
    fam, dim = st.features[f]
    return orc.widen_ss(fam, st.get_ss(f).astype(orc.ss_dtype(fam, dim, "f32")), dim)


def _per_slot(st, f, counted):
    """the double twin's score_data of feature f's counted slots, from the suff-stats downloaded from the device"""
    fam, dim = st.features[f]
    if not counted.any():
        return np.zeros(0)
    return orc.Family(fam, st.get_hp(f), dim, "f64").score_data_all(_held(st, f)[counted])


def _check_parts(st, row, counted=None, name="joint"):
    """a downloaded row of st against the twin -> the sum of |per-slot term| over all features"""
    cnt = st.get_group_counts()
    counted = cnt > 0 if counted is None else counted
    mag = 0.0
    for f in range(len(st.features)):
        per = _per_slot(st, f, counted)
        audit(name + ".score_data_sum", abs(row[2 + f] - float(per.sum())), 1e-8 * (np.abs(per).sum() + 1.0))
        mag += float(np.abs(per).sum())
    want = orc.score_assignment(np.repeat(np.arange(st.K), cnt), float(st.get_alpha()))
    audit(name + ".score_assignment", abs(row[1] - want) / max(1.0, abs(want)), 1e-8)
    assert row[0] == _written_order(row)
    return mag


@pytest.mark.parametrize("family,dim", FAMILIES)
@pytest.mark.parametrize("K", [1, 37, 300])
def test_parts_match_the_double_twin(gpu_ctx, family, dim, K):
    import common_amd
    rng = np.random.default_rng(2000 * family + K)
    empty = rng.random(K) < 0.3
    if K > 1:
        empty[0] = True                              # (bbnc: the invalid p sits in slot 0)
    else:
        empty[0] = False
    rec, n = _records(family, dim, K, rng, empty)
    st = common_amd.State(gpu_ctx, [(family, dim)], K)
    st.set_hp(0, distinct_hp(family, dim))
    st.set_alpha(1.75)
    st.set_ss(0, rec)
    st.set_group_counts(n)
    row = st.score_joint().cpu().numpy()
    assert row.shape == (4,) and row.dtype == np.float64 and np.all(np.isfinite(row))
    _check_parts(st, row)
    assert row[3] == 0.0                             # no priors given
    per = orc.Family(family, st.get_hp(0), dim, "f64").score_data_all(_ss64(family, dim, rec)[n > 0])
    audit("joint.score_data_sum_host_records", abs(row[2] - float(per.sum())), 1e-8 * (np.abs(per).sum() + 1.0))
    again = st.score_joint().cpu().numpy()
    assert again.tobytes() == row.tobytes()
    # a caller's mask: some empty slots counted, some occupied ones not, slot 0 (bbnc's invalid p) excluded
    mask = rng.random(K) < 0.6
    mask[0] = False
    mrow = st.score_joint(slots=torch.from_numpy(mask.astype(np.uint8)).to(gpu_ctx.torch_device)).cpu().numpy()
    assert np.all(np.isfinite(mrow))
    _check_parts(st, mrow, counted=mask, name="joint.masked")
    assert mrow[1] == row[1]                         # the mask counts slots of the features' sums only
    st.close()


def test_noop_contributes_zero(gpu_ctx):
    import common_amd
    K = 5
    st = common_amd.State(gpu_ctx, [(orc.NOOP, 0), (orc.BB, 0)], K)
    rec, n = _records(orc.BB, 0, K, np.random.default_rng(1), np.zeros(K, bool))
    st.set_ss(1, rec)
    st.set_group_counts(n)
    row = st.score_joint().cpu().numpy()
    assert row[2] == 0.0 and row[3] != 0.0 and row[0] == _written_order(row)
    st.close()


def test_priors_match_the_closed_forms(gpu_ctx):
    import common_amd
    K = 6
    rng = np.random.default_rng(4)
    st = common_amd.State(gpu_ctx, [(orc.BB, 0), (orc.NICH, 0)], K)
    st.set_hp(0, distinct_hp(orc.BB))                # alpha 0.75, beta 2.5
    st.set_hp(1, distinct_hp(orc.NICH))              # mu -1.25, kappa 0.375, sigmasq 2.5, nu 3.5
    st.set_alpha(1.75)
    for f, (fam, dim) in enumerate(st.features):
        rec, n = _records(fam, dim, K, rng, np.zeros(K, bool))
        st.set_ss(f, rec)
    st.set_group_counts(n)
    coords = [
        {"feature": 1, "coord": 3, "prior": "flat"},
        {"feature": "alpha", "prior": "exponential", "a": 0.5},
        {"feature": 1, "coord": 0, "prior": "normal", "a": 0.25, "b": 4.0},
        {"feature": 0, "coord": 0, "prior": "noninf_beta", "partner": 1},
        {"feature": 0, "coord": 1, "prior": "noninf_beta", "partner": 0},
        {"feature": 1, "coord": 2, "prior": "exponential", "a": 2.0, "width": 3.0},
    ]
    terms = [0.0,
             math.log(0.5) - 0.5 * 1.75,
             -0.5 * math.log(2.0 * math.pi * 4.0) - 0.5 * ((-1.25 - 0.25) ** 2) / 4.0,
             -2.5 * math.log(0.75 + 2.5),
             -2.5 * math.log(2.5 + 0.75),
             math.log(2.0) - 2.0 * 2.5]
    base = st.score_joint().cpu().numpy()
    for i in range(len(coords)):                     # each kind alone, then all of them in entry order
        row = st.score_joint(priors=[coords[i]]).cpu().numpy()
        audit("joint.prior_term", abs(row[-1] - terms[i]), 1e-12 * max(1.0, abs(terms[i])))
        assert row[1:-1].tobytes() == base[1:-1].tobytes() and row[0] == _written_order(row)
    row = st.score_joint(priors=coords).cpu().numpy()
    want = 0.0
    for t in terms:
        want += t
    audit("joint.prior_sum", abs(row[-1] - want), 1e-12 * max(1.0, abs(want)))
    assert row[0] == _written_order(row)
    # more entries than one launch carries: the sum goes on in entry order
    many = coords * 30
    row = st.score_joint(priors=many).cpu().numpy()
    want = 0.0
    for _ in range(30):
        for t in terms:
            want += t
    audit("joint.prior_sum_chunked", abs(row[-1] - want), 1e-12 * max(1.0, abs(want)))
    assert row[0] == _written_order(row) and row[1:-1].tobytes() == base[1:-1].tobytes()
    st.close()


def test_gibbs_identity_on_integer_statistics(gpu_ctx):
    """J(r joins k) - J(r nowhere) = log(n_k or alpha) - log(N - 1 + alpha) + sum_f score_value_f(r, k): the number every
    sweep draws from (for bnb less the row's data-only binomial coefficient, see below).  Per-slot terms of the gate: the twin's score_data of every (feature, counted slot) of the state
    with r in k -- the larger of the two sums whose difference is taken."""
    import common_amd
    N, K, alpha, r = 40, 8, 1.75, 11
    rng = np.random.default_rng(12)
    feats = [make_feature(f, N, 6, rng, d, hp=distinct_hp(f, d, i)) for i, (f, d) in enumerate(EXACT)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    z = rng.integers(0, K - 2, N).astype(np.int32)   # slots K - 2 and K - 1 stay empty
    z[r] = -1
    st = common_amd.State(gpu_ctx, EXACT, K)
    for f, ft in enumerate(feats):
        st.set_hp(f, ft["hp"])
    st.set_alpha(alpha)
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    st.accumulate(view, zt)
    cnt = st.get_group_counts()
    assert np.array_equal(cnt, np.bincount(z[z >= 0], minlength=K)) and (cnt == 0).sum() == 2
    j0 = st.score_joint().cpu().numpy()
    _check_parts(st, j0, name="joint.gibbs_base")
    values = [orc.Family(f, st.get_hp(i), d, "f64").score_matrix(_held(st, i), feats[i]["values"][r:r + 1])[0]
              for i, (f, d) in enumerate(EXACT)]
    # bnb's score_data is the marginal up to the data-only term sum_i log C(r + v_i - 1, v_i), which its statistics
    # {count, sum} cannot carry (the reference's definition, family_math.hpp bnb_score_data), while its score_value holds
    # the row's term: the identity holds with that term -- the same for every k -- taken out of score_value
    for i, (f, d) in enumerate(EXACT):
        if f == orc.BNB:
            rr, v = float(feats[i]["hp"]["r"]), float(feats[i]["values"][r])
            values[i] = values[i] - (math.lgamma(rr + v) - math.lgamma(v + 1.0) - math.lgamma(rr))
    for k in range(K):
        st.entity_op(view, r, k, join=True)
        jk = st.score_joint().cpu().numpy()
        mag = _check_parts(st, jk, name="joint.gibbs_joined")
        st.entity_op(view, r, k, join=False)
        want = math.log(cnt[k] if cnt[k] else alpha) - math.log(N - 1 + alpha) + sum(float(v[k]) for v in values)
        audit("joint.gibbs_identity", abs((jk[0] - j0[0]) - want), 2e-8 * (mag + 1.0))
    _check_parts(st, st.score_joint().cpu().numpy(), name="joint.gibbs_left")   # the tables are the twin's again
    st.close()


def _ensemble(gpu_ctx, nchains=5, N=200, K=32, seed=7):
    feats, _, view = H.data(gpu_ctx, MIX, N, K, seed)
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    ens.seat(view, seed=1000 + seed)
    ens.sweep(view, 2, 1000 + seed, sweep=1)
    hrng = np.random.default_rng(seed + 1)
    for st in ens.states:
        st.set_alpha(float(np.float32(hrng.uniform(0.5, 3.0))))
        for f, (fam, dim) in enumerate(MIX):
            st.set_hp(f, random_hp(fam, dim, hrng))
    return ens, view, feats


def test_ensemble_rows_equal_the_single_state_call(gpu_ctx):
    import common_amd
    from common_amd import _lib as L
    ens, view, feats = _ensemble(gpu_ctx)
    priors = [{"feature": "alpha", "prior": "exponential", "a": 1.0},
              {"feature": 4, "coord": 1, "prior": "exponential", "a": 0.5},
              {"feature": 0, "coord": 0, "prior": "noninf_beta", "partner": 1}]
    for pr in (None, priors):
        rows = ens.score_joint(priors=pr).cpu().numpy()
        assert rows.shape == (5, len(MIX) + 3)
        for c, st in enumerate(ens.states):
            assert st.score_joint(priors=pr).cpu().numpy().tobytes() == rows[c].tobytes()
            _check_parts(st, rows[c], name="joint.ensemble")
        assert ens.score_joint(priors=pr).cpu().numpy().tobytes() == rows.tobytes()
        assert len({r.tobytes() for r in rows}) == 5                         # the chains differ
        assert (rows[:, -1] != 0.0).all() == (pr is not None)
    # the launch's width moves no bit: a 2-chain ensemble over the states of chains 0 and 1
    lib = gpu_ctx.lib
    hs = (C.c_void_p * 2)(ens.states[0]._h.value, ens.states[1]._h.value)
    h2 = C.c_void_p()
    L.check(lib.msc_chains_create(hs, 2, C.byref(h2)))
    try:
        out = torch.full((2, len(MIX) + 5), -7.0, dtype=torch.float64, device=gpu_ctx.torch_device)
        arr, n = common_amd.State._joint_priors(priors)
        L.check(lib.msc_chains_score_joint(h2, arr, n, None, 0, C.c_void_p(out.data_ptr()), out.stride(0)))
        got = out.cpu().numpy()
        assert got[:, :len(MIX) + 3].tobytes() == rows[:2].tobytes()
        assert (got[:, len(MIX) + 3:] == -7.0).all()                         # a padded row's tail is not written
    finally:
        lib.msc_chains_destroy(h2)
    # one mask for all chains, and one per chain
    rng = np.random.default_rng(3)
    one = torch.from_numpy((rng.random(ens.K) < 0.6).astype(np.uint8)).to(gpu_ctx.torch_device)
    per = torch.from_numpy((rng.random((5, ens.K)) < 0.6).astype(np.uint8)).to(gpu_ctx.torch_device)
    r_one, r_per = ens.score_joint(slots=one).cpu().numpy(), ens.score_joint(slots=per).cpu().numpy()
    for c, st in enumerate(ens.states):
        assert st.score_joint(slots=one).cpu().numpy().tobytes() == r_one[c].tobytes()
        assert st.score_joint(slots=per[c]).cpu().numpy().tobytes() == r_per[c].tobytes()
    ens.close()


def test_more_chains_than_compute_units(gpu_ctx):
    feats, _, view = H.data(gpu_ctx, [(orc.NICH, 0)], 64, 8, 5)
    ens = H.ensemble(gpu_ctx, feats, 8, 300)
    ens.seat(view, seed=9)
    rows = ens.score_joint().cpu().numpy()
    for c in (0, 1, 150, 299):
        assert ens.states[c].score_joint().cpu().numpy().tobytes() == rows[c].tobytes()
        _check_parts(ens.states[c], rows[c], name="joint.ensemble_wide")
    ens.close()


def test_a_call_leaves_no_trace_in_the_states(gpu_ctx):
    A, view, _ = _ensemble(gpu_ctx, nchains=3, N=120, K=7, seed=21)
    B, _, _ = _ensemble(gpu_ctx, nchains=3, N=120, K=7, seed=21)
    assert H.ensemble_bits(A) == H.ensemble_bits(B)
    for s in range(3):
        A.sweep(view, 1, 40, sweep=10 + s)
        B.sweep(view, 1, 40, sweep=10 + s)
        A.score_joint(priors=[{"feature": "alpha", "prior": "exponential", "a": 1.0}])
        A.states[s].score_joint()
    assert H.ensemble_bits(A) == H.ensemble_bits(B)
    A.close()
    B.close()


def _hp_step(ens):
    from common_amd import hypers, models
    from common_amd.scalar_functions import log_exponential
    by = {orc.BB: models.bb, orc.GP: models.gp, orc.BNB: models.bnb, orc.NICH: models.nich}
    descs = [models.dd(d) if f == orc.DD else by[f] for f, d in MIX]
    return hypers.EnsembleHpSlice(ens, descs, cparam={"alpha": (log_exponential(1.0), 1.0)})


def test_tracker_is_the_calls_made_by_hand(gpu_ctx):
    import common_amd
    A, view, _ = _ensemble(gpu_ctx, nchains=4, N=120, K=7, seed=50)
    B, _, _ = _ensemble(gpu_ctx, nchains=4, N=120, K=7, seed=50)
    D, _, _ = _ensemble(gpu_ctx, nchains=4, N=120, K=7, seed=50)
    ha, hb, hd = _hp_step(A), _hp_step(B), _hp_step(D)
    tracker = common_amd.JointTracker(A, priors=ha)
    assert tracker.best_iter.cpu().tolist() == [-1] * 4 and tracker.joint.shape == (4, 0, len(MIX) + 3)
    res = A.run(view, 12, 60, hp=ha, split_merge=2, trace_every=1, joint=tracker)
    assert res._fields == ("trace", "values")
    # the hand loop: the calls run documents, score_joint after each iteration
    want, ztrace, values = [], [], []
    for i in range(12):
        B.sweep(view, 1, 60, sweep=i)
        B.split_merge(view, 60, sweep=i * 2, nproposals=2)
        hb.step(60, i)
        values.append(hb.last_values.copy())
        ztrace.append(B.z.cpu().numpy().copy())
        want.append(B.score_joint(priors=hb.coords).cpu().numpy())
    want, ztrace = np.stack(want, 1), np.stack(ztrace, 1)
    joint = tracker.joint.cpu().numpy()
    assert joint.shape == (4, 12, len(MIX) + 3) and joint.tobytes() == want.tobytes()
    assert res.trace.cpu().numpy().tobytes() == ztrace.tobytes()
    # run without a tracker returns what the hand loop gives (what it returned before there was one)
    plain = D.run(view, 12, 60, hp=hd, split_merge=2, trace_every=1)
    assert plain.trace.cpu().numpy().tobytes() == ztrace.tobytes()
    assert plain.values.tobytes() == np.stack(values, 1).tobytes() == res.values.tobytes()
    assert H.ensemble_bits(A) == H.ensemble_bits(B) == H.ensemble_bits(D)
    totals = joint[:, :, 0]
    assert np.all(np.isfinite(totals))
    first = totals.argmax(1)                                                 # (numpy: the first of equal maxima)
    assert tracker.best_iter.cpu().numpy().tolist() == first.tolist()
    assert tracker.best_joint.cpu().numpy().tobytes() == totals[np.arange(4), first].tobytes()
    assert tracker.best_z.cpu().numpy().tobytes() == ztrace[np.arange(4), first].tobytes()
    c, zmap, jmap = tracker.map()
    assert jmap == totals.max() and c == int(totals.max(1).argmax()) and np.array_equal(zmap.cpu().numpy(), ztrace[c, first[c]])
    assert tracker.totals().tobytes() == totals.tobytes()
    assert math.isfinite(tracker.rhat()) and math.isfinite(tracker.ess())
    # a second leg continues the numbering; an earlier best it does not beat is kept
    A.run(view, 6, 60, hp=ha, split_merge=2, sweep=12, joint=tracker)
    t2 = tracker.joint.cpu().numpy()[:, :, 0]
    assert t2.shape == (4, 18) and t2[:, :12].tobytes() == totals.tobytes()
    f2 = t2.argmax(1)
    assert tracker.best_iter.cpu().numpy().tolist() == f2.tolist()
    kept = f2 < 12
    assert tracker.best_z.cpu().numpy()[kept].tobytes() == ztrace[np.arange(4), first][kept].tobytes()
    # an unbeatable best: nothing is replaced
    tracker.best_joint.fill_(float("inf"))
    frozen = (tracker.best_iter.clone(), tracker.best_z.clone())
    A.run(view, 2, 60, sweep=18, joint=tracker)
    assert torch.equal(tracker.best_iter, frozen[0]) and torch.equal(tracker.best_z, frozen[1])
    assert bool(torch.isinf(tracker.best_joint).all()) and tracker.joint.shape[1] == 20
    for e in (A, B, D):
        e.close()


def test_tracker_every_third_iteration(gpu_ctx):
    import common_amd
    A, view, _ = _ensemble(gpu_ctx, nchains=3, N=100, K=7, seed=60)
    B, _, _ = _ensemble(gpu_ctx, nchains=3, N=100, K=7, seed=60)
    tracker = common_amd.JointTracker(A, every=3, keep_best=False)
    A.run(view, 12, 5, joint=tracker)
    want = []
    for i in range(12):
        B.sweep(view, 1, 5, sweep=i)
        if (i + 1) % 3 == 0:                         # after iterations 3, 6, 9 and 12
            want.append(B.score_joint().cpu().numpy())
    assert tracker.joint.cpu().numpy().tobytes() == np.stack(want, 1).tobytes()
    assert tracker.best_iter.cpu().tolist() == [-1] * 3                      # keep_best=False keeps nothing
    with pytest.raises(ValueError):
        tracker.map()
    with pytest.raises(ValueError):
        B.run(view, 1, 5, joint=tracker)                                     # another ensemble's tracker
    A.close()
    B.close()


def test_keep_best_ties_and_nan(gpu_ctx):
    """the rule on values the sampler does not produce: a tie (and -0.0 against 0.0) keeps the earlier sample, a NaN
    never wins, +inf beats a finite best, -inf does not beat -inf"""
    ens, view, _ = _ensemble(gpu_ctx, nchains=6, N=50, K=7, seed=70)
    dev, n = gpu_ctx.torch_device, 50
    joint = torch.tensor([[1.5, 9.0], [float("nan"), 9.0], [0.0, 9.0], [float("inf"), 9.0], [float("-inf"), 9.0], [2.0, 9.0]],
                         dtype=torch.float64, device=dev)
    best = torch.tensor([1.5, -1e300, -0.0, 7.0, float("-inf"), 1.0], dtype=torch.float64, device=dev)
    best_z = torch.full((6, n + 3), -5, dtype=torch.int32, device=dev)
    best_iter = torch.full((6,), -1, dtype=torch.int64, device=dev)
    rc = gpu_ctx.lib.msc_chains_keep_best(ens._h, C.c_void_p(joint.data_ptr()), 2, C.c_void_p(ens.z.data_ptr()),
                                          int(ens.z.stride(0)), n, 41, C.c_void_p(best.data_ptr()),
                                          C.c_void_p(best_z.data_ptr()), n + 3, C.c_void_p(best_iter.data_ptr()))
    assert rc == 0
    assert best_iter.cpu().tolist() == [-1, -1, -1, 41, -1, 41]
    b = best.cpu().numpy()
    assert b[0] == 1.5 and b[1] == -1e300 and np.signbit(b[2]) and b[3] == np.inf and b[4] == -np.inf and b[5] == 2.0
    bz, z = best_z.cpu().numpy(), ens.z.cpu().numpy()
    for c in range(6):
        assert np.array_equal(bz[c, :n], z[c] if c in (3, 5) else np.full(n, -5))
        assert (bz[c, n:] == -5).all()
    ens.close()


def test_errors_write_nothing(gpu_ctx):
    import common_amd
    from common_amd import MicroscopesHipError
    ens, view, _ = _ensemble(gpu_ctx, nchains=3, N=100, K=7, seed=80)
    lib, dev, W = gpu_ctx.lib, gpu_ctx.torch_device, len(MIX) + 3
    out = torch.full((3, W), -7.0, dtype=torch.float64, device=dev)
    op = C.c_void_p(out.data_ptr())
    assert lib.msc_chains_score_joint(ens._h, None, 0, None, 0, op, W - 1) == -1           # ld_out too small
    assert lib.msc_chains_score_joint(ens._h, None, 0, None, 0, None, W) == -1             # null output
    assert lib.msc_chains_score_joint(ens._h, None, 2, None, 0, op, W) == -1               # entries, but no list
    assert lib.msc_score_joint(ens.states[0]._h, None, 0, None, None) == -1
    slots = torch.ones((3, 7), dtype=torch.uint8, device=dev)
    assert lib.msc_chains_score_joint(ens._h, None, 0, C.c_void_p(slots.data_ptr()), 6, op, W) == -1   # ld_slots < K
    with pytest.raises(MicroscopesHipError) as e:                                          # dd alphas have no prior entry
        ens.score_joint(priors=[{"feature": 3, "coord": 0}], out=out)
    assert e.value.code == -4
    with pytest.raises(MicroscopesHipError) as e:                                          # a coordinate outside the block
        ens.score_joint(priors=[{"feature": 0, "coord": 2}], out=out)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ens.score_joint(out=torch.zeros((3, W), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        ens.score_joint(out=torch.zeros((2, W), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ens.states[0].score_joint(out=torch.zeros(W - 1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ens.score_joint(priors=[3])
    # a member between sweep_step_begin and commit_reduce: named, refused
    ens.states[1].sweep_step_begin(view, ens.z[1], 1, 0)
    with pytest.raises(MicroscopesHipError) as e:
        ens.score_joint(out=out)
    assert e.value.code == -1 and "state 1" in str(e.value)
    with pytest.raises(MicroscopesHipError) as e:
        ens.states[1].score_joint()
    assert e.value.code == -1
    ens.states[1].commit_reduce()
    # keep_best's shapes
    best = torch.full((3,), -np.inf, dtype=torch.float64, device=dev)
    bz = torch.full((3, 100), -5, dtype=torch.int32, device=dev)
    bi = torch.full((3,), -1, dtype=torch.int64, device=dev)

    def keep(ld_joint=W, ld_z=100, ld_best=100, jp=op, it=0):
        return lib.msc_chains_keep_best(ens._h, jp, ld_joint, C.c_void_p(ens.z.data_ptr()), ld_z, 100, it,
                                        C.c_void_p(best.data_ptr()), C.c_void_p(bz.data_ptr()), ld_best,
                                        C.c_void_p(bi.data_ptr()))
    assert keep(ld_z=99) == -1 and keep(ld_best=99) == -1 and keep(ld_joint=0) == -1 and keep(jp=None) == -1
    assert keep(it=1 << 63) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((bz == -5).all()) and bi.cpu().tolist() == [-1] * 3
    assert bool(torch.isinf(best).all())
    # a niw state is refused
    st = common_amd.State(gpu_ctx, [(orc.BB, 0), (orc.NIW, 2)], 8)
    with pytest.raises(MicroscopesHipError) as e:
        st.score_joint()
    assert e.value.code == -4 and "niw" in str(e.value)
    st.close()
    # and the calls still work afterwards
    assert np.all(np.isfinite(ens.score_joint(out=out).cpu().numpy()))
    ens.close()
