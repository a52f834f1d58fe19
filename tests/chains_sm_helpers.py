"""What the tests of the ensemble's split-merge call (msc_chains_split_merge, tests/test_gpu_chains_splitmerge.py) share:
the clustered data as a view and an ensemble, seeded perturbations of the start, and the gates of the single-state tests
restated for one chain of a call -- a proposal held against its own records (tests/test_gpu_splitmerge.py's
_propose_and_check) and a state held against a fresh accumulate of its z (tests/test_gpu_sequential.py's
_compare_tables).  Yardsticks: tests/sm_helpers.py."""
import math

import numpy as np
import torch

from oracle import oracle as orc
from tests import sm_helpers as smh
from tests.gpu_helpers import TOL, audit, recarray_of, rel_err

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]
SHORT_PLAN = (7, 3, 5, 3, 2)         # proposals per category of sm_helpers.CATEGORIES: 20
RECORD_CASES = {
    "c3_mix": dict(specs=C3_SMALL),
    "masked_mix": dict(specs=C3_SMALL + [(orc.BNB, 0)], masked=True),
    "gp_beyond_table": dict(specs=[(orc.GP, 0)], gp_large=True),
    "dd128": dict(specs=[(orc.DD, 128)]),
    "nich": dict(specs=[(orc.NICH, 0)]),
}
INT_SPECS = [(orc.BB, 0)] * 3 + [(orc.DD, 5), (orc.BNB, 0)]      # integer suff-stats only: no sum depends on its order
NOOP = 5          # common_amd.NOOP: a column the model ignores (make_feature has no such family)


def noop_feature(N, seed):
    return dict(family=NOOP, dim=0, hp=None, values=np.random.default_rng(seed).random(N) < 0.5, np_dtype=np.bool_)


def ensemble(gpu_ctx, feats, K, nchains, alpha):
    import common_amd
    ens = common_amd.ChainEnsemble(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K, nchains, alpha=alpha)
    for st in ens.states:
        for i, f in enumerate(feats):
            if f["family"] != NOOP:
                st.set_hp(i, f["hp"])
    return ens


def perturbed_starts(z0, nchains, seed, groups=6, share=0.05):
    """[nchains, N]: z0 itself, then seeded perturbations of it -- a share of the assigned rows sent to a random one of
    the first `groups` groups (those z0 uses), so no new group appears and an empty slot stays empty"""
    out = [z0.copy()]
    for c in range(1, nchains):
        rng = np.random.default_rng(seed + c)
        z = z0.copy()
        idx = rng.choice(np.nonzero(z0 >= 0)[0], max(1, int(share * len(z0))), replace=False)
        z[idx] = rng.integers(0, groups, len(idx)) + z0[z0 >= 0].min()
        out.append(z)
    return np.stack(out).astype(np.int32)


def setup(gpu_ctx, specs, N, K, seed, nchains, alphas, masked=False, gp_large=False, noop_at=None):
    """sm_helpers.clustered_case as a view and an ensemble of nchains chains -> dict; noop_at: a noop column is put in at
    that index (the move ignores it: no tables, no draws, no score)"""
    import common_amd
    feats, masks, truth, z0 = smh.clustered_case(specs, N, seed, masked, gp_large)
    if noop_at is not None:
        feats.insert(noop_at, noop_feature(N, seed))
        masks.insert(noop_at, None)
    data = recarray_of(feats)
    if masked:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in data.dtype.names])
        for pos in range(len(feats)):
            mask["f%d" % pos] = masks[pos]
        data = np.ma.masked_array(data, mask=mask)
    view = common_amd.DataView.from_recarray(gpu_ctx, data)
    alphas = [float(alphas[c % len(alphas)]) for c in range(nchains)]
    Fs = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"], m) for f, m in zip(feats, masks)
          if f["family"] != NOOP]
    return dict(view=view, ens=ensemble(gpu_ctx, feats, K, nchains, alphas), K=K, N=N, alphas=alphas, feats=feats,
                masks=masks, Fs=Fs, z0=z0, truth=truth, nchains=nchains)


def terms(tabs, feats, masks, rows):
    """the addends of a row's two scores, float64 from the float32 tables: [terms][n, 2]"""
    out = [np.repeat(tabs["logw"].cpu().numpy().astype(np.float64)[None, :], len(rows), axis=0)]
    for i, (f, mask) in enumerate(zip(feats, masks)):
        t = tabs[i].cpu().numpy().astype(np.float64)
        v = f["values"][rows]
        if f["family"] == orc.BB:
            add = np.where(v.astype(bool)[:, None], t[1][None, :], t[0][None, :])
        elif f["family"] in (orc.GP, orc.BNB):
            add = t[0][None, :] + v.astype(np.float64)[:, None] * t[1][None, :]
        elif f["family"] == orc.DD:
            add = t[v.astype(np.int64)]
        else:
            add = t[0][None, :] + t[2][None, :] * (v.astype(np.float64)[:, None] - t[1][None, :]) ** 2
        if mask is not None:
            add = np.where(mask[rows][:, None], 0.0, add)
        out.append(add)
    return out


def check_proposal(s, c, tabs, before, after, lg, ell, cn, seed, sweep, launch_iters, name, row_id0=0):
    """chain c's one proposal of a call held against its own records, gate for gate as the single call is held
    (tests/test_gpu_splitmerge.py _propose_and_check) -> (kind, accepted).  tabs: ens.states[c].split_merge_tables()"""
    K, n, alpha = s["K"], s["N"], s["alphas"][c]
    i, j = smh.anchors(seed, sweep, n)
    assert (int(lg[0]), int(lg[1])) == (i, j)
    gi, gj = int(before[i]), int(before[j])
    occupied = np.bincount(before[(before >= 0) & (before < K)], minlength=K)
    empty = np.nonzero(occupied == 0)[0]
    valid = 0 <= gi < K and 0 <= gj < K
    kind = smh.VOID if not valid or (gi == gj and len(empty) == 0) else smh.SPLIT if gi == gj else smh.MERGE
    assert int(lg[2]) == kind
    if kind == smh.VOID:
        assert np.array_equal(after, before) and (ell == -1).all() and not lg[3:].any()
        assert list(cn) == [0, 0, 0, 0, 1]
        return kind, False
    inS = (before == gi) | (before == gj)
    assert np.array_equal(ell >= 0, inS) and set(np.unique(ell[inS])) <= {0, 1}     # the support of l' is exactly S
    assert ell[i] == 0 and ell[j] == 1
    n0, n1 = int((ell == 0).sum()), int((ell == 1).sum())
    assert (int(lg[3]), int(lg[4])) == (n0, n1)
    S = np.nonzero(inS)[0]
    free = (S != i) & (S != j)
    tm = terms(tabs, s["feats"], s["masks"], S)
    lp = smh.two_way(sum(tm))
    mag = sum(np.maximum(1.0, np.abs(t)).sum(axis=1) for t in tm)
    want_q = float(lp[np.arange(len(S)), ell[S]][free].sum())
    audit("chains_splitmerge_logq_" + name, abs(lg[5] - want_q), 1e-6 * max(1.0, float(mag[free].sum())))
    if kind == smh.SPLIT:
        n_off = 0
        for r, p0, on in zip(S, np.exp(lp[:, 0]), free):
            if not on:
                continue
            u = smh.label_dart(seed, sweep, launch_iters, row_id0 + int(r))
            if int(ell[r]) != (0 if u < p0 else 1):
                assert abs(u - p0) < 1e-5, (r, ell[r], u, p0)
                n_off += 1
        assert n_off <= max(3, 0.005 * int(free.sum())), n_off
    else:
        assert np.array_equal(ell[S], (before[S] == gj).astype(np.int32))
    want_A, amag = smh.log_accept(s["Fs"], alpha, np.nonzero(ell == 0)[0], np.nonzero(ell == 1)[0], kind, float(lg[5]),
                                  float_state=True)
    audit("chains_splitmerge_logA_" + name, abs(lg[6] - want_A), 1e-6 * amag)
    u = smh.accept_dart(seed, sweep)
    accepted = bool(lg[7])
    log_u = math.log(u) if u > 0 else -math.inf
    if accepted != (log_u < lg[6]):
        assert abs(log_u - lg[6]) < 1e-5, (u, lg[6], accepted)
    assert list(cn) == [int(kind == 0), int(kind == 0 and accepted), int(kind == 1), int(kind == 1 and accepted), 0]
    want = before.copy()
    if accepted:
        want[ell == 1] = empty[0] if kind == smh.SPLIT else gi
    assert np.array_equal(after, want)
    return kind, accepted


def compare_tables(gpu_ctx, st, view, z, K):
    """a member state against a fresh State accumulated from its z: integer fields equal, float fields within 1e-6
    max(1, |y|), score_value with and without the CRP prior within TOL (tests/test_gpu_sequential.py _compare_tables)"""
    import common_amd
    fresh = common_amd.State(gpu_ctx, st.features, K)
    for i in range(len(st.features)):
        fresh.set_hp(i, st.get_hp(i))
    fresh.set_alpha(st.get_alpha())
    fresh.accumulate(view, torch.from_numpy(np.ascontiguousarray(z)).to(gpu_ctx.torch_device), reset=True)
    assert np.array_equal(st.get_group_counts(), fresh.get_group_counts())
    for i in range(len(st.features)):
        a, b = st.get_ss(i), fresh.get_ss(i)
        for name in a.dtype.names:
            x, y = a[name].astype(np.float64), b[name].astype(np.float64)
            if np.issubdtype(a.dtype[name].base, np.integer):
                assert np.array_equal(x, y), name
            else:
                assert np.all(np.abs(x - y) <= 1e-6 * np.maximum(1.0, np.abs(y))), name
    for crp in (False, True):
        got = st.score_value(view, crp_prior=crp).cpu().numpy()
        want = fresh.score_value(view, crp_prior=crp).cpu().numpy()
        assert rel_err(got, want).max() <= TOL
    fresh.close()


def _live(st):
    """the features that have suff-stats (all but noop)"""
    return [i for i, (fam, _) in enumerate(st.features) if fam != NOOP]


def state_bits(st):
    """everything a call leaves in a state, as bytes: the group counts and every feature's suff-stats"""
    return [st.get_group_counts().tobytes()] + [st.get_ss(i).tobytes() for i in _live(st)]


def pin_start(ens):
    """accumulate adds its double sums with atomics, in an order that varies from run to run: the start is pinned by
    reading every chain's records back and installing them again (as tests/test_gpu_chains.py does) -> the records"""
    starts = []
    for st in ens.states:
        starts.append((st.get_group_counts(), [st.get_ss(i) for i in _live(st)]))
        install(st, starts[-1])
    return starts


def install(st, start):
    cnt, ss = start
    st.set_group_counts(cnt)
    for i, rec in zip(_live(st), ss):
        st.set_ss(i, rec)


def result_bytes(ens, res):
    """a call's outputs and what it left in the ensemble, as bytes"""
    out = [ens.z.cpu().numpy().tobytes(), res.counters.cpu().numpy().tobytes()]
    for t in (res.log, res.trace, res.proposed):
        out.append(None if t is None else t.cpu().numpy().tobytes())
    for st in ens.states:
        out += state_bits(st)
    return out
