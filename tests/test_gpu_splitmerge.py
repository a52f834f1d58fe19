"""GPU: split-merge proposals on the device (msc_split_merge / msc_split_merge_tables) -- every proposal replayed from
its records (anchors, set, labels, log q, log A, the decision, the move, the tables on return), the shapes that take the
other kernels, the exact posterior of six rows, what the move is for, determinism, a full table, and the error cases.
Yardsticks: tests/sm_helpers.py."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests import sm_helpers as smh
from tests.gpu_helpers import audit, recarray_of

pytestmark = pytest.mark.gpu

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]
ALPHA = 1.3
PLAN = (20, 10, 16, 10, 4)           # proposals per category of sm_helpers.CATEGORIES: 60
SHORT_PLAN = (7, 3, 5, 3, 2)         # 20
TINY_PLAN = (4, 1, 3, 1, 1)          # 10

FAMILY_CASES = {
    "bb": dict(specs=[(orc.BB, 0)] * 3),
    "gp": dict(specs=[(orc.GP, 0)]),
    "gp_beyond_table": dict(specs=[(orc.GP, 0)], gp_large=True),
    "bnb": dict(specs=[(orc.BNB, 0)]),
    "dd2": dict(specs=[(orc.DD, 2)]),
    "dd128": dict(specs=[(orc.DD, 128)]),
    "nich": dict(specs=[(orc.NICH, 0)]),
    "c3_mix": dict(specs=C3_SMALL),
    "masked_mix": dict(specs=C3_SMALL + [(orc.BNB, 0)], masked=True),
}


def _state(gpu_ctx, feats, K, alpha):
    import common_amd
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    for i, f in enumerate(feats):
        st.set_hp(i, f["hp"])
    st.set_alpha(alpha)
    return st


def _setup(gpu_ctx, specs, N, K, seed, masked=False, gp_large=False, order=None, alpha=ALPHA):
    """the clustered data of sm_helpers.clustered_case as a view (its columns in `order`), a state, a fresh twin for the
    table comparison, and the replay's features in the state's order"""
    import common_amd
    feats, masks, truth, z0 = smh.clustered_case(specs, N, seed, masked, gp_large)
    order = list(range(len(feats))) if order is None else list(order)
    data = recarray_of([feats[c] for c in order])
    if masked:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in data.dtype.names])
        for pos, c in enumerate(order):
            mask["f%d" % pos] = masks[c]
        data = np.ma.masked_array(data, mask=mask)
    view = common_amd.DataView.from_recarray(gpu_ctx, data)
    cols = None if order == list(range(len(feats))) else [order.index(f) for f in range(len(feats))]
    Fs = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"], m) for f, m in zip(feats, masks)]
    return dict(view=view, st=_state(gpu_ctx, feats, K, alpha), fresh=_state(gpu_ctx, feats, K, alpha), cols=cols, K=K,
                N=N, alpha=alpha, feats=feats, masks=masks, Fs=Fs, z0=z0, truth=truth)


def _terms(tabs, s, rows):
    """the addends of a row's two scores, float64 from the float32 tables: [terms][n, 2]"""
    out = [np.repeat(tabs["logw"].cpu().numpy().astype(np.float64)[None, :], len(rows), axis=0)]
    for i, (f, mask) in enumerate(zip(s["feats"], s["masks"])):
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


def _ss_bits(st):
    out = [st.get_group_counts()]
    for i in range(len(st.features)):
        out.append(st.get_ss(i).view(np.uint8).copy())
    return out


def _einval(call):
    import common_amd
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        call()
    assert e.value.code == -1


def _propose_and_check(gpu_ctx, s, zt, seed, sweep, launch_iters, name, row0=0, nrows=None, row_id0=None, tables=True):
    """one proposal in one call on the rows [row0, row0 + nrows) of zt, held against its records -> (kind, accepted)"""
    dev = gpu_ctx.torch_device
    st, view, K = s["st"], s["view"], s["K"]
    n = s["N"] - row0 if nrows is None else nrows
    rid0 = row0 if row_id0 is None else row_id0
    zr = zt[row0:row0 + n]
    st.accumulate(view, zr, row0=row0, nrows=n, cols=s["cols"])
    st.blocked_draw(1, 0)
    before_all = zt.cpu().numpy()
    before = before_all[row0:row0 + n]
    log = torch.zeros(8, dtype=torch.float64, device=dev)
    prop = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(5, dtype=torch.int64, device=dev)
    st.split_merge(view, zr, seed, sweep, nproposals=1, launch_iters=launch_iters, log=log, proposed=prop, counters=cnt,
                   row0=row0, nrows=n, row_id0=row_id0, cols=s["cols"])
    after_all = zt.cpu().numpy()
    after = after_all[row0:row0 + n]
    lg, ell, cn = log.cpu().numpy(), prop.cpu().numpy(), cnt.cpu().numpy()
    # the anchors and the kind
    i, j = smh.anchors(seed, sweep, n)
    assert (int(lg[0]), int(lg[1])) == (i, j)
    gi, gj = int(before[i]), int(before[j])
    occupied = np.bincount(before[(before >= 0) & (before < K)], minlength=K)
    empty = np.nonzero(occupied == 0)[0]
    valid = 0 <= gi < K and 0 <= gj < K
    kind = smh.VOID if not valid or (gi == gj and len(empty) == 0) else smh.SPLIT if gi == gj else smh.MERGE
    assert int(lg[2]) == kind
    # rows outside the range are never written
    assert np.array_equal(after_all[:row0], before_all[:row0]) and np.array_equal(after_all[row0 + n:], before_all[row0 + n:])
    accepted = False
    if kind == smh.VOID:
        assert np.array_equal(after, before) and (ell == -1).all() and not lg[3:].any()
        assert list(cn) == [0, 0, 0, 0, 1]
    else:
        inS = (before == gi) | (before == gj)
        assert np.array_equal(ell >= 0, inS) and set(np.unique(ell[inS])) <= {0, 1}     # the support of l' is exactly S
        assert ell[i] == 0 and ell[j] == 1
        n0, n1 = int((ell == 0).sum()), int((ell == 1).sum())
        assert (int(lg[3]), int(lg[4])) == (n0, n1)
        S = np.nonzero(inS)[0]
        free = (S != i) & (S != j)
        terms = _terms(st.split_merge_tables(), s, row0 + S)
        lp = smh.two_way(sum(terms))
        mag = sum(np.maximum(1.0, np.abs(t)).sum(axis=1) for t in terms)
        want_q = float(lp[np.arange(len(S)), ell[S]][free].sum())
        audit("splitmerge_logq_" + name, abs(lg[5] - want_q), 1e-6 * max(1.0, float(mag[free].sum())))
        if kind == smh.SPLIT:
            n_off = 0
            for r, p0, on in zip(S, np.exp(lp[:, 0]), free):
                if not on:
                    continue
                u = smh.label_dart(seed, sweep, launch_iters, rid0 + int(r))
                if int(ell[r]) != (0 if u < p0 else 1):
                    assert abs(u - p0) < 1e-5, (r, ell[r], u, p0)
                    n_off += 1
            assert n_off <= max(3, 0.005 * int(free.sum())), n_off
        else:
            assert np.array_equal(ell[S], (before[S] == gj).astype(np.int32))
        # (the oracle scores the state the device keeps: double sums, the float fields rounded to float -- gp's log_prod
        # is tens of thousands where the block's score is hundreds)
        want_A, amag = smh.log_accept(s["Fs"], s["alpha"], row0 + np.nonzero(ell == 0)[0], row0 + np.nonzero(ell == 1)[0],
                                      kind, float(lg[5]), float_state=True)
        audit("splitmerge_logA_" + name, abs(lg[6] - want_A), 1e-6 * amag)
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
    # the state on return: a fresh state's accumulate of the final z, bit for bit; a blocked draw made before is stale
    if tables:
        s["fresh"].accumulate(view, zr, row0=row0, nrows=n, cols=s["cols"], reset=True)
        for a, b in zip(_ss_bits(st), _ss_bits(s["fresh"])):
            assert np.array_equal(a, b)
        assert np.array_equal(st.get_group_counts(), np.bincount(after[(after >= 0) & (after < K)], minlength=K))
    _einval(lambda: st.blocked_assign(view, zr.clone(), 1, 0, row0=row0, nrows=n, cols=s["cols"]))
    return kind, accepted


def _records_run(gpu_ctx, s, plan, seed, name, launch_iters=1, row0=0, nrows=None, row_id0=None):
    """every planned proposal from the start z0, one per call -> {(kind, accepted): count}"""
    n = s["N"] - row0 if nrows is None else nrows
    tally = {}
    for sweep in smh.plan_sweeps(s["z0"][row0:row0 + n], seed, plan, s["truth"][row0:row0 + n]):
        zt = torch.from_numpy(s["z0"].copy()).to(gpu_ctx.torch_device)
        k = _propose_and_check(gpu_ctx, s, zt, seed, sweep, launch_iters, name, row0, nrows, row_id0)
        tally[k] = tally.get(k, 0) + 1
    return tally


@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_records_replay_per_family(gpu_ctx, case):
    """N = 700 (three 256-row workgroups and a ragged tail), K = 12, 60 proposals, one per call, launch_iters = 1; each
    from the start z0, whose group 0 holds two clusters and whose groups 1 and 2 share one"""
    c = FAMILY_CASES[case]
    s = _setup(gpu_ctx, c["specs"], 700, 12, seed=sum(map(ord, case)), masked=c.get("masked", False),
               gp_large=c.get("gp_large", False))
    tally = _records_run(gpu_ctx, s, PLAN, 11, case)
    print("split-merge records %s: %s" % (case, sorted(tally.items())))
    for kind in (smh.SPLIT, smh.MERGE):
        assert tally.get((kind, True), 0) >= 5 and tally.get((kind, False), 0) >= 5, tally
    assert tally.get((smh.VOID, False), 0) <= 0.15 * sum(tally.values())


def test_records_replay_many_slots(gpu_ctx):
    """K = 300 (kpad 512): the empty slot is found beyond the first 256"""
    s = _setup(gpu_ctx, C3_SMALL, 700, 300, seed=300)
    s["z0"] = np.where(s["z0"] >= 0, s["z0"] + 290, -1).astype(np.int32)     # groups 290 .. 295: 0 is the lowest empty slot
    tally = {}
    for sweep in smh.plan_sweeps(np.where(s["z0"] >= 0, s["z0"] - 290, -1), 13, SHORT_PLAN, s["truth"]):
        zt = torch.from_numpy(s["z0"].copy()).to(gpu_ctx.torch_device)
        k = _propose_and_check(gpu_ctx, s, zt, 13, sweep, 1, "k300")
        tally[k] = tally.get(k, 0) + 1
    assert tally.get((smh.SPLIT, True), 0) >= 1 and tally.get((smh.MERGE, True), 0) >= 1, tally
    # with slots 0 .. 255 taken by one row each the lowest empty slot lies in the second half of the count table
    z = s["z0"].copy()
    z[np.nonzero(z >= 293)[0][:256]] = np.arange(256)
    sweep = smh.plan_sweeps(np.where(s["z0"] >= 0, s["z0"] - 290, -1), 13, (1, 0, 0, 0, 0), s["truth"])[0]
    zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
    _propose_and_check(gpu_ctx, s, zt, 13, sweep, 1, "k300")


def test_records_replay_sub_range_and_cols(gpu_ctx):
    """rows [131, 531) of 700 with global ids from 10^6, the view's columns permuted: rows outside the range are never
    anchors and never written"""
    s = _setup(gpu_ctx, C3_SMALL + [(orc.BNB, 0)], 700, 12, seed=41, masked=True, order=[3, 0, 4, 2, 1])
    tally = _records_run(gpu_ctx, s, SHORT_PLAN, 17, "subrange", row0=131, nrows=400, row_id0=10 ** 6)
    assert tally.get((smh.SPLIT, True), 0) >= 1 and tally.get((smh.MERGE, True), 0) >= 1, tally


@pytest.mark.parametrize("nfeat", [40, 70, 300])
def test_records_replay_many_features_takes_the_other_kernels(gpu_ctx, nfeat):
    """40 features: the staged kernel with 128 rows a workgroup; 70: 64 rows; 300: the codes re-read from the columns"""
    s = _setup(gpu_ctx, [(orc.BB, 0)] * (nfeat - 2) + [(orc.NICH, 0), (orc.DD, 5)], 700, 12, seed=nfeat)
    _records_run(gpu_ctx, s, TINY_PLAN, 19, "nfeat%d" % nfeat)
    assert gpu_ctx.last_kernel("sweep").startswith("k_sm_assign<%d," % (0 if nfeat > 256 else 1))


# ---- the chain ---------------------------------------------------------------------------------------------------------
def test_exact_posterior_of_six_rows(gpu_ctx):
    """N = 6, K = 32, alpha = 1, split-merge proposals only from z = 0: 5e4 proposals (launch_iters = 0) visit the 203
    partitions with the exact posterior's frequencies, TV <= 0.05 and KL <= 0.01.  The float64 numpy yardstick
    (sm_helpers.Yardstick, five seeds, the same number of proposals): bb3 TV 0.0205 - 0.0245, KL 0.0036 - 0.0045;
    nich_bb TV 0.0349 - 0.0392, KL 0.0055 - 0.0072 (its own bar: TV <= 0.042, KL <= 0.008)."""
    import common_amd
    dev = gpu_ctx.torch_device
    N, K, alpha, per_call, calls = 6, 32, 1.0, 10000, 5
    for name, feats in smh.six_row_datasets().items():
        Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
        parts, p = sh.exact_posterior([(F, f["values"]) for F, f in zip(Fs, feats)], alpha)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
        st = _state(gpu_ctx, feats, K, alpha)
        zt = torch.zeros(N, dtype=torch.int32, device=dev)
        st.accumulate(view, zt)
        trace = torch.empty(per_call * N, dtype=torch.int32, device=dev)
        cnt = torch.zeros(5, dtype=torch.int64, device=dev)
        traces = []
        for c in range(calls):
            st.split_merge(view, zt, 77, c * per_call, nproposals=per_call, launch_iters=0, trace=trace, counters=cnt)
            traces.append(trace.cpu().numpy().reshape(per_call, N))
        assert np.array_equal(traces[-1][-1], zt.cpu().numpy())
        freq = sh.partition_frequencies(np.concatenate(traces), parts)
        tv, kl = sh.tv_kl(freq, p)
        cn = cnt.cpu().numpy()
        print("exact posterior %s: split-merge TV %.4f KL %.5f, splits %d / %d, merges %d / %d, void %d" %
              (name, tv, kl, cn[1], cn[0], cn[3], cn[2], cn[4]))
        assert cn[0] + cn[2] + cn[4] == per_call * calls and cn[4] == 0
        assert tv <= 0.05 and kl <= 0.01, (name, tv, kl)


def _two_cluster_setup(gpu_ctx):
    import common_amd
    feats, truth = smh.two_cluster_data()
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    return feats, truth, view, _state(gpu_ctx, feats, 8, 1.0)


def test_it_splits_a_group_that_holds_two_clusters(gpu_ctx):
    """two nich clusters at -10 / +10 (sd 1) and a bb column with p = 0.1 / 0.9, N = 1500 in one group, K = 8: after 20
    proposals with launch_iters = 3 the two largest groups hold >= 99 % of the rows and agree with the truth on >= 99 %.
    The nich prior holds the variance at 1 (sm_helpers.two_cluster_data says why).  The float64 numpy yardstick
    (sm_helpers.Yardstick, `python -m tests.sm_helpers`) on five seeds: share 1.0000, agreement 0.9993 - 1.0000."""
    dev = gpu_ctx.torch_device
    feats, truth, view, st = _two_cluster_setup(gpu_ctx)
    zt = torch.zeros(len(truth), dtype=torch.int32, device=dev)
    st.accumulate(view, zt)
    cnt = torch.zeros(5, dtype=torch.int64, device=dev)
    st.split_merge(view, zt, 5, 0, nproposals=20, launch_iters=3, counters=cnt)
    share, agree = smh.two_largest_agree(zt.cpu().numpy(), truth)
    print("two clusters from one group: share %.4f agreement %.4f counters %s" % (share, agree, cnt.cpu().numpy()))
    assert share >= 0.99 and agree >= 0.99, (share, agree)


def test_it_merges_groups_that_hold_one_cluster(gpu_ctx):
    """the same data with each true cluster cut into two groups by hand: after 40 proposals (launch_iters = 3) two groups
    remain (the numpy yardstick: two groups on each of five seeds)"""
    dev = gpu_ctx.torch_device
    feats, truth, view, st = _two_cluster_setup(gpu_ctx)
    z = (2 * truth + (np.arange(len(truth)) % 2)).astype(np.int32)
    zt = torch.from_numpy(z).to(dev)
    st.accumulate(view, zt)
    cnt = torch.zeros(5, dtype=torch.int64, device=dev)
    st.split_merge(view, zt, 5, 100, nproposals=40, launch_iters=3, counters=cnt)
    got = zt.cpu().numpy()
    print("two clusters from four groups: groups %s counters %s" % (np.unique(got, return_counts=True), cnt.cpu().numpy()))
    assert len(np.unique(got)) == 2
    assert smh.two_largest_agree(got, truth) == (1.0, 1.0)


def test_same_arguments_same_bits_and_split_calls(gpu_ctx):
    dev = gpu_ctx.torch_device
    runs = []
    for way in ("one", "one", "ten"):
        s = _setup(gpu_ctx, C3_SMALL, 700, 12, seed=61)
        st, view = s["st"], s["view"]
        zt = torch.from_numpy(s["z0"].copy()).to(dev)
        st.accumulate(view, zt)
        log = torch.zeros(80, dtype=torch.float64, device=dev)
        trace = torch.zeros(10 * 700, dtype=torch.int32, device=dev)
        cnt = torch.zeros(5, dtype=torch.int64, device=dev)
        if way == "one":
            st.split_merge(view, zt, 23, 4, nproposals=10, launch_iters=2, log=log, trace=trace, counters=cnt)
        else:
            for p in range(10):
                st.split_merge(view, zt, 23, 4 + p, nproposals=1, launch_iters=2, log=log[8 * p:8 * p + 8],
                               trace=trace[700 * p:700 * (p + 1)], counters=cnt)
        tabs = {k: t.cpu().numpy().view(np.uint32).copy() for k, t in st.split_merge_tables().items()}
        runs.append((zt.cpu().numpy(), log.cpu().numpy().view(np.uint64), trace.cpu().numpy(), cnt.cpu().numpy(), tabs,
                     _ss_bits(st)))
    assert runs[0][3][:4].sum() + runs[0][3][4] == 10
    for z, lg, tr, cn, tabs, ss in runs[1:]:
        assert np.array_equal(z, runs[0][0]) and np.array_equal(lg, runs[0][1]) and np.array_equal(tr, runs[0][2])
        assert np.array_equal(cn, runs[0][3])
        for k in tabs:
            assert np.array_equal(tabs[k], runs[0][4][k]), k
        for a, b in zip(ss, runs[0][5]):
            assert np.array_equal(a, b)


def test_full_table_voids_every_split_until_a_merge_frees_a_slot(gpu_ctx):
    """K = the number of occupied groups: a split is void, merges run, and the proposal after an accepted merge can split"""
    s = _setup(gpu_ctx, C3_SMALL, 700, 6, seed=71)
    z0 = s["z0"].copy()
    z0[z0 < 0] = 3
    s["z0"] = z0
    assert len(np.unique(z0)) == 6
    dev = gpu_ctx.torch_device
    zt = torch.from_numpy(z0.copy()).to(dev)
    same = smh.plan_sweeps(z0, 29, (2, 2, 0, 0, 0))
    for sweep in same:
        kind, _ = _propose_and_check(gpu_ctx, s, zt, 29, sweep, 1, "full")
        assert kind == smh.VOID
    merged = False
    for sweep in smh.plan_sweeps(z0, 29, (0, 0, 12, 0, 0)):
        kind, merged = _propose_and_check(gpu_ctx, s, zt, 29, sweep, 1, "full")
        assert kind == smh.MERGE
        if merged:
            break
    assert merged
    z1 = zt.cpu().numpy()
    assert len(np.unique(z1)) == 5
    # the next proposal whose anchors share a group is a split now, not void
    sweep = next(sw for sw in range(10 ** 6) if z1[smh.anchors(29, sw, 700)[0]] == z1[smh.anchors(29, sw, 700)[1]])
    kind, _ = _propose_and_check(gpu_ctx, s, zt, 29, sweep, 1, "full")
    assert kind == smh.SPLIT


@pytest.mark.parametrize("spec", [(orc.NIW, 3), (orc.DM, 4), (orc.BBNC, 0)])
def test_unsupported_families(gpu_ctx, spec):
    import common_amd
    from tests.gpu_helpers import make_feature
    rng = np.random.default_rng(81)
    feats = [make_feature(spec[0], 200, 8, rng, spec[1]), make_feature(orc.NICH, 200, 8, rng)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = _state(gpu_ctx, feats, 8, 1.0)
    zt = torch.from_numpy(rng.integers(0, 6, 200).astype(np.int32)).to(gpu_ctx.torch_device)
    st.accumulate(view, zt)
    for call in (lambda: st.split_merge(view, zt, 1, 0), lambda: st.split_merge_tables()):
        with pytest.raises(common_amd.MicroscopesHipError) as e:
            call()
        assert e.value.code == -4


def test_errors(gpu_ctx):
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, C3_SMALL, 700, 12, seed=91)
    st, view = s["st"], s["view"]
    zt = torch.from_numpy(s["z0"].copy()).to(dev)
    st.accumulate(view, zt)
    # between sweep_step_begin and commit_reduce
    zs = torch.from_numpy(np.where(s["z0"] < 0, 0, s["z0"]).astype(np.int32)).to(dev)
    st.accumulate(view, zs)
    st.sweep_step_begin(view, zs, 1, 0)
    _einval(lambda: st.split_merge(view, zs, 1, 0))
    st.commit_reduce()
    st.split_merge(view, zs, 1, 0)
    # a null z
    _einval(lambda: st.split_merge(view, None, 1, 0))
    # fewer than two rows: every proposal is void and nothing moves
    for n in (0, 1):
        log = torch.full((24,), -1.0, dtype=torch.float64, device=dev)
        cnt = torch.zeros(5, dtype=torch.int64, device=dev)
        before = zt.clone()
        st.split_merge(view, zt[5:], 1, 0, nproposals=3, log=log, counters=cnt, row0=5, nrows=n)
        lg = log.cpu().numpy().reshape(3, 8)
        assert (lg[:, 2] == smh.VOID).all() and not lg[:, 3:].any()
        assert list(cnt.cpu().numpy()) == [0, 0, 0, 0, 3]
        assert torch.equal(before, zt)
    # bad tensors
    with pytest.raises(ValueError):
        st.split_merge(view, zt.to(torch.int64), 1, 0)
    with pytest.raises(ValueError):
        st.split_merge(view, zt, 1, 0, nproposals=2, trace=torch.empty(700, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        st.split_merge(view, zt, 1, 0, nproposals=2, log=torch.empty(8, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        st.split_merge(view, zt, 1, 0, counters=torch.zeros(5, dtype=torch.int32, device=dev))
    gpu_ctx.synchronize()
