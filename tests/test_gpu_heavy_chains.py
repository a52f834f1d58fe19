"""The sequential and chain-ensemble routes at production-sized groups against the 60-digit fixture: what
tests/test_gpu_heavy.py holds for the batched routes, for the calls built since -- the ensemble's row predictive
(k_chains_marginal), a visit of the sequential sweep (seq_visits / seq_move: leave, commit_group, prepare_group, score,
draw, join) through msc_chains_visit, msc_chains_sweep_tempered and msc_sweep_sequential, the tables a visit leaves, and
the log joint (k_score_joint, k_chains_score_joint).  tests/heavy_chain_cases.py is the host side: the rows, who visits
what under which key, the fixture's expectations, the exact tables; tests/test_heavy_chains_cpu.py runs it without a device.

The state is hc.SEQUENTIAL's five families, one feature each, with test_gpu_heavy.install()'s tables in every chain; both
layouts in every test: K = 16 (the sliced scoring of seq_visits, nq = 16) and K = 300 (the strided scoring, two groups a
thread in the draw).  98 rows, at most 128 chains.  Every expectation is the fixture's; the gate is TOL on rel_err through
test_gpu_heavy.check() unless a test says otherwise.

What these tests found (MI355X): no wrong constant, and no library change.  Worst errors per route, K = 16 / K = 300:
  ensemble predictive      1.38e-7 / 1.10e-7 (full value list, the large instantiation), 1.09e-7 / 1.08e-7 (cut to <= 1023
                           and to <= 1000, the plain one); the mix equals every chain
  visit increment          1.67e-7 / 1.10e-7; ens.logw 1.34e-7 / 1.15e-7; all 126 draws the fixture CDF's on either layout
  tempered visit           all 768 draws the fixture CDF's on either layout; the beta = 1 chains draw (b)'s groups
  single-chain call        the ensemble's draw and table bits in all 8 visits
  tables after a visit     integers equal; nich mean 0.49 ulp; gp log_prod 5.3e-8; count_times_variance after the near-mean
                           join 8.8e-7 (the estimate was 2 - 4e-6), after the near-mean leave 0; where the double sum of
                           squares cannot hold TOL (the lopsided rungs) 1.67e-6, 0.37 / 0.49 of that representation
                           bound; every other touched group 3.7e-8
  log joint                assignment 5.4e-16, features 3.9e-15, total 2.5e-15 (state and ensemble); the layouts'
                           difference off by at most 1.8e-4 absolute (gp, sums of 1e11) against a gate of 2.1e5
msc_score_joint refuses niw (its double evaluator has no niw score_data): the two niw states hold that refusal."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import common_amd
from tests import heavy_cases as hc
from tests import heavy_chain_cases as cc
from tests.gpu_helpers import TOL, audit, rel_err
from tests.test_gpu_heavy import CASES, LAYOUTS, Heavy, _id, check, install

pytestmark = pytest.mark.gpu
NAMES = cc.NAMES
FEATURES = [hc.FAMILIES[n] for n in NAMES]
_lay = pytest.mark.parametrize("K", LAYOUTS, ids=["rungs", "K300"])


def _ensemble(ctx, v, nchains):
    """nchains chains of the sequential families, every one holding the heavy tables of the layout of v (an hc.Expect)"""
    ens = common_amd.ChainEnsemble(ctx, FEATURES, v.K, nchains)
    for st in ens.states:
        install(st, NAMES, v.rung, v.counts)
    return ens


# ---- a. the ensemble's row predictive -----------------------------------------------------------------------------------

@_lay
@pytest.mark.parametrize("vmax", [None, 1023, 1000], ids=["full", "le1023", "le1000"])
def test_ensemble_predictive_on_heavy_groups(gpu_ctx, K, vmax):
    """Three chains, each the heavy state: every chain's row predictive and the mix (equal chains: the mix is each chain)
    against the fixture.

    Which instantiation ran: the launch is not recorded in last_kernel, so the host-only plan function says -- the
    launcher takes CmPlan.large and CmPlan.wide from plan_chains_marginal, which cc.cm_plan calls for the same families,
    K and vcap = min(column maximum + 1, 1024).  The full value list (up to 65535) gives large; so does the list cut to
    values <= 1023, whose vcap is the table's cap 1024 -- the plan cannot tell such a column from one with counts beyond
    the table, so that run takes the tabled branch of the large instantiation; the plain instantiation needs a maximum
    below 1023 and is the run cut to values <= 1000.  K = 16 is a narrow tile (batches of 8), K = 300 a wide one
    (batches of 32, a tile of 288 groups and one of 12); bb, dd and nich are staged in LDS, the gp and bnb tables are
    read from global memory."""
    h = Heavy(gpu_ctx, NAMES, K, n=cc.NROWS, vmax=vmax)
    plan = cc.cm_plan(NAMES, h.K, vmax)
    assert plan["large"] == (vmax != 1000) and plan["wide"] == (h.K == 300) and plan["staged"] == [True, False, False, True, True]
    assert int(h.counts.sum()) < 2 ** 32
    ens = _ensemble(gpu_ctx, h, 3)
    mix, per = ens.predictive_logp(h.view, per_chain=True)
    want = h.totals()[1]
    tag = "%s.K%d" % ({None: "full", 1023: "le1023", 1000: "le1000"}[vmax], h.K)
    per = per.cpu().numpy()
    for c in range(3):
        check("chains_predictive.chain%d.%s" % (c, tag), per[c], want)
    check("chains_predictive.mix.%s" % tag, mix.cpu().numpy(), want)
    ens.close()


# ---- b. one visit per chain, untempered (run once a layout, shared by b, c, d and e) ----------------------------------------

_VISIT = {}


def _visit(ctx, K):
    """the one untempered visit of every chain -> dict(v: the cc.Visits, inc float32 [NCHAINS], logw float64 [NCHAINS],
    got int [NCHAINS]: the group joined, tables [NCHAINS]: (group counts, [suff-stats of every feature]))"""
    if K not in _VISIT:
        v = cc.Visits(K)
        assert v.total < 2 ** 32
        view = common_amd.DataView.from_recarray(ctx, v.rec)
        ens = _ensemble(ctx, v, cc.NCHAINS)
        ens.assign(view, v.zfull)                         # (accumulates the rows: the heavy tables go in afterwards)
        for st in ens.states:
            install(st, NAMES, v.rung, v.counts)
        order = np.empty((cc.NCHAINS, v.nrows), dtype=np.int32)
        for c in range(cc.NCHAINS):                       # the chain's row first, the others after it
            r = int(v.row_of[c])
            order[c] = [r] + [i for i in range(v.nrows) if i != r]
        logp = ens.visit(view, 0, 1, v.seeds, sweep=cc.SWEEP, order=torch.from_numpy(order).to(ctx.torch_device), want_logp=True)
        logp = logp.cpu().numpy()
        assert np.isnan(logp[:, 1:]).all()                # (one visit a chain)
        z = ens.z.cpu().numpy()
        rows = np.arange(cc.NCHAINS)
        untouched = np.ones(z.shape, dtype=bool)
        untouched[rows, v.row_of] = False
        assert np.array_equal(z[untouched], np.broadcast_to(v.zfull, z.shape)[untouched])
        tables = [(st.get_group_counts(), [st.get_ss(i) for i in range(len(NAMES))]) for st in ens.states]
        _VISIT[K] = dict(v=v, inc=logp[:, 0], logw=ens.logw.cpu().numpy(), got=z[rows, v.row_of].astype(np.int64), tables=tables)
        ens.close()
    return _VISIT[K]


def _check_draws(tag, ts, us, got, K):
    """test_gpu_heavy._sweep_check's rule for visits with a key and a row id each: at least 0.98 of the draws are the
    fixture CDF's, every other one is proven on a CDF step by _check_agreement's own test (cc.step_proven)"""
    got = np.asarray(got)
    assert np.all((got >= 0) & (got < K))
    want = np.array([cc.want_draw(t, u) for t, u in zip(ts, us)])
    agree = float((got == want).mean())
    print("%s: draw agreement %.4f over %d visits" % (tag, agree, len(got)))
    assert agree >= 0.98, agree
    for i in np.nonzero(got != want)[0]:
        assert cc.step_proven(ts[i], us[i], got[i], want[i]), (tag, i, got[i], want[i], us[i])


@_lay
def test_one_visit_per_chain_on_heavy_groups(gpu_ctx, K):
    """Chain c visits row c mod 98 of the pristine heavy state under its own key: a row with a group leaves it first (the
    fixture's loo score in its own group, score_value elsewhere), an unassigned one only joins.  The increment, ens.logw
    and the draw against the fixture.  Share of the visited fixture rows whose dart lies within 1e-5 of a step of the
    fixture's CDF, computed on the host (tests/test_heavy_chains_cpu.py holds it below 0.02): 0 of 126 on either layout
    at cc.SEED = 7100 -- the 1e8-row groups hold all but 1e-4 of the mass, the steps are few."""
    run = _visit(gpu_ctx, K)
    v = run["v"]
    fx = np.nonzero(v.row_of < v.n)[0]                    # the chains on fixture rows (the two near-mean rows: test c)
    rows = v.row_of[fx]
    # every value of every family is visited, and every rung a row can leave loses one
    for i, nm in enumerate(NAMES):
        assert len(np.unique(v.vidx[i][rows])) == len(hc.values(nm)), nm
    left = v.z[rows]
    feasible = np.unique(v.rung[np.nonzero(v.ok.any(axis=0))[0]])
    assert np.array_equal(np.unique(v.rung[left[left >= 0]]), feasible) and (left < 0).any()
    tag = "K%d" % v.K
    check("visit.increment." + tag, run["inc"][fx], v.inc[rows])
    check("visit.logw." + tag, run["logw"][fx], v.inc[rows])
    # logw is the increment before its rounding to float: the two differ by that rounding alone
    assert np.all(np.abs(run["logw"][fx] - run["inc"][fx].astype(np.float64)) <= np.spacing(np.abs(run["inc"][fx])).astype(np.float64))
    _check_draws("visit." + tag, v.t[rows], v.u[fx], run["got"][fx], v.K)
    # the unassigned near-mean row lands in the lopsided 1e8 group its dart was placed in
    assert run["got"][v.n + 1] == v.lop


# ---- c. the tables a visit leaves ---------------------------------------------------------------------------------------

def _check_tables(v, c, got_group, counts, ss, worst):
    """chain c's tables after its visit against the exact update of the installed fields: the row left zfull[row] (if any)
    and joined got_group.  Untouched groups hold the installed bits; worst: dict of the largest errors seen"""
    r = int(v.row_of[c])
    row, old = v.row_values(r), int(v.zfull[r])
    groups = {}
    if old >= 0:
        groups.setdefault(old, cc.ExactGroup(v.rung[old])).move(row, -1)
    groups.setdefault(got_group, cc.ExactGroup(v.rung[got_group])).move(row, +1)
    want_counts = v.counts.copy()
    if old >= 0:
        want_counts[old] -= 1
    want_counts[got_group] += 1
    assert np.array_equal(counts, want_counts), c
    rest = np.ones(v.K, dtype=bool)
    rest[list(groups)] = False
    for i, nm in enumerate(NAMES):                        # a visit commits the two groups it touches, no other
        src = cc.RUNGS[nm][v.rung]
        for f in ss[i].dtype.names:
            assert np.array_equal(ss[i][f][rest], src[f][rest].astype(ss[i][f].dtype)), (c, nm, f)
    bb, gp, bnb, dd, nich = ss
    for k, g in groups.items():
        assert [int(bb["heads"][k]), int(bb["tails"][k])] == g.bb, (c, k)
        assert [int(gp["count"][k]), int(gp["sum"][k])] == g.gp and [int(bnb["count"][k]), int(bnb["sum"][k])] == g.bnb, (c, k)
        assert [int(x) for x in dd["counts"][k]] == g.dd and int(dd["count_sum"][k]) == sum(g.dd), (c, k)
        assert int(nich["count"][k]) == g.n, (c, k)
        worst["log_prod"] = max(worst["log_prod"], float(rel_err(float(gp["log_prod"][k]), g.log_prod)))
        mean, ctv = g.nich()
        ulp = float(np.spacing(np.abs(np.float32(float(mean))))) if mean != 0 else float(np.spacing(np.float32(0)))
        worst["mean_ulp"] = max(worst["mean_ulp"], abs(float(Fraction(float(nich["mean"][k])) - mean)) / ulp)
        # relative; an exact 0 is held to 1e-6 absolute (test_gpu_heavy._check_accumulated's rule)
        e = abs(float(Fraction(float(nich["count_times_variance"][k])) - ctv)) / max(float(ctv), 1.0 if ctv == 0 else 0.0)
        if r >= v.n and v.rung[k] == cc.LOPSIDED_1E8:
            worst["ctv_near_mean"] = max(worst["ctv_near_mean"], e)
        elif g.ctv_representation_bound() <= TOL:
            worst["ctv"] = max(worst["ctv"], e)
        else:                                             # the double sum of squares cannot hold the field to TOL
            worst["ctv_wide"] = max(worst["ctv_wide"], e)
            worst["ctv_over_bound"] = max(worst["ctv_over_bound"], e / g.ctv_representation_bound())


@_lay
def test_tables_after_one_visit_on_heavy_groups(gpu_ctx, K):
    """get_group_counts / get_ss of every chain after its visit against the exact rational update (fractions.Fraction) of
    the installed float32 fields by the row that left and the group it joined: integers equal, the nich mean within one
    float32 ulp and count_times_variance within TOL relative -- test_lopsided_accumulation_is_exact's gates -- and gp's
    log_prod (a sum of lgamma, no rational) within TOL of the double update.

    The two near-mean rows (nich -1000.375 leaving a lopsided 1e8 group, -1000.5625 joining one: mean -1000.5, count x
    variance 1e4 on sums of squares of 1.001e14) are where commit_group's sxx - n mean^2 was estimated to lose 2 - 4e-6;
    their count_times_variance is held to TOL and reported apart.  Measured: 8.8e-7 for the join (3.9e-7 of it is
    (-1000.5625)^2 rounded into the sum, whose ulp is 1/64 there), 0 for the leave.

    One gate is no plain TOL.  The additive table keeps sum x^2 in double.  On the lopsided rungs (mean -1000.5,
    variance 1e-4) that sum is 1e10 times count_times_variance, so every store of it rounds away up to 2^-53 x 1e10 =
    1.1e-6 of the field, whatever the commit then does: the first run of this test found 1.67e-6 on the lopsided
    one-row rung joined by -1000.5 (two stores of a sum of 2.002e6 for a field of 1e-4).  For a touched group whose
    bound -- cc.ExactGroup.ctv_representation_bound, from the exact sums and the number of stores, nothing read off
    the device -- exceeds TOL, the gate is that bound; every other touched group is held to TOL."""
    run = _visit(gpu_ctx, K)
    v = run["v"]
    worst = dict(log_prod=0.0, mean_ulp=0.0, ctv=0.0, ctv_near_mean=0.0, ctv_wide=0.0, ctv_over_bound=0.0)
    for c in range(cc.NCHAINS):
        _check_tables(v, c, int(run["got"][c]), run["tables"][c][0], run["tables"][c][1], worst)
    tag = "K%d" % v.K
    print("tables after a visit, %s: mean off by %.3f ulp, ctv by %.3g relative (near the lopsided 1e8 mean: %.3g; where "
          "the sum of squares cannot hold TOL: %.3g, %.3f of its bound), gp log_prod by %.3g"
          % (tag, worst["mean_ulp"], worst["ctv"], worst["ctv_near_mean"], worst["ctv_wide"], worst["ctv_over_bound"],
             worst["log_prod"]))
    audit("heavy.visit_mean_ulp." + tag, worst["mean_ulp"], 1.0)
    audit("heavy.visit_ctv." + tag, worst["ctv"], TOL)
    audit("heavy.visit_ctv_near_mean." + tag, worst["ctv_near_mean"], TOL)
    audit("heavy.visit_ctv_over_representation_bound." + tag, worst["ctv_over_bound"], 1.0)
    audit("heavy.visit_log_prod." + tag, worst["log_prod"], TOL)


# ---- d. one visit per chain, tempered --------------------------------------------------------------------------------------

@_lay
def test_one_tempered_visit_per_chain_on_heavy_groups(gpu_ctx, K):
    """(b) through ens.sweep(view, 1, keys, beta=...) over a one-row range: call j visits fixture row j in eight chains,
    reinstalled pristine before it, chain i at float32 {1, 0.5, 0.25, 0}[i mod 4].  The draw against the CDF of
    log pseudocount + float64(beta32) * (the features' fixture sum) -- at beta = 0 the CRP terms alone -- by (b)'s
    CDF-step rule; chain 0's key is that of (b)'s chain j, and at beta = 1 its draw is (b)'s bit for bit.  Share of the
    768 tempered visits whose dart lies within 1e-5 of a CDF step, from the host: 0 (K = 16), 0.0013 (K = 300)."""
    run = _visit(gpu_ctx, K)
    v = run["v"]
    view = common_amd.DataView.from_recarray(gpu_ctx, v.rec)
    ens = _ensemble(gpu_ctx, v, cc.ND)
    ens.assign(view, v.zfull)
    beta = torch.from_numpy(v.beta_d.copy()).to(gpu_ctx.torch_device)
    got = np.empty((v.n, cc.ND), dtype=np.int64)
    for j in range(v.n):
        for st in ens.states:
            install(st, NAMES, v.rung, v.counts)
        ens.sweep(view, 1, v.keys_d[j], sweep=cc.SWEEP, row0=j, nrows=1, beta=beta)
    z = ens.z.cpu().numpy()
    got[:] = z[:, :v.n].T
    assert np.array_equal(z[:, v.n:], np.broadcast_to(v.zfull[v.n:], (cc.ND, 2)))
    ts, us, gs = [], [], []
    for j in range(v.n):
        for i in range(cc.ND):
            ts.append(v.t_tempered(j, v.beta_d[i]))
            us.append(v.u_d[j, i])
            gs.append(got[j, i])
    _check_draws("tempered.K%d" % v.K, ts, us, gs, v.K)
    assert v.beta_d[0] == 1.0 and all(v.keys_d[j][0] == v.seeds[j] and v.row_of[j] == j for j in range(v.n))
    assert np.array_equal(got[:, 0], run["got"][:v.n])     # beta = 1: the untempered visit's bits
    ens.close()


# ---- e. the single-chain call -------------------------------------------------------------------------------------------

@_lay
def test_single_chain_visit_is_the_ensembles_on_heavy_groups(gpu_ctx, K):
    """eight rows through State.sweep_sequential with nrows = 1 from a reinstalled heavy state: the draws of (b)'s chains
    (kernels_seq.hip: a chain of the ensemble performs the arithmetic of the single-chain launch)"""
    run = _visit(gpu_ctx, K)
    v = run["v"]
    view = common_amd.DataView.from_recarray(gpu_ctx, v.rec)
    st = common_amd.State(gpu_ctx, FEATURES, v.K)
    for c in (0, 7, 13, 40, 77, v.n, v.n + 1, 111):       # assigned and unassigned rows, both near-mean rows, a second visit of a row
        r = int(v.row_of[c])
        install(st, NAMES, v.rung, v.counts)
        zt = torch.from_numpy(v.zfull[r:r + 1].copy()).to(gpu_ctx.torch_device)
        st.sweep_sequential(view, zt, v.seeds[c], cc.SWEEP, row0=r, nrows=1)
        assert int(zt.cpu().numpy()[0]) == run["got"][c], (c, r)
        counts = st.get_group_counts()
        assert np.array_equal(counts, run["tables"][c][0])
        for i in range(len(NAMES)):
            assert st.get_ss(i).tobytes() == run["tables"][c][1][i].tobytes(), (c, i)
    st.close()


# ---- f. the log joint --------------------------------------------------------------------------------------------------------

def _joint_want(h):
    """-> (score_assignment, [the features' score_data summed over the counted slots]) from the fixture"""
    assert h.R == 16
    return hc.load_score_assignment()["K%d" % h.K], [math.fsum(h.data[f][h.counts > 0]) for f in range(len(h.names))]


def _check_joint(tag, got, h):
    crp, data = _joint_want(h)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(h.names) + 3,) and got[-1] == 0.0        # (no hyper-prior asked for)
    check("joint.assignment." + tag, got[1:2], [crp])
    check("joint.data." + tag, got[2:-1], data)
    check("joint.total." + tag, got[0:1], [crp + math.fsum(data)])


def _check_layout_difference(tag, a_dev, b_dev, a, b):
    """what exchange and anneal_weights consume is a difference of such sums: device a - b against the fixture's, gate
    TOL max(1, |a|, |b|) -- the most two TOL-held operands can differ by"""
    worst = 0.0
    for x, y, p, q in zip(a_dev, b_dev, a, b):
        err, gate = abs((x - y) - (p - q)), TOL * max(1.0, abs(p), abs(q))
        worst = max(worst, err / gate)
        print("%s: layout difference %.17g (fixture %.17g): off by %.3g, gate %.3g" % (tag, x - y, p - q, err, gate))
        audit("heavy.joint_layout_difference." + tag, err, gate)
    return worst


@pytest.mark.parametrize("names", CASES, ids=_id)
def test_score_joint_on_heavy_groups(gpu_ctx, names):
    """State.score_joint of the nine single-family states and the mixed one, both layouts: the CRP term against the
    fixture's score_assignment, every feature's entry against math.fsum of the fixture's score_data over the counted
    (non-empty) slots, the total against their sum, and the difference of the two layouts' per-feature sums.
    The two niw states have no log joint -- msc_score_joint refuses the family (its double evaluator has no niw
    score_data) -- so what is held for them is that refusal: an error, no number."""
    hs = [Heavy(gpu_ctx, names, K) for K in LAYOUTS]
    if names[0].startswith("niw"):
        for h in hs:
            with pytest.raises(common_amd.MicroscopesHipError, match="niw"):
                h.st.score_joint()
        return
    got = [h.st.score_joint().cpu().numpy() for h in hs]
    for h, g in zip(hs, got):
        _check_joint("%s.K%d" % (_id(names), h.K), g, h)
    wants = [_joint_want(h) for h in hs]
    _check_layout_difference(_id(names), got[0][1:-1], got[1][1:-1], [wants[0][0]] + wants[0][1], [wants[1][0]] + wants[1][1])


def test_ensemble_score_joint_on_heavy_groups(gpu_ctx):
    """ChainEnsemble.score_joint of three chains on the sequential families, both layouts: every chain's row as above"""
    got, wants = [], []
    for K in LAYOUTS:
        h = hc.Expect(NAMES, K, 8)
        ens = _ensemble(gpu_ctx, h, 3)
        rows = ens.score_joint().cpu().numpy()
        for c in range(3):
            _check_joint("chains.chain%d.K%d" % (c, h.K), rows[c], h)
        got.append(rows[0])
        wants.append(_joint_want(h))
        ens.close()
    _check_layout_difference("chains", got[0][1:-1], got[1][1:-1], [wants[0][0]] + wants[0][1], [wants[1][0]] + wants[1][1])
