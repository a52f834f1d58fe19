"""Row predictive log-density on the device (msc_score_marginal, State.predictive_logp) against the oracle's double
twin: t[r][k] = oracle_scores + crp_prior_matrix, scipy's logsumexp in float64, minus log(n_r + alpha).

The gate is derived, not measured: every t[r][k] is within E_r = 1e-6 max_k sum_f max(1, |score_f|) of the twin by the
project's standing gates (the prior term is exact) and a log-sum-exp moves by no more than the
largest change of an entry, so logp and map_logresp are held to E_r + 1e-6 max(1, |want|), the second term being the
plain gate for the reduction and the final rounding.  map equals the twin's arg-max except on rows whose two largest
twin totals lie within 2 E_r of each other, where it must be one of the twin's entries inside that band; such rows are
at most 1 % of a case (asserted from the twin alone)."""

import os
import re

import numpy as np
import pytest
import torch
from scipy.special import logsumexp

import common_amd
from oracle import oracle as orc
from tests.gpu_helpers import audit, crp_prior_matrix, load_state, make_feature, recarray_of, state_from_assignment

pytestmark = pytest.mark.gpu
MIX = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 5), (orc.NICH, 0)]


class Case(object):
    def __init__(self, ctx, specs, N, K, seed, alpha=1.5, used=None, masked=(), hp_of=None):
        """hp_of(j, family, dim) -> feature j's hyperparameter block, or None for make_feature's (set after the values are
        drawn: the data of a seed does not depend on it)"""
        rng = np.random.default_rng(seed)
        used = K if used is None else used
        self.N, self.K, self.alpha, self.specs = N, K, alpha, specs
        self.feats = [make_feature(fam, N, max(used, 1), rng, dim) for fam, dim in specs]
        if hp_of is not None:
            self.feats = [dict(f, hp=hp_of(j, f["family"], f["dim"]) or f["hp"]) for j, f in enumerate(self.feats)]
        z = rng.integers(0, max(used, 1), N).astype(np.int32)
        if used < K:                                  # a singleton group: it empties when its row leaves
            z[N // 2] = used
        self.z = z
        self.fs = state_from_assignment(self.feats, K, z)
        self.counts = np.bincount(z, minlength=K).astype(np.uint32)
        rec = recarray_of(self.feats)
        self.masks = [np.zeros(N, dtype=bool) for _ in specs]
        if masked:
            mrec = np.zeros(N, dtype=[(n, np.bool_, rec.dtype[n].shape) for n in rec.dtype.names])   # (a vector value is masked whole)
            for f in masked:
                self.masks[f] = rng.random(N) < 0.2
                mrec["f%d" % f] = self.masks[f] if rec.dtype["f%d" % f].shape == () else self.masks[f][:, None]
            rec = np.ma.masked_array(rec, mask=mrec)
        self.ctx = ctx
        if ctx is None:                               # (the twin alone: what the seeds' tie shares are checked with)
            return
        self.view = common_amd.DataView.from_recarray(ctx, rec)
        self.st = common_amd.State(ctx, specs, K)
        load_state(self.st, self.fs)
        self.st.set_group_counts(self.counts)
        self.st.set_alpha(alpha)

    def loo_z(self, seed=5):
        """the assignment with a tenth of the rows unassigned (ids -1 and K: both read as unassigned)"""
        rng = np.random.default_rng(seed)
        z = self.z.copy()
        off = rng.random(self.N) < 0.1
        off[self.N // 2] = False                      # (the singleton's row stays assigned)
        z[off] = np.where(rng.random(off.sum()) < 0.5, -1, self.K)
        return z

    def twin(self, rows, z=None, feats=None):
        """-> (t [n, K], E [n], logp [n]) of the rows, in float64"""
        zz = None
        if z is not None:
            zz = z[rows].copy()
            zz[(zz < 0) | (zz >= self.K)] = -1
        total, mag = 0.0, 0.0
        for i, (f, (F, ss64, _)) in enumerate(zip(self.feats, self.fs)):
            if feats is not None and i not in feats:
                continue
            m = F.score_matrix(ss64, f["values"][rows], zz)
            m = np.where(self.masks[i][rows][:, None], 0.0, m)
            total = total + m
            mag = mag + np.where(self.masks[i][rows][:, None], 0.0, np.maximum(1.0, np.abs(m)))
        t = total + crp_prior_matrix(self.counts, self.alpha, zz)
        n_r = float(self.counts.sum()) - (0 if zz is None else (zz >= 0).astype(np.float64))
        return t, 1e-6 * np.max(mag + np.zeros_like(t), axis=1), logsumexp(t, axis=1) - np.log(n_r + self.alpha)


def check_case(c, name, z=None, nsample=2048, seed=3):
    rows = np.sort(np.random.default_rng(seed).choice(c.N, min(nsample, c.N), replace=False))
    if z is not None and c.N // 2 not in rows:
        rows[0] = c.N // 2
        rows.sort()
    zt = None if z is None else torch.from_numpy(z).to(c.ctx.torch_device)
    logp, mp, lr = c.st.predictive_logp(c.view, z=zt, want_map=True)
    alone = c.st.predictive_logp(c.view, z=zt)
    torch.cuda.synchronize()
    kernel = c.ctx.last_kernel("marginal")
    logp, mp, lr, alone = (a.cpu().numpy()[rows] for a in (logp, mp, lr, alone))
    t, E, want = c.twin(rows, z)
    lse = logsumexp(t, axis=1)
    gate = E + 1e-6 * np.maximum(1.0, np.abs(want))
    print("%s%s: kernel %s, max |logp - want| / gate = %.3f" % (name, "" if z is None else " loo", kernel,
                                                                 float(np.max(np.abs(logp - want) / gate))))
    audit("marginal_logp_" + name, np.max(np.abs(logp - want) / gate), 1.0)
    audit("marginal_logp_nomap_" + name, np.max(np.abs(alone - want) / gate), 1.0)
    want_lr = t.max(axis=1) - lse
    gate_lr = E + 1e-6 * np.maximum(1.0, np.abs(want_lr))
    audit("marginal_logresp_" + name, np.max(np.abs(lr - want_lr) / gate_lr), 1.0)
    assert np.all(lr <= 0.0)
    # the arg-max: exact, but for rows whose two largest totals the twin itself holds within 2 E_r
    top = t.max(axis=1)
    second = np.partition(t, -2, axis=1)[:, -2] if c.K > 1 else np.full(len(rows), -np.inf)
    close = top - second <= 2 * E
    assert close.mean() <= 0.01, (name, close.mean())
    am = t.argmax(axis=1)
    assert np.array_equal(mp[~close], am[~close]), name
    assert np.all(t[close, mp[close]] >= top[close] - 2 * E[close]), name
    return kernel


CASES = {
    "nich_k40": ([(orc.NICH, 0)], 20000, 40, {}),
    "nich_k256": ([(orc.NICH, 0)], 40000, 256, {}),
    "nich_k1000": ([(orc.NICH, 0)], 20000, 1000, {}),
    "nich_k256_mostly_empty": ([(orc.NICH, 0)], 20000, 256, dict(used=9)),
    "nich_mask": ([(orc.NICH, 0)], 20000, 100, dict(masked=(0,), used=90)),   # (a seed whose two largest groups differ in size: masked rows see the prior alone)
    "mix_k64": (MIX, 33000, 64, dict(used=60)),
    "mix_k256": (MIX, 34000, 256, dict(used=250)),
    "mix_k256_full": (MIX, 33000, 256, {}),
    "mix_k300": (MIX, 6000, 300, dict(used=290)),
    "mix_k1000": (MIX, 6000, 1000, dict(used=900)),
    "mix_masked": (MIX, 33000, 128, dict(masked=(0, 1, 2, 3), used=120)),
    "bnb_bbnc_dm": ([(orc.BNB, 0), (orc.BBNC, 0), (orc.DM, 4)], 5000, 48, dict(used=40)),
    "niw3": ([(orc.NIW, 3), (orc.BB, 0)], 5000, 40, dict(used=36)),
    "niw32": ([(orc.NIW, 32)], 3000, 24, dict(used=20)),
    "bnb_dm_masked": ([(orc.BNB, 0), (orc.BBNC, 0), (orc.DM, 4)], 5000, 48, dict(used=40, masked=(0, 2))),
    "bbnc_masked": ([(orc.BBNC, 0), (orc.GP, 0), (orc.NICH, 0)], 5000, 48, dict(used=40, masked=(0,))),
    "niw3_masked": ([(orc.NIW, 3), (orc.BB, 0)], 5000, 40, dict(used=36, masked=(0,))),
    "niw32_masked": ([(orc.NIW, 32), (orc.GP, 0)], 3000, 24, dict(used=20, masked=(0,))),
    "k1": (MIX, 3000, 1, {}),
    "k1_nich": ([(orc.NICH, 0)], 5000, 1, {}),
    "k1_many_rows": ([(orc.DD, 5), (orc.NICH, 0), (orc.NICH, 0)], 17000, 1, {}),
    "mix_k300_many_rows": (MIX, 20000, 300, dict(used=290)),
    "few_rows": (MIX, 700, 64, dict(used=50)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_logp_map_and_logresp_against_the_twin(gpu_ctx, name):
    specs, N, K, kw = CASES[name]
    c = Case(gpu_ctx, specs, N, K, seed=sum(map(ord, name)), **kw)
    check_case(c, name)
    check_case(c, name, z=c.loo_z())


@pytest.mark.parametrize("name", ["nich_k256", "mix_k256", "mix_k300", "mix_k300_many_rows", "mix_masked"])
def test_row_ranges_give_the_whole_calls_bits(gpu_ctx, name):
    specs, N, K, kw = CASES[name]
    c = Case(gpu_ctx, specs, N, K, seed=11, **kw)
    for z in (None, c.loo_z()):
        zt = None if z is None else torch.from_numpy(z).to(gpu_ctx.torch_device)
        whole = [a.clone() for a in c.st.predictive_logp(c.view, z=zt, want_map=True)]
        cuts = [0, 129, N // 3 + 7, N]
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = c.st.predictive_logp(c.view, z=None if zt is None else zt[a:b].contiguous(), row0=a, nrows=b - a, want_map=True)
            torch.cuda.synchronize()
            for w, p in zip(whole, part):
                assert torch.equal(w[a:b], p), (name, a, b)


def test_against_the_long_route_at_a_million_rows_and_faster_than_it(gpu_ctx):
    """predictive_logp against float64 torch.logsumexp of score_value(crp_prior=True)'s matrix minus log(n + alpha),
    within twice the gate (both sides are within one gate of the twin; E_r from the library's own matrix: one nich
    feature, so E_r = 1e-6 max_k max(1, |t - prior|) <= 1e-6 max_k (1 + |t| + |prior|)) -- and, on this shape (C2: one
    nich column, 10^6 x 256), faster than that route, median of several runs each, no factor: the long route holds the
    whole score pass plus a second pass over nrows x K floats."""
    N, K = 1000000, 256
    c = Case(gpu_ctx, [(orc.NICH, 0)], N, K, seed=2, used=250)
    dev = gpu_ctx.torch_device
    mat = torch.empty((N, K), dtype=torch.float32, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    norm = float(np.log(float(c.counts.sum()) + c.alpha))

    def fused():
        c.st.predictive_logp(c.view, out=out)

    def long_route():
        c.st.score_value(c.view, out=mat, crp_prior=True)
        return torch.logsumexp(mat, dim=1)

    def median_ms(fn, reps=7):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))
    t_fused, t_long = median_ms(fused), median_ms(long_route)
    print("C2 shape: predictive_logp %.3f ms, score_value + logsumexp %.3f ms (%s)" % (t_fused, t_long, gpu_ctx.last_kernel("marginal")))
    want = (torch.logsumexp(mat.double(), dim=1) - norm).cpu().numpy()
    prior = crp_prior_matrix(c.counts, c.alpha)
    E = 1e-6 * (1.0 + mat.abs().max(dim=1).values.cpu().numpy().astype(np.float64) + np.abs(prior).max())
    gate = 2.0 * (E + 1e-6 * np.maximum(1.0, np.abs(want)))
    audit("marginal_vs_long_route", np.max(np.abs(out.cpu().numpy() - want) / gate), 1.0)
    assert t_fused < t_long, (t_fused, t_long)


@pytest.mark.parametrize("name", ["nich_k256", "mix_k256", "mix_k300"])
def test_the_state_is_read_only(gpu_ctx, name):
    specs, N, K, kw = CASES[name]

    def run(between):
        c = Case(gpu_ctx, specs, N, K, seed=19, **kw)
        zt = torch.from_numpy(c.z.copy()).to(gpu_ctx.torch_device)
        c.st.sweep_step(c.view, zt, seed=5, sweep=0)
        if between:
            c.st.predictive_logp(c.view, z=zt, want_map=True)
            c.st.predictive_logp(c.view)
        ss = [c.st.get_ss(f) for f in range(len(specs))]
        counts, sd = c.st.get_group_counts(), c.st.score_data().cpu().numpy()
        c.st.sweep_step(c.view, zt, seed=5, sweep=1)
        torch.cuda.synchronize()
        return ss, counts, sd, zt.cpu().numpy()
    a, b = run(False), run(True)
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_given_is_the_conditional_density_and_sums_to_one_over_a_label(gpu_ctx):
    specs = [(orc.DD, 4), (orc.BB, 0), (orc.GP, 0), (orc.NICH, 0)]
    N, K = 33000, 64
    c = Case(gpu_ctx, specs, N, K, seed=23, used=60)
    others = [1, 2, 3]
    sub = c.st.subset(others)
    for i, f in enumerate(others):
        assert sub.get_hp(i).tobytes() == c.st.get_hp(f).tobytes()
        assert sub.get_ss(i).tobytes() == c.st.get_ss(f).tobytes()
    assert np.array_equal(sub.get_group_counts(), c.counts) and sub.get_alpha() == c.st.get_alpha()
    rows = np.arange(0, N, 16)
    got = c.st.predictive_logp(c.view, given=others).cpu().numpy()[rows]
    t_all, E_all, lp_all = c.twin(rows)
    t_sub, E_sub, lp_sub = c.twin(rows, feats=others)
    want = lp_all - lp_sub
    gate = (E_all + 1e-6 * np.maximum(1.0, np.abs(lp_all))) + (E_sub + 1e-6 * np.maximum(1.0, np.abs(lp_sub)))
    audit("marginal_given", np.max(np.abs(got - want) / gate), 1.0)
    # over the label's values the conditional probabilities add up to one
    total = np.zeros(N)
    for v in range(4):
        feats = [dict(f) for f in c.feats]
        feats[0]["values"] = np.full(N, v, dtype=np.int32)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
        total += np.exp(c.st.predictive_logp(view, given=others).cpu().numpy().astype(np.float64))
    audit("marginal_given_sums_to_one", np.max(np.abs(total - 1.0)), 1e-5)
    # a table changes: the cached subset goes
    assert c.st.__dict__.get("_subsets")
    c.st.set_alpha(2.0)
    assert not c.st.__dict__.get("_subsets")


def test_bad_arguments(gpu_ctx):
    c = Case(gpu_ctx, [(orc.NICH, 0)], 1000, 8, seed=1)
    dev = gpu_ctx.torch_device
    out = torch.empty(1000, dtype=torch.float32, device=dev)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "microscopes_hip.h")) as fh:
        einval = int(re.search(r"MSC_EINVAL\s*=\s*(-?\d+)", fh.read()).group(1))
    lib = gpu_ctx.lib
    assert lib.msc_score_marginal(c.st._h, c.view._h, None, 0, 1000, None, 1, out.data_ptr(), None, None) == einval   # flags
    assert lib.msc_score_marginal(c.st._h, c.view._h, None, 0, 1000, None, 0, None, None, None) == einval           # no output
    assert lib.msc_score_marginal(None, c.view._h, None, 0, 1000, None, 0, out.data_ptr(), None, None) == einval    # no state
    assert c.st.predictive_logp(c.view, nrows=0).numel() == 0
    # between sweep_step_begin and commit_reduce the tables hold uncommitted sums: refused, and fine again afterwards
    zt = torch.from_numpy(c.z.copy()).to(dev)
    c.st.sweep_step_begin(c.view, zt, seed=3, sweep=0)
    assert lib.msc_score_marginal(c.st._h, c.view._h, None, 0, 1000, None, 0, out.data_ptr(), None, None) == einval
    c.st.commit_reduce()
    assert lib.msc_score_marginal(c.st._h, c.view._h, None, 0, 1000, None, 0, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
