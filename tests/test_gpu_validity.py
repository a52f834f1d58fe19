"""GPU: the state's table-validity bookkeeping, seen from outside -- a matrix of mutator x consumer on one tiny model.
Two states A and B get the same history up to and including the mutator.  B is then made to forget everything cached
(set_ss(get_ss()) of every feature, set_group_counts(get_group_counts()), set_alpha(get_alpha()): the additive, derived
and CRP tables and any blocked draw are stale after that), A is left alone, the consumer runs on both and the outputs
are compared BIT FOR BIT: a flag left valid that should not be shows as a table A did not rebuild.

A pair in ROUNDING is one where two code paths of the library compute the same table with different rounding: that pair
alone is held at the plain gate 1e-6 max(1, |B|), through gpu_helpers.audit, with the difference measured.  Run on the
commit before the bookkeeping was gathered in table_validity.hpp, all 114 pairs were bit-equal: the list is empty.

Written against common_amd's public Python API only."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.gpu_helpers import TOL, audit, distinct_hp, make_feature, recarray_of

pytestmark = pytest.mark.gpu

N, K, ALPHA = 500, 20, 1.3          # (the size of tests/test_gpu_blocked.py::test_errors)
MODELS = {
    "mixed": [(orc.BB, 0), (orc.GP, 0), (orc.DD, 4), (orc.NICH, 0)],
    "niw": [(orc.NIW, 3), (orc.NICH, 0)],
}
# per model: the feature set_ss / set_hp change, the feature the grid covers, the nich feature the slice step moves
PICK = {"mixed": dict(ss=3, hp=2, grid=2, slice=3), "niw": dict(ss=0, hp=0, grid=1, slice=1)}
# what a family does not support is left out by name: niw with the sequential, blocked and split-merge samplers
UNSUPPORTED = {"niw": {"sweep_sequential", "sweep_blocked", "split_merge", "blocked_draw"}}

# (model, mutator, consumer) -> max |A - B| / max(1, |B|) measured before the refactor; every other pair is bit-equal
# (none: every pair was)
ROUNDING = {}


class Pair(object):
    """one state and the assignment vector that describes it"""

    def __init__(self, ctx, model, view, z0):
        import common_amd
        self.ctx, self.model, self.view = ctx, model, view
        self.st = common_amd.State(ctx, MODELS[model], K)
        for i, (fam, dim) in enumerate(MODELS[model]):
            self.st.set_hp(i, distinct_hp(fam, dim, i))
        self.st.set_alpha(ALPHA)
        self.z = torch.from_numpy(z0.copy()).to(ctx.torch_device)
        self.st.accumulate(view, self.z)
        self.keep = []

    def forget(self):
        st = self.st
        for f in range(len(st.features)):
            st.set_ss(f, st.get_ss(f))
        st.set_group_counts(st.get_group_counts())
        st.set_alpha(st.get_alpha())


@pytest.fixture(scope="module")
def data(gpu_ctx):
    """per model: the view and the starting assignment (the last two groups empty, row 5 unassigned); nich and niw
    values are multiples of 1/8, so that their sums are exact in whatever order the additions happen"""
    import common_amd
    out = {}
    for model, specs in MODELS.items():
        rng = np.random.default_rng(20 + len(specs))
        feats = [make_feature(f, N, K, rng, d) for f, d in specs]
        for f in feats:
            if f["family"] in (orc.NICH, orc.NIW):
                f["values"] = (np.round(f["values"] * 8.0) / 8.0).astype(np.float32)
        z0 = rng.integers(0, K - 2, N).astype(np.int32)
        z0[5] = -1
        z1 = rng.integers(0, K - 2, N).astype(np.int32)
        out[model] = (common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats)), z0, z1)
    return out


# ---- mutators: p is a Pair; z1 a second assignment ---------------------------------------------------------------------
def m_set_ss(p, z1):
    f = PICK[p.model]["ss"]
    rec = p.st.get_ss(f)
    rec[K - 1] = rec[0]                    # (a valid record into an empty group: no row's leave-one-out term reads it)
    p.st.set_ss(f, rec)


def m_set_hp(p, z1):
    f = PICK[p.model]["hp"]
    fam, dim = MODELS[p.model][f]
    p.st.set_hp(f, distinct_hp(fam, dim, 3))


def m_set_alpha(p, z1):
    p.st.set_alpha(2.5)


def m_set_group_counts(p, z1):
    p.st.set_group_counts(p.st.get_group_counts() * 2)


def m_accumulate_reset(p, z1):
    p.z.copy_(torch.from_numpy(z1))
    p.st.accumulate(p.view, p.z, reset=True)


def m_accumulate(p, z1):
    # rows 100 .. 149 leave their groups
    p.st.accumulate(p.view, p.z[100:], row0=100, nrows=50, reset=False, subtract=True)
    p.z[100:150] = -1


def m_step_begin_commit(p, z1):
    p.st.sweep_step_begin(p.view, p.z, 7, 0)
    p.st.commit_reduce()


def m_entity_op(p, z1):
    g = int(p.z[7].item())
    p.st.entity_op(p.view, 7, g, join=False, z=p.z)
    p.st.entity_op(p.view, 7, (g + 1) % (K - 2), join=True, z=p.z)


def m_sweep_step(p, z1):
    p.st.sweep_step(p.view, p.z, 7, 0)


def m_sweep_sequential(p, z1):
    p.z[5] = 0                             # (every row assigned: the chain visits them all)
    p.st.accumulate(p.view, p.z, reset=True)
    p.st.sweep_sequential(p.view, p.z, 7, 0)


def m_sweep_blocked(p, z1):
    p.st.sweep_blocked(p.view, p.z, 7, 0)


def m_split_merge(p, z1):
    p.z[5] = 0
    p.st.accumulate(p.view, p.z, reset=True)
    p.st.split_merge(p.view, p.z, 7, 0, nproposals=2)


def m_grid_gibbs(p, z1):
    f = PICK[p.model]["grid"]
    fam, dim = MODELS[p.model][f]
    grids = [p.st.hp_grid(f, [distinct_hp(fam, dim, i) for i in (1, 2, 4)]), p.st.crp_grid([0.5, 1.0, 2.0])]
    p.keep += grids
    p.st.hp_gibbs(grids, seed=7, sweep=0)


def m_slice(p, z1):
    p.st.hp_slice([{"feature": PICK[p.model]["slice"], "coord": 1, "width": 0.5}, {"feature": "alpha", "width": 0.5}],
                  seed=7, sweep=0)


MUTATORS = [("set_ss", m_set_ss), ("set_hp", m_set_hp), ("set_alpha", m_set_alpha),
            ("set_group_counts", m_set_group_counts), ("accumulate_reset", m_accumulate_reset),
            ("accumulate", m_accumulate), ("step_begin_commit", m_step_begin_commit), ("entity_op", m_entity_op),
            ("sweep_step", m_sweep_step), ("sweep_sequential", m_sweep_sequential), ("sweep_blocked", m_sweep_blocked),
            ("split_merge", m_split_merge), ("grid_gibbs", m_grid_gibbs), ("slice", m_slice)]


# ---- consumers: -> list of numpy arrays ---------------------------------------------------------------------------------
def c_score_value(p):
    return [p.st.score_value(p.view, z=p.z, crp_prior=True).cpu().numpy()]


def c_score_data(p):
    return [p.st.score_data().cpu().numpy()]


def c_score_marginal(p):
    return [p.st.predictive_logp(p.view, z=p.z).cpu().numpy()]


def c_get_ss(p):
    out = []
    for f in range(len(p.st.features)):
        rec = p.st.get_ss(f)
        out += [np.ascontiguousarray(rec[name]) for name in rec.dtype.names]
    return out + [p.st.get_group_counts()]


def c_blocked_draw(p):
    p.st.blocked_draw(3, 0)
    tabs = p.st.blocked_tables()
    return [tabs[k].cpu().numpy() for k in ["logw"] + list(range(len(p.st.features)))]


CONSUMERS = [("score_value", c_score_value), ("score_data", c_score_data), ("score_marginal", c_score_marginal),
             ("get_ss", c_get_ss), ("blocked_draw", c_blocked_draw)]

CASES = [(model, mn, cn) for model in MODELS for mn, _ in MUTATORS for cn, _ in CONSUMERS
         if not {mn, cn} & UNSUPPORTED.get(model, set())]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("model,mutator,consumer", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_pair(gpu_ctx, data, model, mutator, consumer):
    view, z0, z1 = data[model]
    a, b = Pair(gpu_ctx, model, view, z0), Pair(gpu_ctx, model, view, z0)
    mutate, consume = dict(MUTATORS)[mutator], dict(CONSUMERS)[consumer]
    mutate(a, z1)
    mutate(b, z1)
    assert torch.equal(a.z, b.z)
    b.forget()
    got, want = consume(a), consume(b)
    gpu_ctx.synchronize()
    assert len(got) == len(want)
    err, bit_equal = 0.0, True
    for x, y in zip(got, want):
        assert x.shape == y.shape and x.dtype == y.dtype
        if np.array_equal(_bits(x), _bits(y)):
            continue
        bit_equal = False
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        same = (x64 == y64) | (np.isnan(x64) & np.isnan(y64))
        with np.errstate(invalid="ignore"):
            d = np.where(same, 0.0, np.abs(x64 - y64) / np.maximum(1.0, np.abs(y64)))
        err = max(err, float(np.nan_to_num(d, nan=np.inf).max()))
    print("validity %s / %s / %s: bit-equal %s, max |A - B| / max(1, |B|) = %.3g" % (model, mutator, consumer, bit_equal, err))
    if (model, mutator, consumer) in ROUNDING:
        audit("validity %s/%s/%s" % (model, mutator, consumer), err, TOL)
    else:
        assert bit_equal, "A and B differ (by %g): a table that should have been rebuilt was not, or the reverse" % err
