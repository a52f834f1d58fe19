"""The host side of tests/test_gpu_heavy_chains.py (tests/heavy_chain_cases.py) without a device: the visits' plan is
well formed, few darts lie on a step of the fixture's CDF, the exact tables agree with a plain recomputation, and the
ensemble predictive's tile plan is what the GPU test says it is."""
from fractions import Fraction

import numpy as np
import pytest

from tests import heavy_cases as hc
from tests import heavy_chain_cases as cc

_lay = pytest.mark.parametrize("K", cc.LAYOUTS, ids=["rungs", "K300"])
_V = {}


def visits(K):
    if K not in _V:
        _V[K] = cc.Visits(K)
    return _V[K]


def test_score_assignment_of_the_layouts_is_in_the_fixture():
    """the CRP term of every layout, against a double evaluation (lgamma of 1e8 is 1.7e9: double holds the sum to ~1e-6
    absolute, far inside 1e-12 relative)"""
    import math
    sa = hc.load_score_assignment()
    assert sorted(sa) == sorted(hc.LAYOUT_KEYS)
    a = float(hc.ALPHA32)
    for key, (R, K) in hc.LAYOUT_KEYS.items():
        c = [int(x) for x in hc.layout_counts(R, K) if x > 0]
        twin = len(c) * math.log(a) + math.fsum(math.lgamma(x) for x in c) + math.lgamma(a) - math.lgamma(sum(c) + a)
        assert abs(twin - sa[key]) <= 1e-12 * abs(sa[key]), (key, twin, sa[key])
    for names in ([n] for n in hc.FAMILIES if not n.startswith("niw")):      # (niw has 14 rungs and no score_joint)
        for K in (None, 300):
            KK, rung, counts = hc.layout(names, K)
            assert np.array_equal(counts, hc.layout_counts(16, KK))


@_lay
def test_the_visits_cover_every_value_and_every_rung_a_row_can_leave(K):
    v = visits(K)
    assert v.nrows <= 100 and cc.NCHAINS <= 128 and v.total < 2 ** 32
    assert (v.K, v.total) in ((16, 220202080), (300, 3963839520))
    for i, nm in enumerate(cc.NAMES):
        assert len(np.unique(v.vidx[i])) == len(hc.values(nm))
    assert set(v.row_of) == set(range(v.nrows))
    own = v.z >= 0
    assert v.ok[np.nonzero(own)[0], v.z[own]].all()              # every assigned row can leave its group
    assert np.array_equal(np.unique(v.rung[v.z[own]]), np.unique(v.rung[np.nonzero(v.ok.any(axis=0))[0]]))
    assert (~own).any() and np.all(np.isfinite(v.inc))
    # the near-mean rows: one in a lopsided 1e8 group, one unassigned whose dart lies well inside that group's share
    assert v.rung[v.lop] == cc.LOPSIDED_1E8 and v.counts[v.lop] == 10 ** 8 and v.zfull[v.n] == v.lop and v.zfull[v.n + 1] == -1
    assert cc.want_draw(v.t_join, v.u[v.n + 1]) == v.lop and not cc.near_edge(v.t_join, v.u[v.n + 1])
    for x in cc.NEAR_MEAN:
        assert Fraction(float(x)).denominator <= 16 and abs(float(x) + 1000.5) <= 0.125


@_lay
def test_few_darts_lie_on_a_cdf_step(K):
    """the share of visits whose dart lies within 1e-5 of a step of the fixture's CDF, for the untempered visits (b) and
    the tempered ones (d): below 0.02, so that the 0.98 agreement the GPU tests ask for is no accident of the seed"""
    plain, tempered = visits(K).near_share()
    print("K = %s: near-step share %.4f (untempered), %.4f (tempered)" % (K, plain, tempered))
    assert plain < 0.02 and tempered < 0.02


def test_tempered_totals():
    v = visits(None)
    j = 5
    assert np.array_equal(v.t_tempered(j, np.float32(1.0)), v.t[j])
    assert np.array_equal(v.t_tempered(j, np.float32(0.0)), v.crp[j])
    half = v.t_tempered(j, np.float32(0.5))
    assert np.allclose(half - v.crp[j], 0.5 * v.feat[j], rtol=1e-15, atol=0)
    assert list(v.beta_d) == [1.0, 0.5, 0.25, 0.0] * 2 and all(v.keys_d[r][0] == v.seeds[r] for r in range(v.n))


def test_exact_group_is_the_plain_moments():
    """ExactGroup on a group of real rows: leave and join against the moments recomputed from the rows"""
    rows = [dict(bb=bool(i % 2), gp=3 * i, bnb=i, dd=i % 7, nich=float(np.float32(0.75 + i / 8.0))) for i in range(6)]
    g = cc.ExactGroup(0)                                             # rung 0: empty
    assert g.n == 0 and g.nich() == (0, 0)
    for r in rows:
        g.move(r, +1)
    g.move(rows[2], -1)
    kept = [r for i, r in enumerate(rows) if i != 2]
    xs = [Fraction(r["nich"]) for r in kept]
    mean = sum(xs) / len(xs)
    assert g.nich() == (mean, sum((x - mean) ** 2 for x in xs))
    assert g.bb == [sum(r["bb"] for r in kept), sum(not r["bb"] for r in kept)]
    assert g.gp == [5, sum(r["gp"] for r in kept)] and g.bnb == [5, sum(r["bnb"] for r in kept)]
    assert g.dd == [sum(r["dd"] == c for r in kept) for c in range(7)]
    # a heavy rung: the near-mean row leaves the lopsided 1e8 group
    g = cc.ExactGroup(cc.LOPSIDED_1E8)
    x = Fraction(float(cc.NEAR_MEAN[0]))
    g.move(dict(cc.NEAR_ROW, nich=float(cc.NEAR_MEAN[0])), -1)
    n, m = 10 ** 8, Fraction(-2001, 2)
    mean, ctv = g.nich()
    assert mean == (n * m - x) / (n - 1) and ctv == 10 ** 4 + n * m * m - x * x - (n * m - x) ** 2 / (n - 1)
    assert abs(float(ctv) - 1e4) < 0.02


def test_ensemble_predictive_tile_plans():
    """which instantiation of k_chains_marginal the heavy states take (route_calls.hpp plan_chains_marginal)"""
    for K, wide in ((16, False), (300, True)):
        for vmax, large in ((None, True), (1023, True), (1000, False)):
            p = cc.cm_plan(cc.NAMES, K, vmax)
            assert (p["wide"], p["large"]) == (wide, large), (K, vmax, p)
            assert p["staged"] == [True, False, False, True, True]
    assert cc.cm_plan(cc.NAMES, 300)["TG"] == 288                     # two tiles: 288 groups and 12
