"""Grid hyper-parameter inference, host side: the merged grids, their packed blocks and log-priors as upstream defines
them (common_amd/hypers.py), the empty-grid rules of FeatureHpGibbs, and the new entry points in the header and the
binding.  No device needed."""
import os
import re

import numpy as np
import pytest

import common_amd
from common_amd import hypers, models, scalar_functions as sf
from common_amd.runtime import pack_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("msc_hp_grid_create", "msc_hp_grid_destroy", "msc_hp_grid_score", "msc_hp_grid_gibbs")

CURRENT = {
    "bb": {"alpha": 2.5, "beta": 0.75},
    "bbnc": {"alpha": 1.5, "beta": 3.0},
    "bnb": {"alpha": 1.5, "beta": 2.0, "r": 7},
    "gp": {"alpha": 3.0, "inv_beta": 0.5},
    "nich": {"mu": 0.25, "kappa": 4.0, "sigmasq": 2.0, "nu": 6.0},
}


@pytest.mark.parametrize("name", sorted(CURRENT))
def test_default_grids_merge_into_the_current_hp_and_pack_as_pack_hp(name):
    desc = getattr(models, name)
    cur = CURRENT[name]
    partial = desc.default_partial_hypergrid()
    assert len(partial) == 10000
    pts = hypers.merged_points(desc, cur)
    blocks = hypers.grid_blocks(desc, cur)
    assert blocks.shape == (10000, len(pack_hp(desc.family, cur))) and blocks.dtype == np.float32
    for i, (p, m) in enumerate(zip(partial, pts)):
        want = dict(cur)
        want.update(p)
        assert m == want
        if i % 97 == 0:
            assert np.array_equal(blocks[i], pack_hp(desc.family, want))
    # the keys the grid does not name stay at the current hp: nich kappa and nu, bnb r
    fixed = {"nich": ("kappa", "nu"), "bnb": ("r",)}.get(name, ())
    for k in fixed:
        assert all(m[k] == cur[k] for m in pts)
    # and the flat block the state holds merges the same way as its dict
    flat = pack_hp(desc.family, cur)
    assert np.array_equal(hypers.grid_blocks(desc, flat), blocks)


@pytest.mark.parametrize("name", sorted(CURRENT))
def test_grid_logprior_is_the_sum_of_the_hyperpriors_point_by_point(name):
    desc = getattr(models, name)
    pts = hypers.merged_points(desc, CURRENT[name])
    lp = hypers.grid_logprior(desc, pts)
    assert lp.dtype == np.float64 and lp.shape == (len(pts),)
    beta = sf.log_noninformative_beta_prior
    for i in range(0, len(pts), 131):
        p = pts[i]
        if name in ("bb", "bbnc", "bnb"):
            want = beta(p["alpha"], p["beta"])                # the tuple key, called in the tuple's order
        elif name == "gp":
            want = sf.log_exponential(1.)(p["alpha"]) + sf.log_exponential(1.)(p["inv_beta"])
        else:
            want = sf.log_normal(0., 1.)(p["mu"]) + sf.log_exponential(1.)(p["sigmasq"])
        assert lp[i] == want, (i, lp[i], want)


def test_tuple_keys_follow_the_tuple_order():
    pts = [{"a": 2.0, "b": 5.0}]
    pri = {("b", "a"): lambda x, y: x - 10 * y}
    assert hypers.grid_logprior(models.bb, pts, pri)[0] == 5.0 - 20.0


class _FakeState(object):
    """what FeatureHpGibbs asks of a State before it touches the device"""

    def __init__(self, descs):
        self.descs = descs
        self.features = [(d.family, d.dim) for d in descs]
        self.made = []

    def get_hp(self, f):
        d = self.descs[f]
        return pack_hp(d.family, d.default_hyperparams(), d.dim)

    def hp_grid(self, f, blocks, logprior=None):
        self.made.append((f, blocks.shape, logprior.shape))
        return object()

    def crp_grid(self, alphas, logprior=None):
        self.made.append(("alpha", len(alphas)))
        return object()


def test_empty_default_grids_are_skipped_and_explicit_empty_grids_raise():
    descs = [models.dd(4), models.bb, models.niw(2), models.dm(3), models.gp]
    st = _FakeState(descs)
    g = hypers.FeatureHpGibbs(st, descs, cluster_grid=np.logspace(-1, 1, 5))
    assert g.features == [1, 4]
    assert st.made == [(1, (10000, 2), (10000,)), (4, (10000, 2), (10000,)), ("alpha", 5)]
    with pytest.raises(ValueError):
        hypers.FeatureHpGibbs(st, descs, grids=[None, [], None, None, None])
    with pytest.raises(ValueError):
        hypers.FeatureHpGibbs(st, descs, cluster_grid=[])
    # an explicit grid for a family without a default one is taken
    g = hypers.FeatureHpGibbs(st, descs, grids=[[{"alphas": [0.5] * 4}, {"alphas": [2.0] * 4}], None, None, None, None])
    assert g.features == [0, 1, 4]


def test_unpack_hp_inverts_pack_hp():
    for name, cur in CURRENT.items():
        d = getattr(models, name)
        assert hypers.unpack_hp(d.family, pack_hp(d.family, cur)) == {k: float(np.float32(v)) if k != "r" else v
                                                                      for k, v in cur.items()}
    assert hypers.unpack_hp(common_amd.DD, [1.0, 2.0]) == {"alphas": [1.0, 2.0]}
    with pytest.raises(ValueError):
        hypers.unpack_hp(common_amd.NIW, [1.0, 2.0])


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "microscopes_hip.h")).read()
    declared = set(re.findall(r"\b(msc_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in common_amd.EXPORTS, name
    assert "#define MSC_HP_CLUSTER 0xFFFFFFFFu" in hdr and common_amd.HP_CLUSTER == 0xFFFFFFFF
    assert re.search(r"#define MSC_ABI_VERSION 1\b", hdr)


def test_hypers_module_stays_product_code():
    src = open(os.path.join(ROOT, "common_amd", "hypers.py")).read()
    assert "oracle" not in src
