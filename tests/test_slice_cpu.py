"""Slice sampling, host side: the new entry points in the header and the binding, the translation of the prior objects,
the coordinates FeatureHpSlice builds from the descriptors, and the host twin's own stationarity on closed-form targets.
No device needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import common_amd
from common_amd import _lib as L
from common_amd import hypers, models, scalar_functions as sf
from tests import slice_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("msc_hp_slice", "msc_theta_slice")


def _header():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        return fh.read()


def test_new_symbols_are_declared_and_exported():
    text = _header()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in common_amd.EXPORTS
    assert declared == set(common_amd.EXPORTS)
    assert "typedef struct {" in text and "} msc_slice_coord;" in text


def test_abi_version_is_still_1():
    assert re.search(r"#define MSC_ABI_VERSION 1\b", _header())
    assert L.ABI_VERSION == 1


def test_header_constants_match_the_binding():
    text = _header()
    for name, value in (("FLAT", L.PRIOR_FLAT), ("EXPONENTIAL", L.PRIOR_EXPONENTIAL), ("NORMAL", L.PRIOR_NORMAL),
                        ("NONINF_BETA", L.PRIOR_NONINF_BETA)):
        assert re.search(r"#define MSC_PRIOR_%s %du\b" % (name, value), text), name
    assert "0x2545F4914F6CDD1D" in text and L.SLICE_KEY == sh.KEY_XOR == 0x2545F4914F6CDD1D
    assert L.SLICE_STEP_OUT == sh.M == 64 and L.SLICE_SHRINK == sh.SHRINK == 256
    # msc_slice_coord is 7 four-byte fields, in the header's order
    assert [f for f, _ in L.SliceCoord._fields_] == ["feature", "coord", "width", "prior", "prior_a", "prior_b",
                                                      "partner"]
    assert ctypes.sizeof(L.SliceCoord) == 28


def test_priors_translate_to_msc_prior():
    assert hypers.slice_prior(sf.log_exponential(2.5)) == (L.PRIOR_EXPONENTIAL, 2.5, 0.0)
    assert hypers.slice_prior(sf.log_normal(-1.0, 3.0)) == (L.PRIOR_NORMAL, -1.0, 3.0)
    assert hypers.slice_prior(sf.log_noninformative_beta_prior) == (L.PRIOR_NONINF_BETA, 0.0, 0.0)
    assert hypers.slice_prior(None) == (L.PRIOR_FLAT, 0.0, 0.0)
    # the float32 parameters the objects carry are what the device gets
    assert hypers.slice_prior(sf.log_exponential(0.1))[1] == float(np.float32(0.1))
    for bad in (lambda x: -x, math.log, sf.log_exponential):
        with pytest.raises(TypeError) as e:
            hypers.slice_prior(bad)
        msg = str(e.value)
        assert "log_exponential" in msg and "log_normal" in msg and "log_noninformative_beta_prior" in msg


def test_twin_priors_equal_the_scalar_functions():
    # the device evaluates the priors in double; the objects in float32: they agree to float precision
    for x in (0.05, 0.7, 3.0, 11.0):
        assert abs(sh.log_prior(sh.PRIOR_EXPONENTIAL, x, 1.5, 0, 0) - sf.log_exponential(1.5)(x)) < 1e-5 * (1 + x)
        assert abs(sh.log_prior(sh.PRIOR_NORMAL, x, 0.5, 2.0, 0) - sf.log_normal(0.5, 2.0)(x)) < 1e-5 * (1 + x * x)
        assert abs(sh.log_prior(sh.PRIOR_NONINF_BETA, x, 0, 0, 2.0) - sf.log_noninformative_beta_prior(x, 2.0)) < 1e-5


class _FakeState(object):
    def __init__(self, descs):
        self.features = [(d.family, d.dim) for d in descs]


def _by_feature(coords):
    out = {}
    for c in coords:
        out.setdefault(c["feature"], []).append((c["coord"], c["prior"], c["a"], c["b"], c["partner"], c["width"]))
    return out


def test_feature_hp_slice_builds_the_default_coordinates_and_skips_dd_dm_niw():
    descs = [models.bb, models.bbnc, models.bnb, models.gp, models.nich, models.dd(4), models.dm(3), models.niw(2)]
    s = hypers.FeatureHpSlice(_FakeState(descs), descs)
    assert s.features == [0, 1, 2, 3, 4]
    got = _by_feature(s.coords)
    beta = [(0, L.PRIOR_NONINF_BETA, 0.0, 0.0, 1, 1.0), (1, L.PRIOR_NONINF_BETA, 0.0, 0.0, 0, 1.0)]
    assert got[0] == beta and got[1] == beta and got[2] == beta      # ('alpha', 'beta'): two entries, each the other's partner
    assert got[3] == [(0, L.PRIOR_EXPONENTIAL, 1.0, 0.0, 0, 1.0), (1, L.PRIOR_EXPONENTIAL, 1.0, 0.0, 0, 1.0)]
    assert got[4] == [(0, L.PRIOR_NORMAL, 0.0, 1.0, 0, 1.0), (2, L.PRIOR_EXPONENTIAL, 1.0, 0.0, 0, 1.0)]   # mu, sigmasq
    assert set(got) == {0, 1, 2, 3, 4} and not s.has_alpha
    # explicit priors and widths, alpha, and a feature given no prior at all
    hp = {4: {"kappa": (sf.log_exponential(2.0), 0.5), "nu": (sf.log_exponential(0.5), 3.0)}, 0: {}}
    s = hypers.FeatureHpSlice(_FakeState(descs), descs, hparams=hp, cparam={"alpha": (sf.log_exponential(1.0), 2.0)})
    got = _by_feature(s.coords)
    assert 0 not in got and s.features == [1, 2, 3, 4]
    assert got[4] == [(1, L.PRIOR_EXPONENTIAL, 2.0, 0.0, 0, 0.5), (3, L.PRIOR_EXPONENTIAL, 0.5, 0.0, 0, 3.0)]
    assert s.has_alpha and s.coords[-1]["feature"] == "alpha" and s.coords[-1]["width"] == 2.0
    # a callable that is not one of the three
    with pytest.raises(TypeError):
        hypers.FeatureHpSlice(_FakeState(descs), descs, hparams={3: {"alpha": (lambda x: -x, 1.0)}})
    with pytest.raises(TypeError):
        hypers.FeatureHpSlice(_FakeState(descs), descs, cparam={"alpha": (lambda x: -x, 1.0)})
    # the noninformative beta prior takes a pair, the others one key
    with pytest.raises(ValueError):
        hypers.FeatureHpSlice(_FakeState(descs), descs, hparams={3: {"alpha": (sf.log_noninformative_beta_prior, 1.0)}})
    with pytest.raises(ValueError):
        hypers.FeatureHpSlice(_FakeState(descs), descs, hparams={0: {("alpha", "beta"): (sf.log_exponential(1.), 1.0)}})
    # dd alphas are not sliced
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        hypers.FeatureHpSlice(_FakeState(descs), descs, hparams={5: {"alphas": (sf.log_exponential(1.), 1.0)}})
    assert e.value.code == -4


def _twin_chain(g, in_support, x0, w, n, seed):
    xs = np.empty(n)
    evals = 0
    x = x0
    for t in range(n):
        x, e, status, _ = sh.slice_update(g, in_support, x, w, sh.Uniforms(seed, 0, 0, t))
        assert status == sh.OK
        evals += e
        xs[t] = x
    return xs, evals / n


def test_twin_is_stationary_on_closed_form_targets():
    from scipy import stats
    n = 20000
    # Gate: for 2e4 independent draws the KS distance exceeds 0.0138 with probability 1e-3; a slice chain's draws are
    # correlated (lag-1 autocorrelation 0.05 and 0.23 here), so 0.025 leaves room for an effective sample size down to a
    # third.  Fixed seeds: the outcome is deterministic (0.0133 and 0.0052 when written).
    a, b = 2.5, 4.0
    xs, ev = _twin_chain(lambda x: (a - 1) * math.log(x) + (b - 1) * math.log(1 - x), sh.theta_support, 0.4, 0.3, n, 11)
    d = stats.kstest(xs, stats.beta(a, b).cdf).statistic
    assert d < 0.025, d
    assert 2 < ev < 15
    k, rate = 3.0, 2.0
    xs, ev = _twin_chain(lambda x: (k - 1) * math.log(x) - rate * x, sh.support(True), 1.5, 1.0, n, 12)
    d = stats.kstest(xs, stats.gamma(k, scale=1 / rate).cdf).statistic
    assert d < 0.025, d
    assert 2 < ev < 15


def test_twin_respects_the_support_and_keeps_a_non_finite_start():
    seen = []

    def g(x):
        seen.append(x)
        return -x
    for t in range(200):
        x, _, status, _ = sh.slice_update(g, sh.support(True), 0.01, 5.0, sh.Uniforms(3, 1, 2, t))
        assert status == sh.OK and x > 0
    assert min(seen) > 0
    x, e, status, _ = sh.slice_update(lambda x: -math.inf, sh.support(True), 0.5, 1.0, sh.Uniforms(3, 1, 2, 0))
    assert (x, e, status) == (0.5, 1, sh.NON_FINITE)
    x, e, status, _ = sh.slice_update(g, sh.support(True), -1.0, 1.0, sh.Uniforms(3, 1, 2, 0))
    assert (x, e, status) == (-1.0, 0, sh.NON_FINITE)       # outside the support: never evaluated
