"""The ensemble's slice step, without a GPU: the ABI declares and exports msc_chains_hp_slice and the binding carries its
argument types; hypers.EnsembleHpSlice builds FeatureHpSlice's coordinate list from the same arguments, against a
stand-in with .features and .nchains (constructing it touches no device), and refuses what FeatureHpSlice refuses."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "msc_chains_hp_slice"
SIG = ("int msc_chains_hp_slice(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev, "
       "uint64_t ld_slots, const uint64_t *host_seeds, uint64_t sweep, float *values_host, uint32_t *evals_host);")


def test_header_declares_and_library_exports_the_call():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    import common_amd
    assert SIG in flat
    assert hasattr(C.CDLL(common_amd.LIB_PATH), NAME)
    assert NAME in common_amd.EXPORTS
    assert "#define MSC_ABI_VERSION 1" in flat


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    lib = L.load()          # dlopen only; no device call
    res, args = L._SIGS[NAME]
    params = re.search(NAME + r"\((.*?)\);", SIG).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 9
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(L.SliceCoord)), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    assert args[5] == C.POINTER(C.c_uint64)         # host_seeds: 64-bit keys
    assert getattr(lib, NAME).argtypes == args


def test_python_surface():
    import common_amd
    from common_amd import chains, hypers
    assert callable(common_amd.ChainEnsemble.hp_slice) and callable(common_amd.ChainEnsemble.run)
    assert chains.RunResult._fields == ("trace", "values")
    assert callable(hypers.EnsembleHpSlice)
    assert "hp_slice" in common_amd.ChainEnsemble.smc.__doc__      # (unbiasedness needs shared hp and alpha)


class _Ens(object):
    """what EnsembleHpSlice reads of an ensemble when it is built"""

    def __init__(self, features, nchains=3):
        self.features, self.nchains = list(features), nchains


class _State(object):
    def __init__(self, features):
        self.features = list(features)


def _descs():
    from common_amd import models
    return [models.bb, models.gp, models.bnb, models.dd(5), models.nich]


def _features(descs):
    return [(d.family, d.dim) for d in descs]


def test_ensemble_builds_the_states_coordinate_list():
    from common_amd import hypers
    from common_amd.scalar_functions import log_exponential, log_normal
    descs = _descs()
    feats = _features(descs)
    cases = [
        dict(),
        dict(cparam={"alpha": (log_exponential(1.0), 2.0)}),
        dict(hparams={4: {"mu": (log_normal(0.0, 4.0), 0.5), "nu": (log_exponential(0.5), 3.0)}},
             cparam={"alpha": (None, 1.0)}),
        dict(hparams=[None, {"alpha": (log_exponential(2.0), 0.25)}, None, {}, None]),
        dict(hparams={f: {} for f in range(5)}),
    ]
    for kw in cases:
        one = hypers.FeatureHpSlice(_State(feats), descs, **kw)
        ens = hypers.EnsembleHpSlice(_Ens(feats), descs, **kw)
        assert ens.coords == one.coords and ens.features == one.features and ens.has_alpha == one.has_alpha
        assert ens.last_evals is None
    # dd contributes no coordinate by default; every other descriptor does, and alpha comes last
    ens = hypers.EnsembleHpSlice(_Ens(feats), descs, cparam={"alpha": (log_exponential(1.0), 2.0)})
    assert ens.features == [0, 1, 2, 4] and ens.coords[-1]["feature"] == "alpha"
    assert all(c["feature"] != 3 for c in ens.coords)


def test_ensemble_with_nothing_to_slice_steps_without_a_device():
    from common_amd import hypers
    descs = _descs()
    ens = hypers.EnsembleHpSlice(_Ens(_features(descs), nchains=4), descs, hparams={f: {} for f in range(5)})
    assert ens.coords == [] and ens.step(1, 0) == [{}, {}, {}, {}]
    assert ens.last_evals.shape == (4, 0) and ens.last_values.shape == (4, 0)


def test_ensemble_argument_errors_are_the_states():
    from common_amd import hypers, models
    from common_amd._lib import MicroscopesHipError
    from common_amd.scalar_functions import log_exponential, log_noninformative_beta_prior
    descs = _descs()
    feats = _features(descs)
    bad = [
        (ValueError, dict(descs=descs[:-1])),                                                # one descriptor short
        (ValueError, dict(descs=[models.bb, models.gp, models.bnb, models.dd(6), models.nich],
                          hparams={3: {}})),                                                 # (dd skipped: no error) ...
        (ValueError, dict(descs=[models.gp, models.gp, models.bnb, models.dd(5), models.nich])),   # ... a sliced one is
        (ValueError, dict(cparam={"beta": (None, 1.0)})),
        (ValueError, dict(cparam={"alpha": (log_noninformative_beta_prior, 1.0)})),
        (ValueError, dict(hparams={0: {"alpha": (log_noninformative_beta_prior, 1.0)}})),  # the pair prior on one key
        (ValueError, dict(hparams={4: {"lambda": (log_exponential(1.0), 1.0)}})),            # no such hyper-parameter
        (TypeError, dict(hparams={4: {"mu": (lambda x: 0.0, 1.0)}})),                        # not a scalar_functions prior
        (MicroscopesHipError, dict(hparams={3: {"alphas": (log_exponential(1.0), 1.0)}})),   # dd is not sliced
    ]
    for i, (exc, kw) in enumerate(bad):
        kw = dict(kw)
        ds = kw.pop("descs", descs)
        raised = []
        for build in (lambda: hypers.FeatureHpSlice(_State(feats), ds, **kw),
                      lambda: hypers.EnsembleHpSlice(_Ens(feats), ds, **kw)):
            if i == 1:
                build()                      # a skipped feature's descriptor is not compared: neither class objects
                continue
            with pytest.raises(exc) as e:
                build()
            raised.append(str(e.value))
        if raised:
            assert raised[0] == raised[1], i
