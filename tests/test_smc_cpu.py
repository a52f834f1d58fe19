"""The particle filter over rows, without a GPU: the ABI declares and exports msc_chains_visit / msc_chains_clone and the
binding carries their argument types; the host helpers of common_amd.smc (weights, ESS, systematic resampling with
survivors in place) on hand-made weights; and the yardsticks of the GPU tests -- the evidence gates (E1) and (E2) of
tests/test_gpu_smc.py -- hold for the same filter run over the double replay of the chain."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import smc_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "msc_chains_visit":
        "int msc_chains_visit(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows, "
        "uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order, uint64_t pos0, "
        "uint64_t npos, const uint64_t *host_seeds, uint64_t sweep, double *logw_dev, float *visit_logp_dev, "
        "uint64_t ld_logp);",
    "msc_chains_clone":
        "int msc_chains_clone(msc_chains *ch, const uint32_t *host_ancestors, int32_t *z_dev, uint64_t ld_z, uint64_t nrows);",
}


def test_header_declares_and_library_exports_the_calls():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    import common_amd
    lib = C.CDLL(common_amd.LIB_PATH)
    for name, sig in SIGS.items():
        assert sig in flat, sig
        assert hasattr(lib, name), name
        assert name in common_amd.EXPORTS
    assert "#define MSC_ABI_VERSION 1" in flat


def test_binding_carries_the_argument_types():
    from common_amd import _lib as L
    lib = L.load()          # dlopen only; no device call
    for name, sig in SIGS.items():
        res, args = L._SIGS[name]
        # one ctypes argument per parameter of the declaration, 64-bit where it says uint64_t
        params = re.search(name + r"\((.*?)\);", sig).group(1).split(", ")
        assert res is C.c_int and len(args) == len(params) == {"msc_chains_visit": 17, "msc_chains_clone": 5}[name]
        for p, a in zip(params, args):
            if "*" in p:
                assert a in (C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)), p
            else:
                assert p.startswith("uint64_t") and a is C.c_uint64, p
        assert getattr(lib, name).argtypes == args


def test_exports():
    import common_amd
    assert common_amd.smc.SMCResult is common_amd.SMCResult and "smc" in common_amd.__all__
    assert common_amd.SMCResult._fields == ("log_evidence", "log_weights", "weights", "ess", "resampled_at", "ancestors",
                                            "truncated")
    for name in ("visit", "clone", "smc"):
        assert callable(getattr(common_amd.ChainEnsemble, name))


# ---- weights ---------------------------------------------------------------------------------------------------------------
def test_log_mean_exp_and_ess_closed_forms():
    from common_amd.smc import ess, log_mean_exp
    with np.errstate(divide="ignore"):
        assert log_mean_exp(np.log([1.0, 3.0])) == pytest.approx(math.log(2.0), abs=1e-15)
        assert log_mean_exp(np.log([1.0, 3.0, 0.0])) == pytest.approx(math.log(4.0 / 3.0), abs=1e-15)    # a -inf weight
        assert log_mean_exp([-1000.0, -1000.0]) == pytest.approx(-1000.0, abs=1e-12)                     # no underflow
        assert log_mean_exp([700.0, 710.0]) == pytest.approx(710.0 + math.log((1.0 + math.exp(-10.0)) / 2.0), abs=1e-12)
        assert log_mean_exp([-np.inf, -np.inf]) == -np.inf
        assert ess(np.zeros(9)) == pytest.approx(9.0, abs=1e-12)
        assert ess([5.0, 5.0, 5.0, 5.0]) == pytest.approx(4.0, abs=1e-12)                                # shift-invariant
        assert ess(np.log([1.0, 0.0, 0.0])) == pytest.approx(1.0, abs=1e-15)
        assert ess(np.log([0.5, 0.5, 0.0])) == pytest.approx(2.0, abs=1e-12)
        assert ess(np.log([0.5, 0.25, 0.25])) == pytest.approx(1.0 / (0.25 + 0.0625 + 0.0625), abs=1e-12)
    with pytest.raises(ValueError):
        ess([-np.inf, -np.inf])


# ---- systematic resampling -------------------------------------------------------------------------------------------------
def _offspring(a):
    return np.bincount(a, minlength=len(a))


def _check_arrangement(w, u):
    from common_amd.smc import systematic_ancestors
    w = np.asarray(w, dtype=np.float64)
    P = len(w)
    with np.errstate(divide="ignore"):
        a = systematic_ancestors(np.log(w), u)
    assert a.dtype == np.uint32 and a.shape == (P,)
    n = _offspring(a)
    pw = P * w / w.sum()
    assert n.sum() == P and np.all(n >= np.floor(pw - 1e-12)) and np.all(n <= np.ceil(pw + 1e-12)), (w, u, a)
    assert np.array_equal(a[a], a)                                   # a source survives in place ...
    alive = n >= 1
    assert np.array_equal(a[alive], np.flatnonzero(alive))           # ... every survivor does
    # the dead slots, in ascending order, take the spare copies dealt in rounds over the ascending survivors
    spare, want = np.maximum(n - 1, 0), []
    while spare.any():
        for p in np.flatnonzero(spare > 0):
            want.append(p)
            spare[p] -= 1
    assert list(a[~alive]) == want, (w, u, a)
    return a


def test_systematic_ancestors_on_hand_made_weights():
    from common_amd.smc import systematic_ancestors
    assert list(_check_arrangement([0.5, 0, 0.5, 0, 0], 0.1)) == [0, 0, 2, 2, 0]
    assert list(_check_arrangement([0.1, 0.2, 0.3, 0.4], 0.5)) == [3, 1, 2, 3]
    assert list(_check_arrangement([0, 0, 0, 1], 0.7)) == [3, 3, 3, 3]
    assert list(_check_arrangement([0.05, 0.05, 0.9, 0, 0, 0, 0, 0, 0, 0], 0.3)) == [0, 2, 2, 2, 2, 2, 2, 2, 2, 2]
    for u in (0.0, 0.25, 0.5, 0.999999):
        assert list(_check_arrangement(np.ones(7), u)) == list(range(7))           # equal weights: the identity
        assert list(_check_arrangement([1, 0, 0, 0, 0, 0], u)) == [0] * 6          # one particle holds all the weight
        assert list(systematic_ancestors([-3.0] * 5, u)) == list(range(5))
    rng = np.random.default_rng(5)
    for _ in range(200):
        P = int(rng.integers(1, 40))
        w = rng.random(P) ** 8 * (rng.random(P) < 0.7)
        if w.sum() == 0:
            w[0] = 1.0
        _check_arrangement(w, rng.random())
    # unbiased: over u the mean offspring count of particle p is P w_p
    w = np.array([0.37, 0.03, 0.21, 0.0, 0.39])
    with np.errstate(divide="ignore"):
        mean = np.mean([_offspring(systematic_ancestors(np.log(w), (j + 0.5) / 4000)) for j in range(4000)], axis=0)
    assert np.allclose(mean, 5 * w, atol=2e-3), mean
    with pytest.raises(ValueError):
        systematic_ancestors([0.0, 0.0], 1.0)
    with pytest.raises(ValueError):
        systematic_ancestors([-np.inf, -np.inf], 0.5)


# ---- the gates of the GPU tests, on the double replay ----------------------------------------------------------------------
N6, K6, ALPHA6 = 6, 8, 1.0


@pytest.fixture(scope="module")
def six_rows():
    """{name: (replay features, exact log p(X))} of the two six-row datasets"""
    out = {}
    for name, feats in H.six_row_datasets().items():
        rfeats = H.replay_features(feats)
        out[name] = (rfeats, H.exact_log_evidence(rfeats, ALPHA6))
    return out


def test_exact_evidence_is_a_normalised_density(six_rows):
    """the yardstick itself: for the bb column log p(X) summed over all 2^6 datasets is log 1"""
    from scipy.special import logsumexp
    rfeats, _ = six_rows["bb"]
    F = rfeats[0][0]
    total = logsumexp([H.exact_log_evidence([(F, np.array([(b >> i) & 1 for i in range(N6)], dtype=np.bool_), None)], ALPHA6)
                       for b in range(1 << N6)])
    assert abs(total) < 1e-9, total


@pytest.mark.parametrize("name", ["bb", "nich"])
def test_gate_e1_holds_for_the_replay(six_rows, name):
    """(E1) 512 particles, no resampling: |log_evidence - exact| <= 5 se + 1e-4, se the delta-method standard error"""
    rfeats, exact = six_rows[name]
    r = H.replay_smc(rfeats, K6, ALPHA6, 512, np.random.default_rng(11), ess_threshold=0.0)
    se = H.evidence_se(r["weights"])
    print("E1 replay %s: exact %.5f, estimate %.5f, se %.5f, t %.2f" % (name, exact, r["log_evidence"], se,
                                                                         (r["log_evidence"] - exact) / se))
    assert r["resampled_at"] == [] and len(r["ess"]) == N6 and not r["truncated"]
    assert abs(r["log_evidence"] - exact) <= 5 * se + 1e-4


@pytest.mark.parametrize("name", ["bb", "nich"])
def test_gate_e2_holds_for_the_replay(six_rows, name):
    """(E2) 16 runs of 64 particles resampled every 2 rows: the mean of exp(log_evidence - exact) is 1 within 5 of its
    standard errors"""
    rfeats, exact = six_rows[name]
    rng = np.random.default_rng(12)
    runs = [H.replay_smc(rfeats, K6, ALPHA6, 64, rng, block=2, ess_threshold=float("inf")) for _ in range(16)]
    assert all(r["resampled_at"] == [2, 4] for r in runs)
    ratio = np.exp(np.array([r["log_evidence"] for r in runs]) - exact)
    sem = ratio.std(ddof=1) / math.sqrt(len(ratio))
    print("E2 replay %s: mean ratio %.5f, sem %.5f, t %.2f" % (name, ratio.mean(), sem, (ratio.mean() - 1) / sem))
    assert abs(ratio.mean() - 1.0) <= 5 * sem
