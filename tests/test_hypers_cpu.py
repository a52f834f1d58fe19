"""The hyperparameter blocks of gpu_helpers.distinct_hp discriminate: on the double twin alone, every plausible way of
misreading a block -- two fields swapped, a field taken for 1, mu negated / zeroed / reversed, alphas reversed / rotated /
flattened, psi taken for I or its diagonal or flipped, nu = dim, kappa and nu exchanged, inv_beta inverted -- moves the
scores of the prior-only group far beyond the gate the device tests hold (tests/test_gpu_hypers.py).  With the all-one
defaults of make_feature most of these mutants change nothing at all, which is why the device tests need other values."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.gpu_helpers import MIXED, TOL, distinct_hp, edge_assignment, make_feature, rel_err, state_from_assignment

N, K = 256, 8
CASES = [(orc.BB, 0), (orc.BBNC, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 5), (orc.DD, 128), (orc.DM, 4), (orc.NICH, 0),
         (orc.NIW, 3), (orc.NIW, 20)]


def _swap(hp, a, b):
    return dict(hp, **{a: hp[b], b: hp[a]})


def mutants(family, dim, hp):
    """-> {name: mutated block}"""
    out = {}
    positive = [k for k in hp if k not in ("alphas", "mu", "psi", "r")]
    for a in range(len(positive)):
        for b in range(a + 1, len(positive)):
            out["swap_%s_%s" % (positive[a], positive[b])] = _swap(hp, positive[a], positive[b])
    for k in positive + (["r"] if family == orc.BNB else []):
        out[k + "_is_1"] = dict(hp, **{k: 1 if k == "r" else 1.0})
    if family == orc.GP:
        out["inv_beta_inverted"] = dict(hp, inv_beta=1.0 / hp["inv_beta"])
    if family in (orc.DD, orc.DM):
        a = np.asarray(hp["alphas"], dtype=np.float64)
        out["alphas_reversed"] = dict(alphas=list(a[::-1]))
        out["alphas_rotated"] = dict(alphas=list(np.roll(a, 1)))
        out["alphas_rotated_back"] = dict(alphas=list(np.roll(a, -1)))
        out["alphas_all_ones"] = dict(alphas=[1.0] * dim)
        out["alphas_all_mean"] = dict(alphas=[float(a.mean())] * dim)
    if family == orc.NICH:
        out["mu_negated"] = dict(hp, mu=-hp["mu"])
        out["mu_zeroed"] = dict(hp, mu=0.0)
    if family == orc.NIW:
        mu, psi = np.asarray(hp["mu"]), np.asarray(hp["psi"])
        out["mu_negated"] = dict(hp, mu=-mu)
        out["mu_zeroed"] = dict(hp, mu=np.zeros(dim))
        out["mu_reversed"] = dict(hp, mu=mu[::-1].copy())
        out["psi_is_I"] = dict(hp, psi=np.eye(dim))
        out["psi_diagonal"] = dict(hp, psi=np.diag(np.diag(psi)))
        out["psi_flipped"] = dict(hp, psi=psi[::-1, ::-1].copy())
        out["nu_is_dim"] = dict(hp, nu=float(dim))
    return out


def _moved(got, base):
    """share of the entries that left the base by more than 100 gates (an entry the mutant makes undefined has moved)"""
    assert np.isfinite(base).all()
    return float((~(rel_err(got, base) <= 100 * TOL)).mean())


def outputs(f, z, hp):
    """the twin's plain matrix, leave-one-out matrix and score_data of every group under hp, on the FLOAT state the
    device would hold (the suff-stats do not depend on the block: bbnc's p is state)"""
    F, ss64, _ = state_from_assignment([dict(f, hp=hp)], K, z)[0]
    return F.score_matrix(ss64, f["values"]), F.score_matrix(ss64, f["values"], z), F.score_data_all(ss64)


@pytest.mark.parametrize("family,dim", CASES, ids=["%s%s" % (orc.FAMILY_NAMES[f], d or "") for f, d in CASES])
def test_every_mutant_of_the_block_moves_the_prior_only_scores(family, dim):
    rng = np.random.default_rng(family * 1000 + dim)
    hp = distinct_hp(family, dim)
    f = make_feature(family, N, K, rng, dim, hp=hp)
    z = edge_assignment(N, K, rng)
    counts = np.bincount(z[z >= 0], minlength=K)
    assert counts[K - 1] == 0 and counts[K - 2] == 1
    base = outputs(f, z, hp)
    muts = mutants(family, dim, hp)
    assert len(muts) >= 3
    for name, mhp in sorted(muts.items()):
        got = outputs(f, z, mhp)
        if family == orc.BBNC:                         # (the block enters score_data alone: the populated groups')
            pop = counts > 0
            share = _moved(got[2][pop], base[2][pop])
        else:                                          # the empty group's column, plain and leave-one-out (the same numbers)
            share = min(_moved(got[i][:, K - 1], base[i][:, K - 1]) for i in (0, 1))
        print("%s%s %s: share moved %.3f" % (orc.FAMILY_NAMES[family], dim or "", name, share))
        assert share >= 0.5, (name, share)


def test_the_blocks_are_dyadic_distinct_and_differ_between_features():
    used = [(f, d, 0) for f, d in CASES + [(orc.NIW, 40), (orc.NIW, 100)]] + [(f, d, j) for j, (f, d) in enumerate(MIXED)]
    for family, dim, i in used:
        hp = distinct_hp(family, dim, i)
        block = orc.pack_hp(family, hp, dim)
        wide = np.concatenate([np.atleast_1d(np.asarray(hp[k], dtype=np.float64)).ravel() for k in hp])
        assert np.array_equal(np.sort(block.astype(np.float64)), np.sort(wide)), (family, dim, i)   # float holds it exactly
        # dyadic with few bits: all but psi, which is rounded to float (the assertion above) and not to a grid
        grid = np.concatenate([np.atleast_1d(np.asarray(hp[k], dtype=np.float64)).ravel() for k in hp if k != "psi"])
        assert np.array_equal(grid * 8.0, np.round(grid * 8.0)), (family, dim, i)
        scal = [float(v) for v in hp.values() if np.ndim(v) == 0]
        assert len(set(scal)) == len(scal) and 1.0 not in scal and 0.0 not in scal, (family, i, scal)
        if family in (orc.DD, orc.DM):
            assert 1.0 not in hp["alphas"] and all(a != b for a, b in zip(hp["alphas"], hp["alphas"][1:]))
        if i:
            assert not np.array_equal(block, orc.pack_hp(family, distinct_hp(family, dim, 0), dim))
        if family == orc.NIW:
            psi = np.asarray(hp["psi"])
            assert np.array_equal(psi, psi.T) and np.linalg.eigvalsh(psi).min() >= 1.5 - 1e-5
            assert np.abs(psi - np.diag(np.diag(psi))).max() > 0.1       # (dense: the off-diagonal part matters)
