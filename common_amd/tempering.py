"""Host side of a tempered ensemble: temperature ladders.  Chain c at temperature beta targets
pi_beta(z) ~ p(z | alpha) p(X | z, hp)^beta: beta = 1 is the posterior, beta = 0 the CRP prior.  The device side is
ChainEnsemble.exchange (msc_chains_exchange: neighbouring rungs of a ladder swap temperatures) and
ChainEnsemble.anneal_weights (msc_chains_anneal_weights: the weight of a step of annealed importance sampling).  numpy
only; nothing here calls the library.
"""
import numpy as np


def ladder(nrungs, kind="geometric", beta_min=0.0):
    """nrungs temperatures descending from 1 -> float32 host array; rung 0 is the posterior.
    linear: equal steps from 1 down to beta_min.  geometric: beta_j = beta_min^(j / (nrungs - 1)) for beta_min > 0; with
    beta_min = 0 the last rung is exactly 0 (the prior, whose chains move freely between modes) and the rungs above it
    halve: 1, 1/2, 1/4, ...  One rung is (1,)."""
    nrungs, beta_min = int(nrungs), float(beta_min)
    if nrungs < 1:
        raise ValueError("nrungs must be >= 1")
    if not 0.0 <= beta_min < 1.0:
        raise ValueError("beta_min must lie in [0, 1)")
    if kind not in ("geometric", "linear"):
        raise ValueError("kind must be 'geometric' or 'linear'")
    j = np.arange(nrungs, dtype=np.float64)
    if nrungs == 1:
        b = np.ones(1)
    elif kind == "linear":
        b = 1.0 - j * (1.0 - beta_min) / (nrungs - 1)
        b[-1] = beta_min
    elif beta_min > 0.0:
        b = beta_min ** (j / (nrungs - 1))
        b[-1] = beta_min
    else:
        b = 0.5 ** j
        b[-1] = 0.0
    return b.astype(np.float32)

