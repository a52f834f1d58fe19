"""Host side of a tempered ensemble.  Chain c at temperature beta targets pi_beta(z) ~ p(z | alpha) p(X | z, hp)^beta: beta = 1
is the posterior, beta = 0 the CRP prior.  The device side is ChainEnsemble.sweep(beta=) (msc_chains_sweep_tempered: every
chain swept at its own temperature), ChainEnsemble.exchange (msc_chains_exchange: neighbouring rungs of a ladder swap
temperatures) and ChainEnsemble.anneal_weights (msc_chains_anneal_weights: the weight of a step of annealed importance
sampling); the drivers over them are ChainEnsemble.run_tempered (replica exchange) and ChainEnsemble.ais (annealed
importance sampling).  Here: the temperature ladders, the exchange's Philox key, the checks of an annealing schedule, the
drivers' result types and the samples a chain took on a rung.  Nothing here calls the library; cold_samples indexes the
tensors it is given, on whatever device they live.
"""
import collections

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



# the key of the exchange's uniforms is the first chain's key xor this.  No chain's sweep key seed + c (c < 2^32) can equal
# it -- adding c changes bits 32 .. 63 by nothing or by a carry, an xor of 0 or of 0..01..1, and the constant's upper half
# 0x9E3779B9 is neither -- and it is not the slice steps' xor either (0x2545F4914F6CDD1D).
EXCHANGE_KEY_XOR = 0x9E3779B97F4A7C15
_U64 = (1 << 64) - 1


def exchange_key(seed):
    """the Philox key run_tempered gives ChainEnsemble.exchange: the first chain's key -- seed itself for an int, the
    first entry of a sequence of per-chain keys -- xor 0x9E3779B97F4A7C15"""
    first = int(seed) if isinstance(seed, (int, np.integer)) else int(list(seed)[0])
    return (first & _U64) ^ EXCHANGE_KEY_XOR


def cold_samples(trace, rungs, rung=0):
    """the samples of a run_tempered trace whose chain held `rung` when they were taken (0: the ladder's first
    temperature, the posterior when betas[0] = 1) -> [count, nrows], chain by chain and within a chain in sample order.
    trace [nchains, ns, nrows] and rungs [nchains, ns]: torch tensors on one device, CPU ones included (on a GPU the
    boolean index waits for the device)."""
    if trace.dim() != 3 or rungs.dim() != 2 or tuple(trace.shape[:2]) != tuple(rungs.shape):
        raise ValueError("trace must be [nchains, ns, nrows] and rungs [nchains, ns]")
    return trace[rungs == int(rung)]


def ais_betas(betas):
    """the schedule of ChainEnsemble.ais as the float32 host array the device sees: non-decreasing, from exactly 0 to
    exactly 1; anything else (NaN included) is a ValueError"""
    b = np.asarray(betas, dtype=np.float32).ravel()
    if b.size < 1 or b[0] != 0.0:
        raise ValueError("betas must start at 0 (the CRP prior, which the chains are drawn from)")
    if b[-1] != 1.0:
        raise ValueError("betas must end at 1 (the posterior)")
    if not np.all(np.diff(b) >= 0.0):
        raise ValueError("betas must be non-decreasing")
    return b


TemperedResult = collections.namedtuple("TemperedResult", "trace rungs beta rung proposed accepted joint")
TemperedResult.__doc__ = """What ChainEnsemble.run_tempered returns; every field a device tensor.

trace      int32 [nchains, niters // trace_every, nrows], every chain's z after each trace_every-th iteration's sweep
           (before its exchange); None without trace_every
rungs      int32 [nchains, niters // trace_every], the rung every chain held when that sample was taken (None likewise):
           a chain's trace is a path through the temperatures, cold_samples(trace, rungs, j) picks rung j's samples
beta       float32 [nchains], the temperature every chain holds at the end
rung       int32 [nchains], the rung every chain holds at the end (within a ladder a permutation of 0 .. R - 1)
proposed   int32 [nchains // R, R - 1], swaps proposed per ladder and pair (j, j + 1), over this run and the runs it continues
accepted   int32 [nchains // R, R - 1], swaps accepted likewise
joint      float64 [nchains, nfeatures + 3], ChainEnsemble.score_joint's rows of the last iteration (unwritten at niters = 0)

Passed as state= to run_tempered, a run continues from copies of beta, rung, proposed and accepted."""

AISResult = collections.namedtuple("AISResult", "log_evidence log_weights weights ess truncated")
AISResult.__doc__ = """What ChainEnsemble.ais returns.

log_evidence   the estimate of log p(X | hp, alpha): smc.log_mean_exp of the log weights
log_weights    float64 host array [nchains], every chain's log importance weight
weights        the same normalised to sum 1
ess            the effective sample size of the weights, between 1 and nchains
truncated      True when some chain had all ngroups slots occupied at the end of some sweep: a new group may have been
               refused there, and the estimate is for the mixture truncated to ngroups slots (an end-of-sweep check)"""
