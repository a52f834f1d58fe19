"""Host side of the particle filter over rows (ChainEnsemble.smc): weights, effective sample size, systematic resampling
and the result record.  numpy float64 throughout and no device call, so everything here runs without a GPU.
"""
import collections

import numpy as np


def log_mean_exp(logw):
    """log of the mean of exp(logw); -inf entries count as zero weight, all -inf gives -inf"""
    logw = np.asarray(logw, dtype=np.float64).ravel()
    m = logw.max()
    if not np.isfinite(m):
        return float(m)                         # (all -inf: -inf; a +inf or nan weight propagates)
    return float(m + np.log(np.exp(logw - m).mean()))


def normalised_weights(logw):
    """exp(logw - max) / its sum"""
    logw = np.asarray(logw, dtype=np.float64).ravel()
    m = logw.max()
    if not np.isfinite(m):
        raise ValueError("no particle has a finite log weight")
    w = np.exp(logw - m)
    return w / w.sum()


def ess(logw):
    """effective sample size 1 / sum w^2 of the normalised weights: P for equal weights, 1 when one holds everything"""
    w = normalised_weights(logw)
    return float(1.0 / np.square(w).sum())


def systematic_ancestors(logw, u):
    """Systematic resampling with SURVIVORS IN PLACE -> uint32 [P], a[p] the particle slot p continues from.

    Offspring counts: w the normalised weights, c = cumsum(w) with its last entry set to 1; n_p is the number of the
    positions (u + j) / P, j = 0 .. P - 1, that fall in [c_{p-1}, c_p) -- floor(P w_p) or ceil(P w_p), summing to P.
    Arrangement: a[p] = p wherever n_p >= 1; the remaining n_p - 1 copies of the survivors fill the dead slots in ascending
    order, dealt out in rounds: every round takes the survivors that still have a copy left in ascending order and gives
    each one slot (P = 5, counts (3, 0, 2, 0, 0) -> [0, 0, 2, 2, 0]), so a heavy particle's copies are spread over the
    slots, not packed together.  a[a[p]] == a[p] for every p: a copy never reads a slot that is being overwritten, which
    is what msc_chains_clone requires.  u in [0, 1)."""
    u = float(u)
    if not 0.0 <= u < 1.0:
        raise ValueError("u must lie in [0, 1)")
    w = normalised_weights(logw)
    P = len(w)
    c = np.cumsum(w)
    c[-1] = 1.0
    # position j falls below c_p when u + j < P c_p: ceil(P c_p - u) positions lie below it.  A boundary within rounding
    # of a position (|P c_p - u - j| <= 1e-12 P) counts as ON it, so that equal weights give one offspring each for any
    # u although their cumulative sums are not exact
    t = P * c - u
    near = np.rint(t)
    below = np.ceil(np.where(np.abs(t - near) <= 1e-12 * P, near, t)).astype(np.int64)
    below[-1] = P
    counts = np.diff(np.concatenate(([0], np.clip(below, 0, P))))
    a = np.arange(P, dtype=np.uint32)
    dead = np.flatnonzero(counts == 0)
    left = np.maximum(counts - 1, 0)
    who = np.repeat(np.arange(P, dtype=np.uint32), left)                 # survivor of every spare copy, ascending
    nth = np.arange(len(who)) - np.repeat(np.cumsum(left) - left, left)  # ... and which of its copies it is: the round
    assert len(who) == len(dead), (counts, u)
    a[dead] = who[np.lexsort((who, nth))]
    return a


SMCResult = collections.namedtuple("SMCResult", "log_evidence log_weights weights ess resampled_at ancestors truncated")
SMCResult.__doc__ = """What ChainEnsemble.smc returns.

log_evidence   the estimate of log p(X | hp, alpha): the log mean weights added at every resampling + log_mean_exp of the
               final log weights (taken before a final resampling zeroes them)
log_weights    float64 [P] on the host: the particles' log weights at the end (all 0 after final_resample)
weights        those, normalised
ess            the effective sample size at every checkpoint, then the final one (before a final resampling)
resampled_at   the positions (rows seated so far) of the checkpoints that resampled
ancestors      the ancestor array of each of those
truncated      True if a particle ends with all ngroups slots occupied: the estimate is then for the mixture truncated to
               ngroups slots, not for the exact CRP"""
