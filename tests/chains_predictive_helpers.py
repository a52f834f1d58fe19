"""Yardsticks of the ensemble's posterior predictive draws (ChainEnsemble.sample_predictive,
msc_chains_sample_predictive): the cases both test files use, the draw's Philox uniforms restated in numpy, and the
running-sum rule of both discrete draws in float64 with the rows it cannot decide.

Undecided rows (the issue's definitions).  The chain draw compares u1 S with the running sums of e_c = exp(a_c - M); the
device forms the same sums in the same order from the same bits, so the two sides differ by the last bits of exp alone:
a row is undecided if |u1 S - cum_c| <= 1e-12 nchains S for some c, and at most 1 row in 1000 may be.  The group draw is
checked against the chosen chain's totals from another kernel (State.score_value), each within g_r = max_k 1e-6 max(1,
|t_k|) of the draw's own: every e_k moves by a factor within exp(+-g_r), the normalised running sum by at most 2 g_r,
so a row is undecided if u2 lies within 2 g_r + 1e-12 of a boundary; at most 5 % of a case's rows may be."""
import numpy as np

from oracle import oracle as orc
from tests import chains_marginal_helpers as M
from tests.gpu_helpers import crp_prior_matrix

PICK_KEY = 0xC2B2AE3D27D4EB4F
CHAIN_CAP, GROUP_CAP = 1e-3, 0.05
SEED, SWEEP = 20240611, 3
N_TRAIN = 400

NICH1 = [(orc.NICH, 0)]
MIX = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 5), (orc.NICH, 0), (orc.BNB, 0)]
WIDE = [(orc.BB, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 33), (orc.NICH, 0), (M.NOOP, 0)]
# name: (specs, K, chains, held-out rows, build_twin's keywords, share of rows given counts beyond the exact table)
CASES = {
    "nich_k8_70_chains": (NICH1, 8, 70, 65, {}, 0.0),                     # more chains than rows, a gather per lane
    "mix_k64_masked": (MIX, 64, 5, 1000, dict(used=60, masked=(0, 1, 2, 3, 4)), 0.0),
    "wide_k300_big_counts": (WIDE, 300, 3, 513, dict(used=290), 0.03),    # the large-count instantiation; K no multiple of 8
    "nich_k8_3_chains_4100_rows": (NICH1, 8, 3, 4100, {}, 0.0),           # 17 row blocks, the last one short
}
_twins = {}


def twin_of(name):
    """the case's twin, built once; big counts are put in here (build_twin's own share of them, 15 %, leaves too many rows
    whose totals are in the thousands, where the score gate cannot decide a group)"""
    if name not in _twins:
        specs, K, nchains, nheld, kw, big = CASES[name]
        twin = M.build_twin(specs, K, nchains, N_TRAIN, nheld, seed=sum(map(ord, name)), **kw)
        if big:
            rng = np.random.default_rng(99)
            for f in twin.held:
                if f["family"] in (orc.GP, orc.BNB):
                    pick = rng.random(nheld) < big
                    pick[0] = True
                    f["values"] = np.where(pick, rng.integers(1024, 1100, nheld), f["values"]).astype(np.uint32)
        _twins[name] = twin
    return _twins[name]


def weights_of(name):
    """uneven finite log weights with one chain left out (none with fewer than three chains)"""
    n = CASES[name][2]
    rng = np.random.default_rng(n)
    logw = rng.uniform(-3.0, 2.0, n)
    if n >= 3:
        logw[int(rng.integers(n))] = -np.inf
    return logw


def twin_totals(twin, c, rows):
    """t [len(rows), K] of chain c in double: the features' scores (masked entries nothing) plus the CRP term"""
    fs, counts, alpha = twin.chains[c]
    total = np.zeros((len(rows), twin.K))
    for i, (f, item) in enumerate(zip(twin.held, fs)):
        if item is None:
            continue
        F, ss64, _ = item
        total += np.where(twin.masks[i][rows][:, None], 0.0, F.score_matrix(ss64, f["values"][rows]))
    return total + crp_prior_matrix(counts, alpha)


# ---- the uniforms ------------------------------------------------------------------------------------------------------
def philox_np(key64, c0, c1, c2, c3):
    """Philox4x32-10 over arrays of counters (uint32 each) under one 64-bit key -> uint32 [n, 4]"""
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xffffffff)
    c = [np.asarray(x, dtype=np.uint64) & mask for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(key64 & 0xffffffff), np.uint64(key64 >> 32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def u53(a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64) + 0.5) / 9007199254740992.0


def pick_words(seed, row_ids, sweep):
    R = np.asarray(row_ids, dtype=np.uint64)
    return philox_np(int(seed) ^ PICK_KEY, R & np.uint64(0xffffffff), R >> np.uint64(32), int(sweep) & 0xffffffff, 0x80000000)


def uniforms(seed, row_ids, sweep):
    """(u1, u2) of the rows: the chain draw's and the group draw's"""
    w = pick_words(seed, row_ids, sweep)
    return u53(w[:, 0], w[:, 1]), u53(w[:, 2], w[:, 3])


# ---- the running-sum rule in float64 -----------------------------------------------------------------------------------
def running_pick(a, u):
    """a: [n_terms, n_rows] log terms, u [n_rows] -> (pick int [n_rows] with -1 for a row with no finite term or a NaN /
    +inf one, cum [n_terms, n_rows] the running sums of exp(a - max), S [n_rows])"""
    a = np.asarray(a, dtype=np.float64)
    bad = np.isnan(a).any(axis=0) | np.isposinf(a).any(axis=0) | ~np.isfinite(a).any(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(bad, 0.0, np.max(np.where(np.isnan(a), -np.inf, a), axis=0))
        e = np.where(np.isneginf(a) | bad[None, :], 0.0, np.exp(a - m[None, :]))
    cum = np.cumsum(e, axis=0)
    S = cum[-1]
    over = cum > (u * S)[None, :]
    first = np.argmax(over, axis=0)
    last = a.shape[0] - 1 - np.argmax((e > 0)[::-1], axis=0)
    pick = np.where(over.any(axis=0), first, last)
    return np.where(bad, -1, pick).astype(np.int32), cum, S


def chain_rule(lw, L, u1):
    """-> (chains [n_rows], undecided bool [n_rows]) from normalised log weights lw [nchains] and the chains' rows L
    [nchains, n_rows]"""
    with np.errstate(invalid="ignore"):
        a = np.asarray(lw, dtype=np.float64)[:, None] + np.asarray(L, dtype=np.float64)
    pick, cum, S = running_pick(a, u1)
    undecided = (np.abs((u1 * S)[None, :] - cum) <= 1e-12 * a.shape[0] * S[None, :]).any(axis=0) & (pick >= 0)
    return pick, undecided


def group_rule(t, u2):
    """-> (groups [n_rows], undecided bool [n_rows]) from the chosen chain's totals t [n_rows, K]"""
    t = np.asarray(t, dtype=np.float64)
    pick, cum, S = running_pick(t.T, u2)
    fin = np.where(np.isfinite(t), np.abs(t), 0.0)
    delta = 2.0 * 1e-6 * np.maximum(1.0, fin.max(axis=1)) + 1e-12
    with np.errstate(invalid="ignore", divide="ignore"):
        undecided = (np.abs(u2[None, :] - cum / S[None, :]) <= delta[None, :]).any(axis=0) & (pick >= 0)
    return pick, undecided
