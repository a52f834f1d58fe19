"""Yardsticks of the particle filter over rows (ChainEnsemble.smc, msc_chains_visit / msc_chains_clone): the same filter
over the double replay of the chain (seq_helpers.Replay), the exact evidence of a few rows, the derived gate of a visit's
log predictive, and the small fixtures the GPU tests share."""
import copy

import numpy as np
from scipy.special import logsumexp

from common_amd import smc as S
from oracle import oracle as orc
from tests import seq_helpers as sh
from tests.gpu_helpers import make_feature, recarray_of

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]


# ---- the six-row datasets ----------------------------------------------------------------------------------------------
def six_row_datasets():
    """one bb column; one nich column (the nich values of test_gpu_sequential.py's six-row tests) -> {name: [feature]}"""
    rng = np.random.default_rng(2024)
    bb = make_feature(orc.BB, 6, 2, rng)
    nich = make_feature(orc.NICH, 6, 2, rng)
    nich["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    return {"bb": [bb], "nich": [nich]}


def replay_features(feats, masks=None):
    """[(Family in double, values, mask)] of make_feature dicts, as seq_helpers.Replay takes them"""
    masks = masks or [None] * len(feats)
    return [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"], m) for f, m in zip(feats, masks)]


def exact_log_evidence(rfeats, alpha):
    """log p(X): logsumexp over every set partition of CRP score_assignment + the sum of score_data of its blocks -- the
    un-normalised numerators of seq_helpers.exact_posterior"""
    n = len(rfeats[0][1])
    logp = []
    for a in sh.set_partitions(n):
        za = np.asarray(a, dtype=np.int32)
        G = int(za.max()) + 1
        s = orc.score_assignment(za, alpha)
        for item in rfeats:
            F, values = item[0], item[1]
            s += float(F.score_data_all(F.accumulate(G, values, za)).sum())
        logp.append(s)
    return float(logsumexp(np.asarray(logp)))


# ---- a visit's log predictive on the replay ----------------------------------------------------------------------------
def replay_increment(rp, row):
    """(want, gate) of the log predictive of `row` against the replay's tables as they stand (the row not seated):
    want = logsumexp(scores) - log(n + alpha); the derived gate of tests/test_gpu_marginal.py, E + 1e-6 max(1, |want|)
    with E = 1e-6 max_k sum_f max(1, |score_f|)"""
    sc = rp.scores(row)
    want = float(logsumexp(sc) - np.log(rp.cnt.sum() + rp.alpha)) if np.isfinite(sc).any() else -np.inf
    mag = np.zeros(rp.K)
    for F, values, mask, ss in rp.feats:
        if not mask[row]:
            mag += np.maximum(1.0, np.abs(F.score_matrix(ss, values[row:row + 1])[0]))
    E = 1e-6 * float(mag.max()) if len(rp.feats) else 0.0
    return want, E + 1e-6 * max(1.0, abs(want))


def replay_pass(rp, order, got_z):
    """one pass of the replay over `order`, joining the device's draws got_z[row] -> (wants, gates) by position, and
    whether some visit found every slot occupied (the truncated branch)"""
    wants, gates, full = np.empty(len(order)), np.empty(len(order)), False
    for pos, row in enumerate(order):
        row, g = int(row), int(rp.z[int(row)])
        if 0 <= g < rp.K:
            rp._move(row, g, -1)
        full |= bool((rp.cnt > 0).all())
        wants[pos], gates[pos] = replay_increment(rp, row)
        rp._move(row, int(got_z[row]), +1)
        rp.z[row] = int(got_z[row])
    return wants, gates, full


def clone_replay(rp):
    """a replay with its own copy of everything a visit changes"""
    new = copy.copy(rp)
    new.z, new.cnt = rp.z.copy(), rp.cnt.copy()
    new.feats = [(F, values, mask, ss.copy()) for F, values, mask, ss in rp.feats]
    return new


# ---- the particle filter over the replay -------------------------------------------------------------------------------
def replay_smc(rfeats, K, alpha, P, rng, block=None, ess_threshold=0.5, order=None):
    """ChainEnsemble.smc on the replay: the same increments, checkpoints and systematic_ancestors, draws from `rng`
    -> dict(log_evidence, weights, ess, resampled_at, truncated)"""
    n = len(rfeats[0][1])
    order = np.arange(n) if order is None else np.asarray(order)
    block = max(1, n // 64) if block is None else block
    parts = [sh.Replay(rfeats, K, alpha, np.full(n, -1, np.int32)) for _ in range(P)]
    logw, log_z, ess, resampled_at = np.zeros(P), 0.0, [], []
    for pos0 in range(0, n, block):
        for pos in range(pos0, min(n, pos0 + block)):
            row = int(order[pos])
            for p, rp in enumerate(parts):
                logw[p] += replay_increment(rp, row)[0]
                rp.visit(row, rng.random())
        if min(n, pos0 + block) == n:
            break
        u = rng.random()
        ess.append(S.ess(logw))
        if ess[-1] < ess_threshold * P:
            log_z += S.log_mean_exp(logw)
            a = S.systematic_ancestors(logw, u)
            parts = [parts[c] if a[c] == c else clone_replay(parts[a[c]]) for c in range(P)]
            logw[:] = 0.0
            resampled_at.append(pos0 + block)
    ess.append(S.ess(logw))
    return dict(log_evidence=log_z + S.log_mean_exp(logw), weights=S.normalised_weights(logw), ess=ess,
                resampled_at=resampled_at, truncated=any((rp.cnt > 0).all() for rp in parts))


def evidence_se(weights):
    """the delta-method standard error of log_evidence from the final normalised weights: std(P w) / sqrt(P)"""
    P = len(weights)
    return float(np.std(np.asarray(weights) * P, ddof=1) / np.sqrt(P))


# ---- fixtures of the GPU tests -------------------------------------------------------------------------------------------
def data(gpu_ctx, specs, N, K, seed, mask_col=None):
    """seeded features, their masks (None: no entry masked) and their view; mask_col: a fifth of that column is masked"""
    import common_amd
    rng = np.random.default_rng(seed)
    feats = [make_feature(f, N, max(min(K, 6), 2), rng, d) for f, d in specs]
    rec, masks = recarray_of(feats), [None] * len(feats)
    if mask_col is not None:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in rec.dtype.names])
        mask["f%d" % mask_col] = rng.random(N) < 0.2
        masks[mask_col] = mask["f%d" % mask_col].copy()
        rec = np.ma.masked_array(rec, mask=mask)
    return feats, masks, common_amd.DataView.from_recarray(gpu_ctx, rec)


def ensemble(gpu_ctx, feats, K, nchains, alpha=1.0):
    import common_amd
    return common_amd.ChainEnsemble(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K, nchains, alpha=alpha,
                                    hps=[f["hp"] for f in feats])


def state_bits(st):
    """everything a sweep leaves in a state, as bytes: the group counts and every feature's suff-stats"""
    return [st.get_group_counts().tobytes()] + [st.get_ss(i).tobytes() for i in range(len(st.features))]


def ensemble_bits(ens):
    return ens.z.cpu().numpy().tobytes(), ens.logw.cpu().numpy().tobytes(), [state_bits(st) for st in ens.states]
