"""Yardsticks of the tempered ensemble's steps between sweeps (msc_chains_exchange, msc_chains_anneal_weights): the numpy
restatements of the likelihood sum, the exchange rule and the annealing weights the GPU tests compare against exactly; the
double replay of a chain at a temperature; the exact tempered posterior over the set partitions of a few rows, and a
replica-exchange sampler and an annealed importance sampler over that table which decide their swaps and weights through
those restatements -- the statistical check that the rule leaves every pi_beta invariant."""
import numpy as np

from oracle import oracle as orc
from tests import seq_helpers as sh

# the ladders of the six-row datasets (smc_helpers.six_row_datasets): rungs whose exact targets are >= 0.10 apart in
# total variation, so that a sampler which ignored beta could not meet the per-rung gate of 0.05
LADDERS = {"nich": (1.0, 2.0 / 3.0, 1.0 / 3.0, 0.0), "bb": (1.0, 0.0)}
MIN_RUNG_TV = 0.10
GATE_TV, GATE_KL = 0.05, 0.01


class TemperedReplay(sh.Replay):
    """seq_helpers.Replay at a temperature: a slot's score is log pseudocount + beta * (the features' sum); at beta = 0
    the CRP terms alone, whatever the features score (no 0 * -inf)"""

    def __init__(self, features, K, alpha, z, beta):
        sh.Replay.__init__(self, features, K, alpha, z)
        self.beta = float(beta)

    def scores(self, row):
        feats, self.feats = self.feats, []
        try:
            crp = sh.Replay.scores(self, row)                # (no feature: the CRP terms)
        finally:
            self.feats = feats
        if self.beta == 0.0:
            return crp
        fsum = np.zeros(self.K)
        for F, values, mask, ss in self.feats:
            if not mask[row]:
                fsum += F.score_matrix(ss, values[row:row + 1])[0]
        return crp + self.beta * fsum


def chain_loglik(joint_row, nfeat):
    """((d_0 + d_1) + ...) + d_{F-1} of a joint row in double, in that order (0 with no feature)"""
    l = np.float64(0.0)
    for f in range(nfeat):
        l = np.float64(joint_row[2 + f]) if f == 0 else l + np.float64(joint_row[2 + f])
    return l


def exchange_np(joint, nfeat, R, beta, rung, parity, seed, sweep, proposed, accepted):
    """msc_chains_exchange on host arrays -> (beta, rung, proposed, accepted, bad): new arrays, and the ladders whose
    rungs were no permutation, which are left as they were"""
    beta, rung = np.array(beta, dtype=np.float32), np.array(rung, dtype=np.int32)
    proposed, accepted = np.array(proposed).copy(), np.array(accepted).copy()
    bad = []
    with np.errstate(all="ignore"):
        for l in range(len(beta) // R):
            c0 = l * R
            if sorted(rung[c0:c0 + R].tolist()) != list(range(R)):
                bad.append(l)
                continue
            for j in range(R - 1):
                if j % 2 != parity % 2:
                    continue
                a = c0 + int(np.flatnonzero(rung[c0:c0 + R] == j)[0])
                b = c0 + int(np.flatnonzero(rung[c0:c0 + R] == j + 1)[0])
                la, lb = chain_loglik(joint[a], nfeat), chain_loglik(joint[b], nfeat)
                r = (np.float64(beta[a]) - np.float64(beta[b])) * (lb - la)
                proposed[l, j] += 1
                u = np.float64(orc.uniform01(seed, sweep, c0 + j))
                # (numpy's log of a double and the device's may differ by an ulp, which shows only where log u falls
                # within an ulp of r: a GPU test that compares with this byte for byte and fails at ONE pair after a
                # change of seeds or rows has met such a tie, not a kernel bug -- look at log u - r there first)
                if not (np.isfinite(r) and np.log(u) < r):
                    continue
                accepted[l, j] += 1
                beta[a], beta[b] = beta[b], beta[a]
                rung[a], rung[b] = j + 1, j
    return beta, rung, proposed, accepted, bad


def anneal_np(joint, nfeat, beta_from, beta_to, logw):
    """msc_chains_anneal_weights on host arrays -> the new log weights: an entry whose temperatures are equal is left as
    it was, whatever its likelihood"""
    out = np.array(logw, dtype=np.float64)
    with np.errstate(all="ignore"):
        for c, (f, t) in enumerate(zip(np.asarray(beta_from, dtype=np.float32), np.asarray(beta_to, dtype=np.float32))):
            if t != f:
                out[c] = out[c] + (np.float64(t) - np.float64(f)) * chain_loglik(joint[c], nfeat)
    return out



# ---- the exact tempered posterior of a few rows ----------------------------------------------------------------------------
class PartitionTable(object):
    """Every set partition of the rows with its log prior (CRP score_assignment) and its data log-likelihood (the sum of
    score_data of its blocks) from the f64 oracle -- the numerators of seq_helpers.exact_posterior kept apart -- and, per
    partition and row, the partitions a Gibbs visit of that row can move to."""

    def __init__(self, rfeats, alpha):
        self.n = len(rfeats[0][1])
        self.parts = sh.set_partitions(self.n)
        self.index = {a: i for i, a in enumerate(self.parts)}
        self.log_prior, self.log_lik = np.empty(len(self.parts)), np.empty(len(self.parts))
        for i, a in enumerate(self.parts):
            za = np.asarray(a, dtype=np.int32)
            G = int(za.max()) + 1
            self.log_prior[i] = orc.score_assignment(za, alpha)
            self.log_lik[i] = sum(float(item[0].score_data_all(item[0].accumulate(G, item[1], za)).sum()) for item in rfeats)
        # moves[p, i, :]: the distinct partitions reached by giving row i any block of the others, or one of its own
        # (-1: no such candidate); the partition itself is among them
        self.moves = np.full((len(self.parts), self.n, self.n + 1), -1, dtype=np.int64)
        for p, a in enumerate(self.parts):
            for i in range(self.n):
                rest = [g for r, g in enumerate(a) if r != i]
                cands = sorted({self.index[sh.canonical(a[:i] + (g,) + a[i + 1:])] for g in set(rest) | {max(a) + 1}})
                self.moves[p, i, :len(cands)] = cands

    def posterior(self, beta):
        """pi_beta: exp(log prior + beta * log likelihood), normalised"""
        lp = self.log_prior + float(beta) * self.log_lik
        p = np.exp(lp - lp.max())
        return p / p.sum()

    def prior_draws(self, nchains, rng):
        return rng.choice(len(self.parts), size=nchains, p=self.posterior(0.0))

    def gibbs_sweep(self, state, beta, rng):
        """one sweep of single-row Gibbs visits at temperature beta[c] on every chain (state: partition indices)"""
        logpi = self.log_prior[None, :] + np.asarray(beta, dtype=np.float64)[:, None] * self.log_lik[None, :]
        who = np.arange(len(state))
        for i in range(self.n):
            cand = self.moves[state, i]                                   # [nchains, n + 1]
            w = np.where(cand >= 0, logpi[who[:, None], np.maximum(cand, 0)], -np.inf)
            w = np.exp(w - w.max(1, keepdims=True))
            cdf = np.cumsum(w, 1)
            pick = (cdf < (rng.random(len(state)) * cdf[:, -1])[:, None]).sum(1)
            state = cand[who, np.minimum(pick, (cand >= 0).sum(1) - 1)]
        return state


def rung_separation(table, betas):
    """the smallest exact total variation between the targets of two rungs"""
    ps = [table.posterior(b) for b in betas]
    return min(0.5 * float(np.abs(ps[i] - ps[j]).sum()) for i in range(len(ps)) for j in range(i))



def replica_exchange_np(table, betas, nladders, burn, niters, rng, seed=12345):
    """A replica-exchange sampler over the table as a tempered ensemble runs it: chain l R + j starts on rung j; per
    iteration one Gibbs sweep of every chain at the temperature it holds, then exchange_np with the iteration's parity
    on joint rows that carry the chains' log-likelihoods -- the TEMPERATURES move, as on the device.  Samples are taken
    after the sweep, before the exchange, and counted under the rung the chain held then
    -> (frequencies [R, npartitions] after the burn-in, accepted / proposed per pair, whether every chain held every rung)"""
    R = len(betas)
    nc = nladders * R
    betas32 = np.asarray(betas, dtype=np.float32)
    state = table.prior_draws(nc, rng)
    beta, rung = np.tile(betas32, nladders), np.tile(np.arange(R, dtype=np.int32), nladders)
    prop = acc = np.zeros((nladders, R - 1), dtype=np.int64)
    cnt = np.zeros((R, len(table.parts)))
    held = np.zeros((nc, R), dtype=bool)
    joint = np.zeros((nc, 4))                                             # F = 1: (total, a, d_0, p)
    for it in range(burn + niters):
        state = table.gibbs_sweep(state, beta, rng)
        held[np.arange(nc), rung] = True
        if it >= burn:
            np.add.at(cnt, (rung, state), 1)
        joint[:, 2] = table.log_lik[state]
        beta, rung, prop, acc, bad = exchange_np(joint, 1, R, beta, rung, it, seed, it, prop, acc)
        assert not bad and np.array_equal(beta, betas32[rung])
    return cnt / cnt.sum(1, keepdims=True), acc.sum(0) / np.maximum(prop.sum(0), 1), bool(held.all())


def ais_np(table, betas, nchains, rng, sweeps_per_temp=1):
    """annealed importance sampling over the table: a prior draw, then per temperature anneal_np's weight step on the
    chains' log-likelihoods and the Gibbs sweeps at the new temperature -> log weights [nchains]"""
    betas32 = np.asarray(betas, dtype=np.float32)
    state = table.prior_draws(nchains, rng)
    logw, joint = np.zeros(nchains), np.zeros((nchains, 4))
    for t in range(1, len(betas32)):
        joint[:, 2] = table.log_lik[state]
        logw = anneal_np(joint, 1, np.full(nchains, betas32[t - 1]), np.full(nchains, betas32[t]), logw)
        for _ in range(sweeps_per_temp):
            state = table.gibbs_sweep(state, np.full(nchains, betas32[t], dtype=np.float64), rng)
    return logw
