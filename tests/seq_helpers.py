"""Yardsticks of the sequential Gibbs sweep (msc_sweep_sequential): a double-precision replay of the chain on the oracle,
and the exact posterior over the set partitions of a few rows."""
import math

import numpy as np

from oracle import oracle as orc


class Replay(object):
    """The sequential collapsed Gibbs chain in double on the oracle's Family add / remove / score_value.

    features: list of (Family, values[, mask]) -- a masked entry takes no part in the sums or the score.  z: int32 group
    of every row (outside [0, K) = unassigned); the suff-stats start as the oracle's accumulate of z."""

    def __init__(self, features, K, alpha, z):
        self.K, self.alpha = K, float(alpha)
        self.z = np.array(z, dtype=np.int32, copy=True)
        self.feats = []
        zin = np.where((self.z >= 0) & (self.z < K), self.z, -1).astype(np.int32)
        for item in features:
            F, values = item[0], item[1]
            mask = item[2] if len(item) > 2 and item[2] is not None else np.zeros(len(values), dtype=bool)
            ss = F.accumulate(K, values, np.where(mask, -1, zin).astype(np.int32))
            self.feats.append((F, values, np.asarray(mask, dtype=bool), ss))
        self.cnt = np.bincount(zin[zin >= 0], minlength=K).astype(np.int64)

    def _move(self, row, g, sign):
        for F, values, mask, ss in self.feats:
            if not mask[row]:
                (F.add_value if sign > 0 else F.remove_value)(ss, g, values[row:row + 1])
        self.cnt[g] += sign

    def scores(self, row):
        """log pseudocount + sum of score_value of the row against every slot as the tables now stand"""
        nempty = int((self.cnt == 0).sum())
        empty = math.log(orc.pseudocount(0, self.alpha, nempty)) if nempty else -np.inf    # (alpha / nempty)
        sc = np.where(self.cnt > 0, np.log(np.maximum(self.cnt, 1).astype(np.float64)), empty)   # (pseudocount(c) = c)
        for F, values, mask, ss in self.feats:
            if not mask[row]:
                sc += F.score_matrix(ss, values[row:row + 1])[0]
        return sc

    def visit(self, row, u, got=None, tol=1e-5):
        """One visit of `row` with the uniform u: leave, score, draw.  got = None: join the replay's own draw; else check
        that `got` is the draw, or that u lies within `tol` of the CDF step between the two, and join `got`.
        -> (the group joined, whether it disagreed with the replay's own draw)"""
        g = int(self.z[row])
        if 0 <= g < self.K:
            self._move(row, g, -1)
        p = orc.scores_to_probs(self.scores(row))
        want = int(orc.sample_discrete(p, u))
        off = False
        if got is not None and int(got) != want:
            cdf = np.cumsum(p)
            lo, hi = sorted((int(got), want))
            assert abs(cdf[lo] - u) < tol or p[lo + 1:hi + 1].sum() < tol, (row, got, want, cdf[lo], u)
            off = True
        j = want if got is None else int(got)
        self._move(row, j, +1)
        self.z[row] = j
        return j, off

    def sweep(self, rows, seed, sweep, row_ids, got=None):
        """visit rows[i] with uniform01(seed, sweep, row_ids[i]); got: the device's draw of each visit (or None)"""
        n_off = 0
        for i, r in enumerate(rows):
            _, off = self.visit(int(r), orc.uniform01(seed, sweep, int(row_ids[i])), None if got is None else got[i])
            n_off += off
        return n_off

    def tables(self):
        return [ss for _, _, _, ss in self.feats], self.cnt.copy()


def set_partitions(n):
    """every set partition of n items as a restricted growth string (Bell(n) of them)"""
    out = []

    def rec(a, m):
        if len(a) == n:
            out.append(tuple(a))
            return
        for g in range(m + 1):
            rec(a + [g], max(m, g + 1))

    rec([0], 1) if n > 0 else out.append(())
    return out


def canonical(z):
    """the set partition a labelled assignment induces, as its restricted growth string"""
    seen, out = {}, []
    for g in z:
        out.append(seen.setdefault(int(g), len(seen)))
    return tuple(out)


def exact_posterior(features, alpha):
    """features: list of (Family, values).  -> (partitions, probabilities): CRP score_assignment + the sum of score_data
    of every block, from the f64 oracle, normalised"""
    n = len(features[0][1])
    parts = set_partitions(n)
    logp = np.empty(len(parts))
    for i, a in enumerate(parts):
        za = np.asarray(a, dtype=np.int32)
        G = int(za.max()) + 1
        s = orc.score_assignment(za, alpha)
        for F, values in features:
            s += float(F.score_data_all(F.accumulate(G, values, za)).sum())
        logp[i] = s
    p = np.exp(logp - logp.max())
    return parts, p / p.sum()


def partition_frequencies(traces, parts):
    """fraction of the sweeps (rows of traces: z after a sweep) that visited each partition"""
    index = {a: i for i, a in enumerate(parts)}
    cnt = np.zeros(len(parts))
    for z in np.asarray(traces):
        cnt[index[canonical(z)]] += 1
    return cnt / cnt.sum()


def tv_kl(freq, p):
    """total variation and KL(empirical || exact)"""
    tv = 0.5 * float(np.abs(freq - p).sum())
    nz = freq > 0
    kl = float((freq[nz] * np.log(freq[nz] / p[nz])).sum())
    return tv, kl
