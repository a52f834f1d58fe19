"""Yardsticks of the split-merge move (msc_split_merge): the streams of common_amd/csrc/splitmerge_math.hpp restated on
the oracle's Philox, the f64 acceptance ratio from the oracle's score_assignment / score_data, and a float64 numpy
restatement of the whole move -- a yardstick for the exact-posterior and the "does what it is for"
tests, not code under test.  `python -m tests.sm_helpers` prints the yardstick's own figures on the tests' data."""
import math

import numpy as np

from oracle import oracle as orc

KEY = 0xA0761D6478BD642F
STRIDE = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
STREAM_PROPOSAL, STREAM_COIN, STREAM_PASS0 = 0, 1, 2
SPLIT, MERGE, VOID = 0, 1, 2
DART_ACCEPT = 4


def stream_key(seed, stream):
    return ((int(seed) ^ KEY) + stream * STRIDE) & M64


def pick_index(hi, lo, n):
    u = float(hi) + float(lo) / 16777216.0
    return min(int(u * n), n - 1)


def anchors(seed, sweep, n):
    """the ordered pair of distinct offsets the device draws for (seed, sweep) over n rows"""
    key = stream_key(seed, STREAM_PROPOSAL)
    i = pick_index(orc.uniform01(key, sweep, 0), orc.uniform01(key, sweep, 1), n)
    t = pick_index(orc.uniform01(key, sweep, 2), orc.uniform01(key, sweep, 3), n - 1)
    return i, (t + 1 if t >= i else t)


def accept_dart(seed, sweep):
    return float(orc.uniform01(stream_key(seed, STREAM_PROPOSAL), sweep, DART_ACCEPT))


def coin(seed, sweep, row_id):
    return 1 if orc.uniform01(stream_key(seed, STREAM_COIN), sweep, int(row_id)) >= 0.5 else 0


def label_dart(seed, sweep, t, row_id):
    return float(orc.uniform01(stream_key(seed, STREAM_PASS0 + t), sweep, int(row_id)))


def block_score(features, rows, float_state=False):
    """sum over features of score_data of the block `rows` (f64 oracle); features: (Family, values[, mask]).
    float_state: the block's suff-stats are accumulated in double and their float fields rounded to float before they
    are scored -- the state the device keeps (tests/gpu_helpers.state_from_assignment does the same for its twin)"""
    s, terms = 0.0, []
    for item in features:
        F, values = item[0], item[1]
        mask = item[2] if len(item) > 2 and item[2] is not None else np.zeros(len(values), dtype=bool)
        z = np.full(len(values), -1, dtype=np.int32)
        z[rows] = 0
        z[mask] = -1
        ss = F.accumulate(1, values, z)
        if float_state:
            ss = orc.widen_ss(F.family, orc.narrow_ss(F.family, ss, F.dim), F.dim)
        v = float(F.score_data_all(ss)[0])
        s += v
        terms.append(v)
    return s, terms


def log_accept(features, alpha, rows0, rows1, kind, logq, float_state=False):
    """-> (log A, the magnitude sum of its terms for the audit gate): the CRP term is the difference of the oracle's
    score_assignment of the divided and the undivided block"""
    n0, n1 = len(rows0), len(rows1)
    za = np.concatenate([np.zeros(n0), np.ones(n1)]).astype(np.int32)
    crp = orc.score_assignment(za, alpha) - orc.score_assignment(np.zeros(n0 + n1, dtype=np.int32), alpha)
    sd0, t0 = block_score(features, np.asarray(rows0), float_state)
    sd1, t1 = block_score(features, np.asarray(rows1), float_state)
    sdS, tS = block_score(features, np.concatenate([rows0, rows1]), float_state)
    t = crp + sd0 + sd1 - sdS
    mag = sum(max(1.0, abs(x)) for x in [crp, logq] + t0 + t1 + tS)
    return (t - logq if kind == SPLIT else -t + logq), mag


def two_way(s):
    """[n, 2] scores -> [n, 2] log-probabilities, float64"""
    m = s.max(axis=1, keepdims=True)
    return s - m - np.log(np.exp(s - m).sum(axis=1, keepdims=True))


class Yardstick(object):
    """The move of include/microscopes_hip.h (msc_split_merge) in float64 numpy with numpy's generator: bb and nich
    columns, no masks.  feats: the dicts of tests/gpu_helpers.make_feature."""

    def __init__(self, feats, alpha, K, seed, masks=None):
        self.alpha, self.K = float(alpha), K
        self.rng = np.random.default_rng(seed)
        self.feats = feats
        self.n = len(feats[0]["values"])
        self.masks = [np.zeros(self.n, dtype=bool) if m is None else np.asarray(m, dtype=bool)
                      for m in (masks or [None] * len(feats))]
        self.F = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"], m) for f, m in zip(feats, self.masks)]
        self.counts = [0, 0, 0, 0, 0]
        self._sd = {}

    def sd(self, rows):
        key = tuple(rows) if len(rows) <= 16 else None
        if key is not None and key in self._sd:
            return self._sd[key]
        v = block_score(self.F, np.asarray(rows))[0]
        if key is not None:
            self._sd[key] = v
        return v

    def _theta(self, lab, S):
        rng, out = self.rng, []
        n0, n1 = int((lab == 0).sum()), int((lab == 1).sum())
        v = rng.beta(1.0 + n0, self.alpha + n1)
        lw = np.log([v, 1.0 - v])
        for f, m in zip(self.feats, self.masks):
            x = f["values"][S].astype(np.float64)
            seen = ~m[S]
            hp, par = f["hp"], []
            for s in (0, 1):
                xs = x[(lab == s) & seen]
                n = len(xs)
                if f["family"] == orc.BB:
                    par.append(rng.beta(hp["alpha"] + xs.sum(), hp["beta"] + n - xs.sum()))
                elif f["family"] == orc.GP:
                    par.append(rng.gamma(hp["alpha"] + xs.sum()) / (hp["inv_beta"] + n))
                elif f["family"] == orc.BNB:
                    par.append(rng.beta(hp["alpha"] + hp["r"] * n, hp["beta"] + xs.sum()))
                elif f["family"] == orc.DD:
                    a = np.asarray(hp["alphas"], dtype=np.float64) + np.bincount(xs.astype(int), minlength=f["dim"])
                    par.append(rng.dirichlet(a))
                elif f["family"] == orc.NICH:
                    mu, kappa, sigmasq, nu = (hp[k] for k in ("mu", "kappa", "sigmasq", "nu"))
                    mean = xs.mean() if n else 0.0
                    ctv = ((xs - mean) ** 2).sum() if n else 0.0
                    kn, nun = kappa + n, nu + n
                    mun = (kappa * mu + n * mean) / kn
                    sn = (nu * sigmasq + ctv + n * kappa * (mu - mean) ** 2 / kn) / nun
                    sig2 = nun * sn / rng.chisquare(nun)
                    par.append((mun + math.sqrt(sig2 / kn) * rng.normal(), sig2))
                else:
                    raise ValueError("the yardstick draws bb, gp, bnb, dd and nich columns")
            out.append(par)
        return lw, out

    def _logp(self, lw, theta, S):
        s = np.repeat(lw[None, :], len(S), axis=0)
        tiny = 1e-300
        for f, m, par in zip(self.feats, self.masks, theta):
            x = f["values"][S].astype(np.float64)
            seen = ~m[S]
            for k in (0, 1):
                if f["family"] == orc.BB:
                    t = np.where(x > 0, np.log(par[k] + tiny), np.log(1.0 - par[k] + tiny))
                elif f["family"] == orc.GP:
                    t = x * np.log(par[k] + tiny) - par[k]
                elif f["family"] == orc.BNB:
                    t = f["hp"]["r"] * np.log(par[k] + tiny) + x * np.log(1.0 - par[k] + tiny)
                elif f["family"] == orc.DD:
                    t = np.log(par[k] + tiny)[x.astype(int)]
                else:
                    mean, sig2 = par[k]
                    t = -0.5 * np.log(2 * np.pi * sig2) - 0.5 * (x - mean) ** 2 / sig2
                s[:, k] += np.where(seen, t, 0.0)
        return two_way(s)

    def propose(self, z, launch_iters, pair=None):
        """one proposal on z (int array, changed in place) -> (kind, accepted); pair: the anchors (None: drawn)"""
        rng, n = self.rng, self.n
        if pair is None:
            i = int(rng.integers(n))
            j = int(rng.integers(n - 1))
            j += j >= i
        else:
            i, j = pair
        gi, gj = int(z[i]), int(z[j])
        if not (0 <= gi < self.K and 0 <= gj < self.K):
            self.counts[4] += 1
            return VOID, False
        kind = SPLIT if gi == gj else MERGE
        empty = [k for k in range(self.K) if not (z == k).any()]
        if kind == SPLIT and not empty:
            self.counts[4] += 1
            return VOID, False
        S = np.nonzero((z == gi) | (z == gj))[0]
        free = (S != i) & (S != j)
        lab = (rng.random(len(S)) >= 0.5).astype(int)
        lab[S == i], lab[S == j] = 0, 1
        for _ in range(launch_iters):
            l = self._logp(*self._theta(lab, S), S)
            lab = np.where(free, (rng.random(len(S)) >= np.exp(l[:, 0])).astype(int), lab)
        l = self._logp(*self._theta(lab, S), S)
        if kind == SPLIT:
            fin = np.where(free, (rng.random(len(S)) >= np.exp(l[:, 0])).astype(int), lab)
        else:
            fin = (z[S] == gj).astype(int)
        logq = float(l[np.arange(len(S)), fin][free].sum())
        A, B = S[fin == 0], S[fin == 1]
        t = math.log(self.alpha) + math.lgamma(len(A)) + math.lgamma(len(B)) - math.lgamma(len(S)) + self.sd(A) + \
            self.sd(B) - self.sd(S)
        logA = t - logq if kind == SPLIT else -t + logq
        ok = math.log(rng.random()) < logA
        self.counts[2 * kind] += 1
        self.counts[2 * kind + 1] += ok
        if ok:
            z[B] = empty[0] if kind == SPLIT else gi
        return kind, ok


# ---- the data of the tests that the yardstick vouches for -------------------------------------------------------------
def six_row_datasets():
    """the two data sets of tests/test_gpu_blocked.py::test_exact_posterior_of_six_rows, restated"""
    from tests.gpu_helpers import make_feature
    rng = np.random.default_rng(2024)
    N = 6
    d = {
        "bb3": [make_feature(orc.BB, N, 2, rng) for _ in range(3)],
        "nich_bb": [make_feature(orc.NICH, N, 2, rng), make_feature(orc.BB, N, 2, rng)],
    }
    d["nich_bb"][0]["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    return d


def two_cluster_data(N=1500, seed=5):
    """two nich clusters at -10 / +10 (sd 1) and a bb column with p = 0.1 / 0.9 -> (features, truth).  The nich prior
    says what the data are: a variance of 1, held firmly (nu = 1e4).  Under the vague prior (nu = 1) the two pair slots of a
    coin-flip start both fit N(0, 101); a row then prefers neither, three launch passes leave the labels at random, and
    what is accepted are partial cuts (the yardstick: the two largest groups hold 0.51 - 0.79 of the rows after 20
    proposals on five seeds).  With the variance known a slot's mean a little above the other's draws every row of the
    upper cluster in one pass."""
    rng = np.random.default_rng(seed)
    truth = (rng.random(N) < 0.5).astype(np.int32)
    x = (np.where(truth == 1, 10.0, -10.0) + rng.normal(0, 1, N)).astype(np.float32)
    b = rng.random(N) < np.where(truth == 1, 0.9, 0.1)
    feats = [dict(family=orc.NICH, dim=0, hp=dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=1e4), values=x, np_dtype=np.float32),
             dict(family=orc.BB, dim=0, hp=dict(alpha=1.0, beta=1.0), values=b.astype(np.bool_), np_dtype=np.bool_)]
    return feats, truth


def clustered_case(specs, N, seed, masked=False, gp_large=False, npair=3, first=150, dd_alpha=0.002, dd_w=1):
    """N rows from four separated clusters for the features `specs` = [(family, dim)] (hyper-parameters and dtypes from
    make_feature -- nich with a weak prior on the mean and wide dd columns with small alphas, so that small groups may
    form --, the values set here), and the
    start z0 of the records tests: group 0 holds npair rows each of clusters 0 and 1 (rows from `first` on), the rest of
    those clusters are groups 4 and 5, cluster 2 is spread over groups 1 and 2, cluster 3 is group 3, a few rows are
    unassigned.  The clusters and z0 depend on (N, npair, first) alone, not on the seed or the features.  A dd column of
    two values tells only even clusters from odd ones.  -> (feats, masks, truth, z0)"""
    from tests.gpu_helpers import make_feature
    lay = np.random.default_rng(1000 + N)
    truth = lay.integers(0, 4, N)
    z0 = np.array([4, 5, 1, 3])[truth].astype(np.int32)
    z0[(truth == 2) & (np.arange(N) % 2 == 1)] = 2
    for c in (0, 1):
        idx = np.nonzero(truth == c)[0]
        z0[idx[idx >= first][:npair]] = 0
    free = np.nonzero(z0 != 0)[0]
    z0[lay.choice(free, max(3, N // 60), replace=False)] = -1
    rng = np.random.default_rng(seed)
    bits = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]])
    feats, nbb = [], 0
    for family, dim in specs:
        hp = None
        if family == orc.NICH:
            hp = dict(mu=0.0, kappa=0.01, sigmasq=1.0, nu=2.0)
        elif family == orc.DD and dim >= 4:
            hp = dict(alphas=[dd_alpha] * dim)
        f = make_feature(family, N, 4, rng, dim, hp=hp)
        if family == orc.BB:
            p = np.where(bits[truth, nbb % 3] == 1, 0.99, 0.01)
            f["values"] = (rng.random(N) < p).astype(np.bool_)
            nbb += 1
        elif family == orc.GP:
            lam = np.array([5.0, 60.0, 1500.0, 3000.0] if gp_large else [1.0, 12.0, 40.0, 100.0])
            f["values"] = rng.poisson(lam[truth]).astype(np.uint32)
        elif family == orc.BNB:
            pr = np.array([0.9, 0.3, 0.08, 0.02])
            f["values"] = rng.negative_binomial(int(f["hp"]["r"]), pr[truth]).astype(np.uint32)
        elif family == orc.DD:
            if dim < 4:
                v = truth % dim
                v = np.where(rng.random(N) < 0.03, rng.integers(0, dim, N), v)
            else:
                w = min(dim // 4, dd_w)
                v = truth * (dim // 4) + rng.integers(0, w, N)
            f["values"] = v.astype(np.int32)
        elif family == orc.NICH:
            f["values"] = (np.array([-15.0, -5.0, 5.0, 15.0])[truth] + rng.normal(0, 1, N)).astype(np.float32)
        feats.append(f)
    masks = [rng.random(N) < 0.2 if masked else None for _ in feats]
    return feats, masks, truth, z0


CATEGORIES = ("split_pair", "split_pure", "merge_same", "merge_cross", "void")
_PLANS = {}


def category(zi, zj):
    """what a proposal with anchors in groups zi, zj of clustered_case's z0 is"""
    if zi < 0 or zj < 0:
        return "void"
    if zi == zj:
        return "split_pair" if zi == 0 else "split_pure"
    if zi == 0 or zj == 0:
        return None
    return "merge_same" if {zi, zj} == {1, 2} else "merge_cross"


def plan_sweeps(z, seed, counts, truth=None):
    """sweep counters, ascending, whose anchors over the rows of z (the call's range) fall into the categories of
    clustered_case's layout `counts` times each (the order of CATEGORIES): the anchors are a function of
    (seed, sweep, len(z)) alone, so the choice of counters is a choice of proposals.  With `truth` (the rows' clusters)
    a split of group 0 counts only when its anchors lie in different clusters: the others cannot cut it cleanly."""
    key = (z.tobytes(), seed, tuple(counts), None if truth is None else truth.tobytes())
    if key in _PLANS:
        return _PLANS[key]
    n, pk = len(z), stream_key(seed, STREAM_PROPOSAL)
    left = dict(zip(CATEGORIES, counts))
    out, sweep = [], 0
    while any(left.values()):
        i = pick_index(orc.uniform01(pk, sweep, 0), orc.uniform01(pk, sweep, 1), n)
        zi = int(z[i])
        # (an anchor in one of the large groups is needed only while a category that can hold it is open)
        if zi == 0 or zi < 0 or left["split_pure"] or left["merge_same"] or left["merge_cross"]:
            j = anchors(seed, sweep, n)[1]
            c = category(zi, int(z[j]))
            if c == "split_pair" and truth is not None and truth[i] == truth[j]:
                c = None
            if c is not None and left[c]:
                left[c] -= 1
                out.append(sweep)
        sweep += 1
        assert sweep < 3000000
    _PLANS[key] = out
    return out


def two_largest_agree(z, truth):
    """-> (share of the rows in the two largest groups, share of all rows on which those two groups agree with the truth
    under the better of the two matchings)"""
    ids, cnt = np.unique(z[z >= 0], return_counts=True)
    top = ids[np.argsort(-cnt)][:2]
    if len(top) < 2:
        return float(cnt.max()) / len(z), 0.0
    share = float(((z == top[0]) | (z == top[1])).sum()) / len(z)
    a = ((z == top[0]) & (truth == 0)).sum() + ((z == top[1]) & (truth == 1)).sum()
    b = ((z == top[0]) & (truth == 1)).sum() + ((z == top[1]) & (truth == 0)).sum()
    return share, float(max(a, b)) / len(z)


def _main():
    from tests import seq_helpers as sh
    nprop = 50000
    for name, feats in six_row_datasets().items():
        Fs = [(orc.Family(f["family"], f["hp"], f["dim"], "f64"), f["values"]) for f in feats]
        parts, p = sh.exact_posterior(Fs, 1.0)
        for seed in range(5):
            y = Yardstick(feats, 1.0, 32, seed)
            z = np.zeros(6, dtype=np.int64)
            trace = np.empty((nprop, 6), dtype=np.int64)
            for t in range(nprop):
                y.propose(z, 0)
                trace[t] = z
            tv, kl = sh.tv_kl(sh.partition_frequencies(trace, parts), p)
            print("yardstick %s seed %d: TV %.4f KL %.5f counts %s" % (name, seed, tv, kl, y.counts))
    feats, truth = two_cluster_data()
    for seed in range(5):
        y = Yardstick(feats, 1.0, 8, seed)
        z = np.zeros(len(truth), dtype=np.int64)
        for _ in range(20):
            y.propose(z, 3)
        share, agree = two_largest_agree(z, truth)
        z = (2 * truth + (np.arange(len(truth)) % 2)).astype(np.int64)
        for _ in range(40):
            y.propose(z, 3)
        print("yardstick two clusters seed %d: share %.4f agree %.4f, groups after merges %d" %
              (seed, share, agree, len(np.unique(z))))


if __name__ == "__main__":
    _main()
