"""Yardsticks of the ensemble's posterior-averaged row predictive density (ChainEnsemble.predictive_logp,
msc_chains_score_marginal): an ensemble whose chains each hold their own assignment, hyper-parameters and alpha, its
double twin, and the derived gates.

Gates (derived, not measured).  Every total t_c[r][k] is within E_{r,c} = 1e-6 max_k sum_f max(1, |score_f|) of the twin
by the project's standing gates (the prior term is exact), and a log-sum-exp moves by no more than
the largest change of an entry, so chain c's row is held to gate_c[r] = E_{r,c} + 1e-6 max(1, |want_c[r]|), the gate of
tests/test_gpu_marginal.py.  mix is a weighted log-sum-exp of those rows (the weights are normalised in double: exact at
this scale), so it moves by no more than the largest gate_c of a chain that takes part, plus the plain gate for its own
reduction and rounding: max_c gate_c[r] + 1e-6 max(1, |want_mix[r]|)."""
import numpy as np
from scipy.special import logsumexp

from oracle import oracle as orc
from tests.gpu_helpers import crp_prior_matrix, distinct_hp, make_feature, recarray_of, state_from_assignment

NOOP = 5          # common_amd.NOOP: a column the model ignores (make_feature has no such family)


def _feature(fam, n, k, rng, dim):
    if fam == NOOP:
        return dict(family=NOOP, dim=0, hp=None, values=rng.random(n) < 0.5, np_dtype=np.bool_)
    return make_feature(fam, n, k, rng, dim)


def normalised(logw, nchains):
    """lw_c = logw_c - logsumexp(logw) in float64; None: equal weights"""
    if logw is None:
        return np.full(nchains, -np.log(nchains))
    logw = np.asarray(logw, dtype=np.float64)
    return logw - logsumexp(logw)


class EnsembleTwin(object):
    """The double side alone: chains[c] = (feature states [(Family64, ss64, ss32) or None for noop], counts, alpha)."""

    def __init__(self, specs, K, chains, held, masks):
        self.specs, self.K, self.chains, self.held, self.masks = specs, K, chains, held, masks
        self.nchains = len(chains)

    def chain(self, c, rows, feats=None):
        """-> (want [n], gate [n]) of chain c for the held-out rows, over the features `feats` (None: all)"""
        fs, counts, alpha = self.chains[c]
        total, mag = np.zeros((len(rows), self.K)), np.zeros((len(rows), self.K))
        for i, (f, item) in enumerate(zip(self.held, fs)):
            if item is None or (feats is not None and i not in feats):
                continue
            F, ss64, _ = item
            m = F.score_matrix(ss64, f["values"][rows])
            dead = self.masks[i][rows][:, None]
            total += np.where(dead, 0.0, m)
            mag += np.where(dead, 0.0, np.maximum(1.0, np.abs(m)))
        t = total + crp_prior_matrix(counts, alpha)
        want = logsumexp(t, axis=1) - np.log(float(counts.sum()) + alpha)
        return want, 1e-6 * mag.max(axis=1) + 1e-6 * np.maximum(1.0, np.abs(want))

    def all_chains(self, rows, feats=None):
        """-> (want [nchains, n], gate [nchains, n])"""
        pairs = [self.chain(c, rows, feats) for c in range(self.nchains)]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])

    @staticmethod
    def mix(want, gate, logw=None):
        """-> (want_mix [n], gate_mix [n]) from the chains' rows under log weights logw (None: equal)"""
        lw = normalised(logw, want.shape[0])
        live = np.isfinite(lw)
        wm = logsumexp(want[live] + lw[live, None], axis=0)
        return wm, gate[live].max(axis=0) + 1e-6 * np.maximum(1.0, np.abs(wm))


def build_twin(specs, K, nchains, ntrain, nheld, seed, used=None, masked=(), big_counts=False, assignments=None,
               alphas=None, hp_of=None):
    """Seeded training and held-out data (drawn separately) and one twin state per chain: chain c has its own assignment
    (assignments[c], or uniform over `used` groups), its own distinct_hp(family, dim, i=c) blocks (hp_of(c, j, family, dim)
    overrides) and its own alpha 0.5 + 0.375 c.  masked: held-out columns with a fifth of their entries masked.
    big_counts: some held-out gp / bnb values lie beyond the exact table (>= 1024), above every training value."""
    rng = np.random.default_rng(seed)
    used = K if used is None else used
    train = [_feature(fam, ntrain, max(used, 1), rng, dim) for fam, dim in specs]
    held = [_feature(fam, nheld, max(used, 1), rng, dim) for fam, dim in specs]
    if big_counts:
        for f in held:
            if f["family"] in (orc.GP, orc.BNB):
                pick = rng.random(nheld) < 0.15
                pick[0] = True
                f["values"] = np.where(pick, rng.integers(1024, 1500, nheld), f["values"]).astype(np.uint32)
    masks = [np.zeros(nheld, dtype=bool) for _ in specs]
    for f in masked:
        masks[f] = rng.random(nheld) < 0.2
    chains = []
    for c in range(nchains):
        z = rng.integers(0, max(used, 1), ntrain).astype(np.int32) if assignments is None else np.asarray(assignments[c], np.int32)
        feats_c = []
        for j, f in enumerate(train):
            if f["family"] == NOOP:
                feats_c.append(None)
                continue
            hp = (hp_of(c, j, f["family"], f["dim"]) if hp_of else None) or distinct_hp(f["family"], f["dim"], i=c)
            feats_c.append(dict(f, hp=hp))
        fs = state_from_assignment([f for f in feats_c if f is not None], K, z)
        it = iter(fs)
        fs = [None if f is None else next(it) for f in feats_c]
        alpha = 0.5 + 0.375 * c if alphas is None else float(alphas[c])
        counts = np.bincount(z[z >= 0], minlength=K).astype(np.uint32)
        chains.append((fs, counts, alpha))
    return EnsembleTwin(specs, K, chains, held, masks)


class EnsembleCase(object):
    """the twin and the device ensemble loaded with its states, with the held-out view"""

    def __init__(self, ctx, twin):
        import common_amd
        self.ctx, self.twin = ctx, twin
        rec = recarray_of(twin.held)
        if any(m.any() for m in twin.masks):
            mrec = np.zeros(len(rec), dtype=[(n, np.bool_) for n in rec.dtype.names])
            for i, m in enumerate(twin.masks):
                mrec["f%d" % i] = m
            rec = np.ma.masked_array(rec, mask=mrec)
        self.view = common_amd.DataView.from_recarray(ctx, rec)
        self.ens = common_amd.ChainEnsemble(ctx, twin.specs, twin.K, twin.nchains)
        for st, (fs, counts, alpha) in zip(self.ens.states, twin.chains):
            for i, item in enumerate(fs):
                if item is None:
                    continue
                F, _, ss32 = item
                st.set_hp(i, F.hp)
                rec_i = np.zeros(ss32.shape[0], dtype=common_amd.ss_dtype(F.family, F.dim))
                for name in rec_i.dtype.names:
                    rec_i[name] = ss32[name]
                st.set_ss(i, rec_i)
            st.set_group_counts(counts)
            st.set_alpha(alpha)


# ---- the exact end-to-end answer: one chain per set partition of five rows, the sixth as the query ----------------------
def partition_twin(feat6, alpha, narrow=True):
    """feat6: one make_feature dict of six rows.  narrow: the chains' suff-stats rounded to the float fields the device
    holds (False: as accumulated in double, for the identity itself).  -> (twin of Bell(5) = 52 chains over K = 6 slots, chain p seated as
    set partition p of rows 0..4 and queried with row 5; log p(partition | rows 0..4) [52]; the exact answer
    log p(x_5 | x_0..4) = log p(x_0..5) - log p(x_0..4) from the enumeration over set partitions)"""
    from tests import seq_helpers as sh
    from tests import smc_helpers as H
    F = orc.Family(feat6["family"], feat6["hp"], feat6["dim"], "f64")
    five = dict(feat6, values=feat6["values"][:5])
    query = dict(feat6, values=feat6["values"][5:])
    parts, prob = sh.exact_posterior([(F, five["values"])], alpha)
    chains = []
    for a in parts:
        z = np.asarray(a, dtype=np.int32)
        fs = state_from_assignment([five], 6, z) if narrow else [(F, F.accumulate(6, five["values"], z), None)]
        chains.append((fs, np.bincount(z, minlength=6).astype(np.uint32), alpha))
    twin = EnsembleTwin([(feat6["family"], feat6["dim"])], 6, chains, [query], [np.zeros(1, dtype=bool)])
    exact = H.exact_log_evidence([(F, feat6["values"], None)], alpha) - H.exact_log_evidence([(F, five["values"], None)], alpha)
    return twin, np.log(prob), exact
