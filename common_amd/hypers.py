"""Grid Gibbs inference of hyper-parameters the way downstream runs it (grid_feature_hp / grid_cluster_hp): every point of
a model descriptor's partial grid is merged into the feature's current hp, scored by the marginal likelihood of the
feature's groups plus the descriptor's hyper-priors, and one point is drawn from the softmax.  The scoring, the draw
and the installation of the chosen point run on the device (State.hp_gibbs, msc_hp_grid_gibbs: one host
synchronisation per step whatever the number of features); this module holds the upstream semantics of the grids:

  merged_points(desc, current_hp, partial_grid)   each partial point merged into the current hp (dicts)
  grid_blocks(desc, current_hp, partial_grid)     the same points packed as the ABI's hp blocks (runtime.pack_hp)
  grid_logprior(desc, points, hyperpriors)        sum of the hyper-priors at each point; a tuple key such as
                                                   ("alpha", "beta") is called with the values in the tuple's order
  FeatureHpGibbs(state, descs, ...)               the grids of a state's features built once, .step(seed, sweep)

and the slice sampler, downstream's `hp` kernel (State.hp_slice, msc_hp_slice: every coordinate's whole update loop in
one kernel, one host synchronisation per step):

  slice_prior(fn)                                 a scalar_functions prior -> (L.PRIOR_*, a, b)
  slice_coords(desc, feature, hparams)            one feature's msc_slice_coord entries: {key or tuple of keys: (prior,
                                                   width)}, default desc.default_hyperpriors() with width 1.0
  FeatureHpSlice(state, descs, hparams, cparam)   the entries of a state's features (and alpha), .step(seed, sweep)
  EnsembleHpSlice(ens, descs, hparams, cparam)    the same for a ChainEnsemble: every chain's step in one launch

A sharded sweep (common_amd.dist.ShardedSweep) calls .step after commit_reduce: every rank holds the same tables and
draws with the same seed, so every rank installs the same points without exchanging anything.
"""
import numpy as np

from . import _lib as L
from .runtime import pack_hp
from .scalar_functions import _log_noninformative_beta_prior, log_exponential, log_normal

_FIELDS = {L.BB: ("alpha", "beta"), L.BBNC: ("alpha", "beta"), L.GP: ("alpha", "inv_beta"),
           L.BNB: ("alpha", "beta", "r"), L.NICH: ("mu", "kappa", "sigmasq", "nu")}


def unpack_hp(family, block, dim=0):
    """the flat hp block of the ABI (State.get_hp) -> the dict microscopes/models.pyx keys it by (niw excluded)"""
    block = [float(v) for v in np.asarray(block, dtype=np.float32).ravel()]
    if family in (L.DD, L.DM):
        return {"alphas": block}
    if family not in _FIELDS:
        raise ValueError("family %d has no hyper-parameter grid" % family)
    hp = dict(zip(_FIELDS[family], block))
    if family == L.BNB:
        hp["r"] = int(round(hp["r"]))
    return hp


def _current(desc, current_hp):
    if current_hp is None:
        return dict(desc.default_hyperparams())
    if isinstance(current_hp, dict):
        return dict(current_hp)
    return unpack_hp(desc.family, current_hp, desc.dim)


def merged_points(desc, current_hp=None, partial_grid=None):
    """[current hp updated with each point of partial_grid] (default grid: desc.default_partial_hypergrid())"""
    base = _current(desc, current_hp)
    grid = desc.default_partial_hypergrid() if partial_grid is None else partial_grid
    out = []
    for pt in grid:
        m = dict(base)
        m.update(pt)
        out.append(m)
    return out


def grid_blocks(desc, current_hp=None, partial_grid=None):
    """float32 [npoints, msc_hp_floats]: the merged points packed with runtime.pack_hp"""
    pts = merged_points(desc, current_hp, partial_grid)
    if not pts:
        return np.zeros((0, len(pack_hp(desc.family, _current(desc, current_hp), desc.dim))), dtype=np.float32)
    return np.stack([pack_hp(desc.family, p, desc.dim) for p in pts])


def grid_logprior(desc, points, hyperpriors=None):
    """float64 [npoints]: sum over the hyper-priors (default desc.default_hyperpriors()) at each merged point"""
    priors = desc.default_hyperpriors() if hyperpriors is None else hyperpriors
    out = np.zeros(len(points), dtype=np.float64)
    for i, pt in enumerate(points):
        s = 0.0
        for key, fn in priors.items():
            s += fn(*[pt[k] for k in key]) if isinstance(key, tuple) else fn(pt[key])
        out[i] = s
    return out


class FeatureHpGibbs(object):
    """Grid Gibbs steps over the hyper-parameters of a state's features (and, optionally, alpha).

    descs[f]: the model descriptor of state feature f.  grids: None, or per feature None (the descriptor's default
    partial grid) or an explicit partial grid; hyperpriors likewise.  Features whose default grid is empty (dd, dm,
    niw) are skipped; an explicit empty grid is an error.  cluster_grid: None or a sequence of alpha values (> 0), with
    cluster_hyperprior a callable of alpha (None: flat).  The grids are merged into the features' hp as the state holds
    them now and uploaded once."""

    def __init__(self, state, descs, grids=None, cluster_grid=None, hyperpriors=None, cluster_hyperprior=None):
        if len(descs) != len(state.features):
            raise ValueError("one model descriptor per state feature expected")
        self.state = state
        self.features, self.points, self._grids = [], {}, []
        for f, desc in enumerate(descs):
            partial = None if grids is None else grids[f]
            if partial is not None and len(partial) == 0:
                raise ValueError("feature %d: explicit empty hyper-parameter grid" % f)
            if partial is None and len(desc.default_partial_hypergrid()) == 0:
                continue
            if (desc.family, desc.dim) != tuple(state.features[f]):
                raise ValueError("feature %d: descriptor does not match the state's feature" % f)
            pts = merged_points(desc, state.get_hp(f), partial)
            prior = grid_logprior(desc, pts, None if hyperpriors is None else hyperpriors[f])
            self._grids.append(state.hp_grid(f, np.stack([pack_hp(desc.family, p, desc.dim) for p in pts]), prior))
            self.features.append(f)
            self.points[f] = pts
        self.alphas = None
        if cluster_grid is not None:
            self.alphas = [float(a) for a in cluster_grid]
            if not self.alphas:
                raise ValueError("explicit empty alpha grid")
            prior = None if cluster_hyperprior is None else np.array([cluster_hyperprior(a) for a in self.alphas])
            self._grids.append(state.crp_grid(self.alphas, prior))

    def step(self, seed, sweep, slots=None):
        """one grid Gibbs step of every grid -> {feature: chosen merged hp dict, "alpha": chosen alpha (if any)}"""
        if not self._grids:
            return {}
        chosen = self.state.hp_gibbs(self._grids, seed, sweep, slots=slots)
        out = {f: self.points[f][int(k)] for f, k in zip(self.features, chosen)}
        if self.alphas is not None:
            out["alpha"] = self.alphas[int(chosen[-1])]
        return out

    def close(self):
        for g in self._grids:
            g.close()
        self._grids = []


def slice_prior(fn):
    """a prior of common_amd.scalar_functions -> (L.PRIOR_*, a, b) as msc_slice_coord carries it; None is flat"""
    if fn is None:
        return L.PRIOR_FLAT, 0.0, 0.0
    if isinstance(fn, log_exponential):
        return L.PRIOR_EXPONENTIAL, fn._lam, 0.0
    if isinstance(fn, log_normal):
        return L.PRIOR_NORMAL, fn._mu, fn._sigma2
    if isinstance(fn, _log_noninformative_beta_prior):
        return L.PRIOR_NONINF_BETA, 0.0, 0.0
    raise TypeError("a slice-sampled prior is one of common_amd.scalar_functions' log_exponential, log_normal or "
                    "log_noninformative_beta_prior, not %r" % (fn,))


def slice_coords(desc, feature, hparams=None):
    """the msc_slice_coord entries (State.hp_slice dicts) of state feature `feature` under `hparams` = {key or tuple of
    keys: (prior, width)} (default: desc.default_hyperpriors(), width 1.0).  A tuple key takes the noninformative beta
    prior and becomes one entry per key, each against the joint prior with the other as partner, in the tuple's order."""
    if hparams is None:
        hparams = {k: (fn, 1.0) for k, fn in desc.default_hyperpriors().items()}
    if not hparams:
        return []
    fields = _FIELDS.get(desc.family)
    if fields is None:
        raise L.MicroscopesHipError(-4, "feature %d: the %s hyper-parameters are not slice-sampled" % (feature, desc.name()))
    out = []
    for key, (fn, w) in hparams.items():
        kind, a, b = slice_prior(fn)
        keys = key if isinstance(key, tuple) else (key,)
        if (kind == L.PRIOR_NONINF_BETA) != (len(keys) == 2) or len(keys) > 2:
            raise ValueError("feature %d: %r: the noninformative beta prior takes a pair of keys, every other prior one"
                             % (feature, key))
        for i, k in enumerate(keys):
            if k not in fields:
                raise ValueError("feature %d: %s has no hyper-parameter %r" % (feature, desc.name, k))
            out.append({"feature": feature, "coord": fields.index(k), "width": float(w), "prior": kind, "a": a, "b": b,
                        "partner": fields.index(keys[1 - i]) if len(keys) == 2 else 0})
    return out


def _slice_entries(features, descs, hparams=None, cparam=None):
    """what FeatureHpSlice and EnsembleHpSlice build from their arguments -> (the entries of every feature in feature
    order, then alpha's; the features that have entries; whether alpha has one).  features: the (family, dim) list of
    the state or ensemble."""
    if len(descs) != len(features):
        raise ValueError("one model descriptor per state feature expected")
    coords, sliced = [], []
    for f, desc in enumerate(descs):
        hp = None
        if hparams is not None:
            hp = hparams.get(f) if isinstance(hparams, dict) else hparams[f]
        cs = slice_coords(desc, f, hp)
        if not cs:
            continue
        if (desc.family, desc.dim) != tuple(features[f]):
            raise ValueError("feature %d: descriptor does not match the state's feature" % f)
        coords += cs
        sliced.append(f)
    has_alpha = False
    if cparam is not None:
        if set(cparam) != {"alpha"}:
            raise ValueError("cparam takes one key, 'alpha'")
        fn, w = cparam["alpha"]
        kind, a, b = slice_prior(fn)
        if kind == L.PRIOR_NONINF_BETA:
            raise ValueError("alpha has no partner for the noninformative beta prior")
        coords.append({"feature": "alpha", "coord": 0, "width": float(w), "prior": kind, "a": a, "b": b,
                       "partner": 0})
        has_alpha = True
    return coords, sliced, has_alpha


class FeatureHpSlice(object):
    """Slice steps over the hyper-parameters of a state's features (and, optionally, alpha): downstream's `hp` kernel.

    hparams: None, or per feature (a list, or a dict keyed by feature) {key or tuple of keys: (prior, width)}, the
    priors being common_amd.scalar_functions objects; a feature hparams does not name takes the descriptor's
    default_hyperpriors() with width 1.0, and a feature with no prior (dd, dm, niw by default) is skipped.
    cparam: None or {"alpha": (prior, width)}."""

    def __init__(self, state, descs, hparams=None, cparam=None):
        self.state, self.descs = state, list(descs)
        self.coords, self.features, self.has_alpha = _slice_entries(state.features, descs, hparams, cparam)
        self.last_evals = None

    def step(self, seed, sweep, slots=None):
        """one slice step of every coordinate -> {feature: the feature's hp dict now, "alpha": alpha now (if sliced)};
        the evaluations each update took are in .last_evals"""
        if not self.coords:
            return {}
        values, self.last_evals = self.state.hp_slice(self.coords, seed, sweep, slots=slots)
        out = {f: unpack_hp(self.descs[f].family, self.state.get_hp(f), self.descs[f].dim) for f in self.features}
        if self.has_alpha:
            out["alpha"] = float(values[-1])
        return out


class EnsembleHpSlice(object):
    """FeatureHpSlice for a ChainEnsemble: the same entries, built the same way from the same arguments (one list for all
    chains), stepped on every chain in one launch (ChainEnsemble.hp_slice, msc_chains_hp_slice).  Constructing it touches
    no device."""

    def __init__(self, ens, descs, hparams=None, cparam=None):
        self.ens, self.descs = ens, list(descs)
        self.coords, self.features, self.has_alpha = _slice_entries(ens.features, descs, hparams, cparam)
        self.last_evals = self.last_values = None

    def step(self, seed, sweep, slots=None):
        """one slice step of every coordinate of every chain -> a list of nchains dicts {feature: the chain's hp dict
        now, "alpha": its alpha now (if sliced)}, built from the returned values and each state's host copy of its hp (no
        device read per chain); .last_values float32 and .last_evals uint32, [nchains, n], are what the step installed
        and the evaluations each update took"""
        nchains = self.ens.nchains
        if not self.coords:
            self.last_values = np.zeros((nchains, 0), np.float32)
            self.last_evals = np.zeros((nchains, 0), np.uint32)
            return [{} for _ in range(nchains)]
        self.last_values, self.last_evals = self.ens.hp_slice(self.coords, seed, sweep, slots=slots)
        out = []
        for c, st in enumerate(self.ens.states):
            d = {f: unpack_hp(self.descs[f].family, st.get_hp(f), self.descs[f].dim) for f in self.features}
            if self.has_alpha:
                d["alpha"] = float(self.last_values[c, -1])
            out.append(d)
        return out
