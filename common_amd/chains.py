"""Many independent sequential Gibbs chains swept in one launch, a workgroup each (msc_chains_*, include/microscopes_hip.h).

A ChainEnsemble owns nchains State objects of one shape and their assignment vectors.  Chain c of a sweep does exactly what
State.sweep_sequential does on ens.states[c] with the same seed and arguments; the ensemble only runs them side by side.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib as L
from . import smc as S
from . import tempering as T
from .runtime import _I32_U32, State

_U64 = (1 << 64) - 1

# what ChainEnsemble.run returns: the thinned trace (int32 device tensor [nchains, niters // trace_every, nrows] or None)
# and the values every iteration's hp step installed (float32 host array [nchains, niters, ncoords])
RunResult = collections.namedtuple("RunResult", ["trace", "values"])


def trace_shape(nsweeps, trace_every, nchains, nrows):
    """shape of the thinned trace of a sweep call: [nchains, nsweeps // trace_every, nrows] -- sample j of a chain is its z
    after sweep (j + 1) * trace_every - 1 of the call; sweeps beyond the last whole multiple leave no sample"""
    nsweeps, trace_every, nchains, nrows = int(nsweeps), int(trace_every), int(nchains), int(nrows)
    if trace_every < 1:
        raise ValueError("trace_every must be >= 1")
    if nsweeps < 0 or nchains < 0 or nrows < 0:
        raise ValueError("nsweeps, nchains and nrows must be >= 0")
    return (nchains, nsweeps // trace_every, nrows)


def chain_seeds(seed, nchains):
    """the Philox key of every chain: an int gives chain c the key seed + c (mod 2^64); a sequence gives its entries"""
    nchains = int(nchains)
    if isinstance(seed, (int, np.integer)):
        return [(int(seed) + c) & _U64 for c in range(nchains)]
    seeds = [int(s) for s in seed]
    if len(seeds) != nchains:
        raise ValueError("seed must be an int or a sequence of nchains = %d ints (got %d)" % (nchains, len(seeds)))
    for s in seeds:
        if not 0 <= s <= _U64:
            raise ValueError("every seed must lie in [0, 2^64)")
    return seeds


# what ChainEnsemble.split_merge returns: counters int64 device tensor [nchains, 5] = {splits proposed, splits accepted,
# merges proposed, merges accepted, void} of THIS call; log float64 [nchains, nproposals, 8], trace and proposed int32
# [nchains, nproposals, nrows] on the device, or None where not asked for
SplitMergeResult = collections.namedtuple("SplitMergeResult", ["counters", "log", "trace", "proposed"])

SPLIT_MERGE_MAX_LAUNCH_ITERS = 1024


def split_merge_args(seed, nchains, nproposals, launch_iters):
    """the argument checks of ChainEnsemble.split_merge that need no device -> (seeds, nproposals, launch_iters)"""
    seeds = chain_seeds(seed, nchains)
    nproposals, launch_iters = int(nproposals), int(launch_iters)
    if not 0 <= nproposals < (1 << 32):
        raise ValueError("nproposals must be in [0, 2^32)")
    if not 0 <= launch_iters <= SPLIT_MERGE_MAX_LAUNCH_ITERS:
        raise ValueError("launch_iters must be in [0, %d]" % SPLIT_MERGE_MAX_LAUNCH_ITERS)
    return seeds, nproposals, launch_iters


def _per_chain(what, value, nchains, is_one):
    """one value for all chains, or a sequence of one per chain -> list of nchains"""
    if value is None:
        return [None] * nchains
    if is_one(value):
        return [value] * nchains
    value = list(value)
    if len(value) != nchains:
        raise ValueError("%s must be one value or one per chain (%d chains, got %d)" % (what, nchains, len(value)))
    return value


class ChainEnsemble(object):
    """nchains states of the same features and ngroups, swept together.

    alpha: one float or nchains floats.  hps: one list with an hp (dict or packed array) per feature, used by every chain,
    or nchains such lists.  ens.states[c] is an ordinary State: get_ss, hp_slice, predictive_logp, set_hp, ... work on it
    between sweeps.  ens.z: int32 [nchains, nrows] on the device once assign() / seat() has run; ens.logw: float64
    [nchains] on the device, zeroed there, the log weights visit() adds the visits' log predictives to;
    ens.split_merge_counters: int64 [nchains, 5] on the device, zeroed there, what run(split_merge=n) adds its proposals'
    counters to."""

    def __init__(self, ctx, features, ngroups, nchains, alpha=None, hps=None):
        nchains = int(nchains)
        if nchains < 1:
            raise ValueError("nchains must be >= 1")
        self.ctx, self.nchains, self.K = ctx, nchains, int(ngroups)
        self.states, self._h, self.z, self.logw, self.split_merge_counters = [], None, None, None, None
        alphas = _per_chain("alpha", alpha, nchains, lambda a: isinstance(a, (int, float, np.floating, np.integer)))
        hpsets = _per_chain("hps", hps, nchains, lambda h: len(h) > 0 and isinstance(h[0], (dict, np.ndarray)))
        try:
            for c in range(nchains):
                st = State(ctx, features, ngroups)
                self.states.append(st)
                if hpsets[c] is not None:
                    if len(hpsets[c]) != len(st.features):
                        raise ValueError("hps needs one entry per feature (%d, got %d)" % (len(st.features), len(hpsets[c])))
                    for f, hp in enumerate(hpsets[c]):
                        st.set_hp(f, hp)
                if alphas[c] is not None:
                    st.set_alpha(alphas[c])
            self._h = _create(ctx, self.states)
        except Exception:
            self.close()
            raise
        self.features = self.states[0].features

    # the assignment -----------------------------------------------------------
    def assign(self, view, z):
        """start every chain from z (int32 [nchains, nrows] or [nrows] for all, host or device; ids outside [0, ngroups)
        are unassigned): ens.z becomes a copy and every state's tables are accumulated from its row"""
        self._check_open()
        n = int(view.nrows)
        zt = torch.as_tensor(z)
        if zt.dtype != torch.int32 or zt.dim() not in (1, 2) or zt.shape[-1] != n or (zt.dim() == 2 and zt.shape[0] != self.nchains):
            raise ValueError("z must be int32 [nchains = %d, nrows = %d] or [nrows]" % (self.nchains, n))
        zt = zt.to(self.ctx.torch_device)
        self.z = (zt.expand(self.nchains, n) if zt.dim() == 1 else zt).contiguous().clone()
        self.logw = torch.zeros(self.nchains, dtype=torch.float64, device=self.ctx.torch_device)
        self.split_merge_counters = torch.zeros((self.nchains, 5), dtype=torch.int64, device=self.ctx.torch_device)
        for c, st in enumerate(self.states):
            st.accumulate(view, self.z[c])
        self._view = view

    def seat(self, view, seed=None, sweep=0):
        """every row of every chain unassigned and the tables empty; the first sweep that follows is then sequential CRP
        seating.  With a seed that sweep is run here (keys as in sweep(), sweep index `sweep`), so ens.z holds groups on return"""
        self.assign(view, torch.full((int(view.nrows),), -1, dtype=torch.int32))
        if seed is not None:
            self.sweep(view, 1, seed, sweep=sweep)

    def _z_at(self, row0):
        """pointer to column row0 of chain 0's row of self.z (the ensemble's own tensor: assign() made it)"""
        zp = self.z.data_ptr() + 4 * row0
        return C.c_void_p(zp)

    # the sweep ----------------------------------------------------------------
    def sweep(self, view, nsweeps, seed, sweep=0, order=None, trace_every=None, zmatrix=None, want_occupied=False, row0=0,
              nrows=None, row_id0=None, cols=None, beta=None):
        """nsweeps sequential sweeps of every chain over rows [row0, row0 + nrows) (msc_chains_sweep; asynchronous).
        seed: an int (chain c takes seed + c) or nchains ints; sweep: the counter's sweep index of the first sweep.
        order: uint32 / int32 device tensor [nrows] (all chains) or [nchains, nrows] of offsets from row0.
        trace_every = e: -> the int32 device tensor [nchains, nsweeps // e, nrows] holding z of the row range after every
        e-th sweep; with want_occupied -> (trace, occupied), occupied int32 [nchains, nsweeps // e] the groups in use at
        those moments.  zmatrix: a ZMatrix over the nrows rows that takes the whole trace in one add (trace_every
        defaults to 1 then).  Without any of the three -> None.
        beta: None, exactly the call above; otherwise every chain is swept at its own temperature
        (msc_chains_sweep_tempered; asynchronous too): a float32 device tensor [nchains], read on the device when the
        sweep runs -- what exchange() swapped in it is what the sweep sees -- or a float or nchains floats, made into
        one.  Chain c targets p(z | alpha) p(X | z, hp)^beta[c]; at beta = 1 every bit is the untempered call's, at
        beta = 0 no feature is read (from seat(): a draw from the CRP prior).  A NaN, negative or infinite entry stops
        its chain for the call and raises MicroscopesHipError at the next one."""
        self._check_open()
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        dev = self.ctx.torch_device
        row0, n = A.rows(int(view.nrows), row0, nrows)
        if row0 + n > self.z.shape[1] or self.z.shape[1] != view.nrows:      # (the trace is sized before the call)
            raise ValueError("rows [%d, %d) outside the assignment (%d rows)" % (row0, row0 + n, self.z.shape[1]))
        nsweeps = int(nsweeps)
        if not 0 <= nsweeps < (1 << 32):
            raise ValueError("nsweeps must be in [0, 2^32)")
        seeds = chain_seeds(seed, self.nchains)
        bp = None
        if beta is not None:
            beta = self._beta(beta)                  # (kept alive until the call is made)
            bp = A.ptr(beta)
        op, ld_order = None, 0
        if order is not None:
            op, ld_order = A.flat(order, _I32_U32, n, dev, "order"), (n if order.dim() == 2 else 0)
            if tuple(order.shape) not in ((n,), (self.nchains, n)):
                raise ValueError("order must hold [nrows] or [nchains, nrows] entries")
        if (zmatrix is not None or want_occupied) and trace_every is None:
            trace_every = 1
        trace = occupied = None
        if trace_every is not None:
            shape = trace_shape(nsweeps, trace_every, self.nchains, n)
            if zmatrix is not None and (zmatrix.n != n or zmatrix.ctx is not self.ctx):
                raise ValueError("zmatrix must be over the %d rows of the sweep, on the ensemble's context" % n)
            trace = torch.empty(shape, dtype=torch.int32, device=dev)
            if want_occupied:
                occupied = torch.empty(shape[:2], dtype=torch.int32, device=dev)
        for st in self.states:
            st._drop_subsets()
            st._bound_view = view        # (the library keeps no reference to a view: the states do, for the last one bound)
        head = (self._h, view._h, self.states[0]._cols(cols), row0, n, row0 if row_id0 is None else int(row_id0),
                self._z_at(row0), int(self.z.stride(0)), op, ld_order, nsweeps, (C.c_uint64 * self.nchains)(*seeds), int(sweep))
        tail = (0 if trace_every is None else int(trace_every),
                A.ptr(trace) if trace is not None and trace.numel() else None,
                A.ptr(occupied) if occupied is not None and occupied.numel() else None)
        if bp is None:
            L.check(self.ctx.lib.msc_chains_sweep(*(head + tail)))
        else:
            L.check(self.ctx.lib.msc_chains_sweep_tempered(*(head + (bp,) + tail)))
        if zmatrix is not None and trace.shape[1] > 0:
            zmatrix.add(trace.view(-1, n))
        if trace is None:
            return None
        return (trace, occupied) if want_occupied else trace

    def _beta(self, beta):
        """the temperatures of a tempered sweep as a float32 device tensor [nchains]: such a tensor as it is, or one made
        from a float (all chains) or nchains floats"""
        dev = self.ctx.torch_device
        if isinstance(beta, torch.Tensor):
            if tuple(beta.shape) != (self.nchains,):
                raise ValueError("beta must hold nchains = %d temperatures (got shape %s)" % (self.nchains, tuple(beta.shape)))
            A.flat(beta, torch.float32, self.nchains, dev, "beta")
            return beta
        b = np.asarray(beta, dtype=np.float32)
        if b.ndim == 0:
            b = np.full(self.nchains, b, dtype=np.float32)
        if b.shape != (self.nchains,):
            raise ValueError("beta must be one float or nchains = %d floats (got shape %s)" % (self.nchains, b.shape))
        return torch.from_numpy(b).to(dev)

    # part of a sweep, with the visits' log predictives --------------------------
    def _order(self, order, n):
        if order is None:
            return None, 0
        op = A.flat(order, _I32_U32, n, self.ctx.torch_device, "order")
        if tuple(order.shape) not in ((n,), (self.nchains, n)):
            raise ValueError("order must hold [nrows] or [nchains, nrows] entries")
        return op, (n if order.dim() == 2 else 0)

    def visit(self, view, pos0, npos, seed, sweep=0, order=None, want_logp=False, row0=0, nrows=None, row_id0=None,
              cols=None):
        """positions [pos0, pos0 + npos) of the order of ONE sweep of every chain over rows [row0, row0 + nrows)
        (msc_chains_visit; asynchronous): the visits sweep(view, 1, seed, sweep=sweep, order=order) makes at those
        positions, bit for bit, so calls over [0, a), [a, b), ... [y, nrows) together are that sweep.  Every visit's log
        predictive -- log p(row | the rows seated at that moment), from the draw's own max and sum -- is added to
        ens.logw[c] in double, in visit order.  want_logp: -> float32 device tensor [nchains, nrows] of those increments
        by order POSITION, NaN where this call made no visit; otherwise -> None."""
        self._check_open()
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        dev = self.ctx.torch_device
        row0, n = A.rows(int(view.nrows), row0, nrows)
        if row0 + n > self.z.shape[1] or self.z.shape[1] != view.nrows:
            raise ValueError("rows [%d, %d) outside the assignment (%d rows)" % (row0, row0 + n, self.z.shape[1]))
        pos0, npos = int(pos0), int(npos)
        if pos0 < 0 or npos < 0 or pos0 + npos > n:
            raise ValueError("positions [%d, %d) outside the order (%d rows)" % (pos0, pos0 + npos, n))
        seeds = chain_seeds(seed, self.nchains)
        op, ld_order = self._order(order, n)
        logp = torch.full((self.nchains, n), float("nan"), dtype=torch.float32, device=dev) if want_logp else None
        for st in self.states:
            st._drop_subsets()
            st._bound_view = view
        L.check(self.ctx.lib.msc_chains_visit(
            self._h, view._h, self.states[0]._cols(cols), row0, n, row0 if row_id0 is None else int(row_id0),
            self._z_at(row0), int(self.z.stride(0)), op, ld_order, pos0, npos, (C.c_uint64 * self.nchains)(*seeds), int(sweep),
            A.ptr(self.logw), A.ptr(logp) if logp is not None and logp.numel() else None, n))
        return logp

    def clone(self, ancestors):
        """chain c becomes chain ancestors[c] wherever the two differ (msc_chains_clone; asynchronous, one launch): its z
        row and its state's sums are the ancestor's bits; hyper-parameters, alpha and ens.logw are left alone.
        ancestors: nchains ints with ancestors[ancestors[c]] == ancestors[c] (a source survives in place:
        smc.systematic_ancestors arranges them so); anything else is a ValueError and changes nothing."""
        self._check_open()
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        anc = [int(a) for a in np.asarray(ancestors).ravel()]
        if len(anc) != self.nchains:
            raise ValueError("ancestors must hold nchains = %d entries (got %d)" % (self.nchains, len(anc)))
        for c, a in enumerate(anc):
            if not 0 <= a < self.nchains:
                raise ValueError("ancestor %d of chain %d is not a chain (%d chains)" % (a, c, self.nchains))
            if anc[a] != a:
                raise ValueError("chain %d copies chain %d, which is itself overwritten: a source must survive in place"
                                 % (c, a))
        for c, a in enumerate(anc):
            if a != c:
                self.states[c]._drop_subsets()
        L.check(self.ctx.lib.msc_chains_clone(self._h, (C.c_uint32 * self.nchains)(*anc), A.ptr(self.z),
                                              int(self.z.stride(0)), int(self.z.shape[1])))

    # the hyper-parameter step ---------------------------------------------------
    def _check_hp_slice(self, seed, slots):
        """the argument checks of hp_slice that need no library -> (seeds, slots' pointer, ld_slots)"""
        self._check_open()
        seeds = chain_seeds(seed, self.nchains)
        if slots is None:
            return seeds, None, 0
        if not isinstance(slots, torch.Tensor) or tuple(slots.shape) not in ((self.K,), (self.nchains, self.K)):
            raise ValueError("slots must be a uint8 tensor [ngroups = %d] (all chains) or [nchains = %d, ngroups]"
                             % (self.K, self.nchains))
        sp = A.flat(slots, torch.uint8, slots.numel(), self.ctx.torch_device, "slots")
        return seeds, sp, (self.K if slots.dim() == 2 else 0)

    def hp_slice(self, coords, seed, sweep=0, slots=None):
        """one slice step of each entry of `coords` on EVERY chain (msc_chains_hp_slice: one launch for the step, one for
        the score and CRP tables it made stale, one host synchronisation).  coords: State.hp_slice's dicts, one list for
        all chains.  seed: an int (chain c takes seed + c) or nchains ints.  slots: uint8 device mask of the counted
        groups, [ngroups] for all chains or [nchains, ngroups] (default: each chain's non-empty ones).
        -> (installed values float32 [nchains, n], evaluations uint32 [nchains, n]) as numpy.
        Chain c ends exactly where ens.states[c].hp_slice(coords, chain_seeds(seed, nchains)[c], sweep, slots_c) would
        have left it, bit for bit.  Afterwards the chains no longer share hyper-parameters and alpha (see smc())."""
        seeds, sp, ld_slots = self._check_hp_slice(seed, slots)
        coords = list(coords)
        arr = State._slice_coord_array(coords)
        values = np.zeros((self.nchains, len(coords)), dtype=np.float32)
        evals = np.zeros((self.nchains, len(coords)), dtype=np.uint32)
        for st in self.states:
            st._drop_subsets()
        L.check(self.ctx.lib.msc_chains_hp_slice(self._h, arr, len(coords), sp, ld_slots, (C.c_uint64 * self.nchains)(*seeds),
                                                 int(sweep), values.ctypes.data_as(C.c_void_p),
                                                 evals.ctypes.data_as(C.c_void_p)))
        return values, evals

    # the log joint ----------------------------------------------------------------
    def score_joint(self, priors=None, slots=None, out=None):
        """log p(X, z | hp, alpha) of EVERY chain and its parts in one launch (msc_chains_score_joint; asynchronous, no
        host synchronisation, changes nothing): a float64 device tensor [nchains, nfeatures + 3], row c = (total,
        score_assignment, the features' summed score_data ..., the hyper-priors' sum) of chain c -- bit for bit what
        ens.states[c].score_joint(priors, slots_c) gives, whatever the number of chains.  priors: State.score_joint's
        (one list for all chains, or a hypers.EnsembleHpSlice).  slots: uint8 device mask of the counted groups,
        [ngroups] for all chains or [nchains, ngroups] (default: each chain's non-empty ones).  out: a float64 device
        tensor of at least [nchains, nfeatures + 3] with contiguous rows (any row stride)."""
        _, sp, ld_slots = self._check_hp_slice(0, slots)
        arr, n = State._joint_priors(priors)
        width = len(self.features) + 3
        if out is None:
            out = torch.empty((self.nchains, width), dtype=torch.float64, device=self.ctx.torch_device)
        op, ld = A.matrix(out, torch.float64, self.nchains, width, self.ctx.torch_device, "out")
        L.check(self.ctx.lib.msc_chains_score_joint(self._h, arr, n, sp, ld_slots, op, ld))
        return out

    # tempered chains: the steps between sweeps -----------------------------------------
    def exchange(self, joint, beta, rung, nrungs, parity, seed, sweep, counters):
        """one replica-exchange step of every ladder of nrungs chains (msc_chains_exchange; asynchronous, one launch, no
        state is read or changed).  joint: score_joint()'s rows, float64 device [nchains, nfeatures + 3]; beta float32 and
        rung int32 device tensors [nchains] -- within ladder l, chains [l nrungs, (l + 1) nrungs), rung is a permutation of
        0 .. nrungs - 1 (tempering.ladder gives the temperatures of the rungs).  For every j < nrungs - 1 with j % 2 ==
        parity % 2 the chains a, b holding rungs j, j + 1 swap their entries of beta and rung when log u < (beta_a - beta_b)
        (L_b - L_a), L the data log-likelihood summed from the joint row and u the Philox uniform of (key seed, counter
        (l nrungs + j, sweep)) -- give it a key no sweep of the chains uses.  The temperatures move, the states stay.
        counters: (proposed, accepted), int32 device tensors [nchains // nrungs, nrungs - 1], added to.  A ladder whose
        rungs are no permutation is left alone and raises at the next call."""
        self._check_open()
        dev, nrungs = self.ctx.torch_device, int(nrungs)
        if nrungs < 1 or self.nchains % nrungs:
            raise ValueError("nchains = %d is no whole number of ladders of %d rungs" % (self.nchains, nrungs))
        jp, ld = A.matrix(joint, torch.float64, self.nchains, len(self.features) + 3, dev, "joint")
        bp = A.flat(beta, torch.float32, self.nchains, dev, "beta")
        rp = A.flat(rung, torch.int32, self.nchains, dev, "rung")
        proposed, accepted = counters
        npairs = (self.nchains // nrungs) * (nrungs - 1)
        pp = A.flat(proposed, _I32_U32, npairs, dev, "counters[0]")
        ap = A.flat(accepted, _I32_U32, npairs, dev, "counters[1]")
        seed, sweep, parity = int(seed), int(sweep), int(parity)
        if not 0 <= seed <= _U64 or not 0 <= sweep <= _U64 or not 0 <= parity <= _U64:
            raise ValueError("seed, sweep and parity must lie in [0, 2^64)")
        L.check(self.ctx.lib.msc_chains_exchange(self._h, jp, ld, nrungs, bp, rp, parity, seed, sweep, pp, ap))

    def anneal_weights(self, joint, beta_from, beta_to, logw=None):
        """logw[c] += (beta_to[c] - beta_from[c]) L_c in double (msc_chains_anneal_weights; asynchronous, one launch): the
        weight of one step of annealed importance sampling.  joint: score_joint()'s rows; beta_from, beta_to: float32 device
        tensors [nchains]; logw: a float64 device tensor [nchains] (default ens.logw).  Equal temperatures leave an entry
        untouched."""
        self._check_open()
        dev = self.ctx.torch_device
        logw = self.logw if logw is None else logw
        jp, ld = A.matrix(joint, torch.float64, self.nchains, len(self.features) + 3, dev, "joint")
        L.check(self.ctx.lib.msc_chains_anneal_weights(
            self._h, jp, ld, A.flat(beta_from, torch.float32, self.nchains, dev, "beta_from"),
            A.flat(beta_to, torch.float32, self.nchains, dev, "beta_to"), A.flat(logw, torch.float64, self.nchains, dev, "logw")))

    # split-merge proposals --------------------------------------------------------
    def split_merge(self, view, seed, sweep=0, nproposals=1, launch_iters=2, want_log=False, want_trace=False,
                    want_proposed=False, row_id0=0):
        """nproposals split-merge proposals on EVERY chain in one launch (msc_chains_split_merge; asynchronous, no host
        synchronisation), proposal p with the sweep counter sweep + p.  seed: an int (chain c takes seed + c) or nchains
        ints.  Chain c proposes, decides and moves as ens.states[c].split_merge(view, ens.z[c], seeds[c], sweep, nproposals,
        launch_iters) does -- the same streams and arithmetic; only the order of the double sums differs -- over all rows of
        the view.  Every table of every state must be that of its row of ens.z (as after assign(), sweep() or this call) and
        is current again on return: a sweep can follow at once.
        -> SplitMergeResult(counters, log, trace, proposed): counters int64 [nchains, 5] = {splits proposed, accepted,
        merges proposed, accepted, void} of this call; with want_log float64 [nchains, nproposals, 8] = State.split_merge's
        log rows; with want_trace int32 [nchains, nproposals, nrows], z after every proposal; with want_proposed int32
        [nchains, nproposals, nrows], the proposed pair labels (-1 outside the two groups); all on the device, None where
        not asked for.  A shape whose single proposal is estimated beyond a launch's budget raises MicroscopesHipError
        (unsupported): loop over ens.states[c].split_merge there, whose kernels are parallel over rows."""
        self._check_open()
        seeds, nprop, iters = split_merge_args(seed, self.nchains, nproposals, launch_iters)
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        n = int(view.nrows)
        if self.z.shape[1] != n:
            raise ValueError("the view has %d rows, the assignment %d" % (n, self.z.shape[1]))
        dev = self.ctx.torch_device
        counters = torch.zeros((self.nchains, 5), dtype=torch.int64, device=dev)
        log = torch.zeros((self.nchains, nprop, 8), dtype=torch.float64, device=dev) if want_log else None
        trace = torch.empty((self.nchains, nprop, n), dtype=torch.int32, device=dev) if want_trace else None
        proposed = torch.empty((self.nchains, nprop, n), dtype=torch.int32, device=dev) if want_proposed else None
        for st in self.states:
            st._drop_subsets()
            st._bound_view = view        # (the library keeps no reference to a view: the states do, for the last one bound)

        def ptr(t):
            return A.ptr(t) if t is not None and t.numel() else None

        L.check(self.ctx.lib.msc_chains_split_merge(
            self._h, view._h, self.states[0]._cols(None), n, int(row_id0), self._z_at(0), int(self.z.stride(0)), nprop, iters,
            (C.c_uint64 * self.nchains)(*seeds), int(sweep), ptr(log), ptr(trace), ptr(proposed), A.ptr(counters)))
        return SplitMergeResult(counters=counters, log=log, trace=trace, proposed=proposed)

    def run(self, view, niters, seed, hp=None, sweep=0, order=None, trace_every=None, zmatrix=None, split_merge=None,
            joint=None):
        """niters iterations of the sampler on every chain: iteration i is self.sweep(view, 1, seed, sweep=sweep + i,
        order=order) followed, when split_merge=n is given, by self.split_merge(view, seed, sweep=(sweep + i) * n,
        nproposals=n) (whose counters are added to ens.split_merge_counters) and, when hp (a hypers.EnsembleHpSlice of this
        ensemble) is given, by hp.step(seed, sweep + i)
        -- exactly those calls, so exactly what they give made by hand.  -> RunResult(trace, values): trace the int32
        device tensor [nchains, niters // trace_every, nrows] of every chain's z after each trace_every-th iteration
        (trace_every None: after every iteration when a zmatrix is given, else no trace and trace is None); values the
        float32 host array [nchains, niters, ncoords] of what each step installed, in the order of hp.coords (ncoords =
        0 without hp).  zmatrix: a ZMatrix over the view's rows that takes the whole trace in one add.
        joint: a JointTracker of this ensemble; at the end of every iteration whose count (over all the runs the tracker
        has seen) is a multiple of tracker.every, self.score_joint writes the chains' log joint into the tracker's next
        sample and, with keep_best, msc_chains_keep_best keeps every chain's best z (iteration number sweep + i).  Two
        asynchronous launches a sample; without `joint` run makes exactly the calls it made before."""
        self._check_open()
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        niters, n = int(niters), int(view.nrows)
        if niters < 0:
            raise ValueError("niters must be >= 0")
        if hp is not None and getattr(hp, "ens", None) is not self:
            raise ValueError("hp must be an EnsembleHpSlice of this ensemble")
        if split_merge is not None and not 0 <= int(split_merge) < (1 << 32):
            raise ValueError("split_merge must be None or a number of proposals in [0, 2^32)")
        if joint is not None and (not isinstance(joint, JointTracker) or joint.ens is not self):
            raise ValueError("joint must be a JointTracker of this ensemble")
        if zmatrix is not None and trace_every is None:
            trace_every = 1
        trace = None
        if trace_every is not None:
            shape = trace_shape(niters, trace_every, self.nchains, n)
            if zmatrix is not None and (zmatrix.n != n or zmatrix.ctx is not self.ctx):
                raise ValueError("zmatrix must be over the %d rows of the view, on the ensemble's context" % n)
            trace = torch.empty(shape, dtype=torch.int32, device=self.ctx.torch_device)
        ncoords = len(hp.coords) if hp is not None else 0
        values = np.zeros((self.nchains, niters, ncoords), dtype=np.float32)
        for i in range(niters):
            self.sweep(view, 1, seed, sweep=sweep + i, order=order)
            if split_merge is not None:
                n_sm = int(split_merge)
                self.split_merge_counters += self.split_merge(view, seed, sweep=(sweep + i) * n_sm, nproposals=n_sm).counters
            if hp is not None:
                hp.step(seed, sweep + i)
                if ncoords:
                    values[:, i, :] = hp.last_values
            if trace is not None and (i + 1) % trace_every == 0:
                trace[:, (i + 1) // trace_every - 1, :].copy_(self.z)
            if joint is not None:
                joint._iteration(sweep + i, niters - i)
        if zmatrix is not None and trace.shape[1] > 0:
            zmatrix.add(trace.view(-1, n))
        return RunResult(trace=trace, values=values)

    def smc(self, view, seed, order=None, block=None, ess_threshold=0.5, resample_seed=None, final_resample=False, sweep=0):
        """A particle filter over the rows, the chains as particles -> smc.SMCResult, whose log_evidence estimates
        log p(X | hp, alpha), the marginal likelihood of the mixture.

        Every particle is seated from all-unassigned (seat(view)) and visits the order in blocks of `block` positions
        (default max(1, nrows // 64)); a row's incremental weight is its predictive density given the rows seated before
        it (visit()).  After every block but the last comes a checkpoint: the nchains log weights are copied to the host
        -- the ONE synchronisation with the device per checkpoint -- and the effective sample size is computed there.  If
        ess < ess_threshold * nchains the particles are resampled: log_mean_exp(logw) is added to the estimate,
        smc.systematic_ancestors(logw, u) chooses the ancestors, clone() copies them and ens.logw is zeroed.
        ess_threshold = 0 never resamples (plain sequential importance sampling); float("inf") always does.  u comes from
        numpy.random.Generator(numpy.random.Philox(key=resample_seed)), resample_seed defaulting to the first chain's
        key; one random() is drawn per checkpoint whether or not it is used, so a run is reproducible from its arguments.
        exp(log_evidence) is unbiased for p(X) whatever the threshold, provided all chains share hyper-parameters and alpha
        -- which hp_slice() (and run() with an hp step) ends: every chain then holds its own; set them equal again first.

        final_resample: one more resampling after the last block, so that the particles end equally weighted: ens.z can go
        straight into a ZMatrix and ens.sweep can continue from them.

        result.truncated: during seating rows only join, so the occupied slots never decrease; a particle that ends with
        an empty slot had one at every visit and the estimate is for the exact CRP.  If a particle ends with all ngroups
        slots occupied, a new group may have been refused somewhere, and the estimate is for the mixture truncated to
        ngroups slots: truncated is True then."""
        self._check_open()
        n, P = int(view.nrows), self.nchains
        seeds = chain_seeds(seed, P)
        block = max(1, n // 64) if block is None else int(block)
        if block < 1:
            raise ValueError("block must be >= 1")
        ess_threshold = float(ess_threshold)
        if not ess_threshold >= 0.0:
            raise ValueError("ess_threshold must be >= 0")
        rng = np.random.Generator(np.random.Philox(key=seeds[0] if resample_seed is None else int(resample_seed)))
        self.seat(view)
        log_z, ess_list, resampled_at, ancestors = 0.0, [], [], []

        def resample(pos, logw, u):
            a = S.systematic_ancestors(logw, u)
            self.clone(a)
            self.logw.zero_()
            resampled_at.append(pos)
            ancestors.append(a)

        for pos0 in range(0, n, block):
            npos = min(block, n - pos0)
            self.visit(view, pos0, npos, seeds, sweep=sweep, order=order)
            if pos0 + npos == n:
                break
            logw = self.logw.cpu().numpy()               # the checkpoint's one synchronisation
            u = rng.random()                             # (drawn whether or not it is used)
            ess_list.append(S.ess(logw))
            if ess_list[-1] < ess_threshold * P:
                log_z += S.log_mean_exp(logw)
                resample(pos0 + npos, logw, u)
        logw = self.logw.cpu().numpy()
        ess_list.append(S.ess(logw))
        log_evidence = log_z + S.log_mean_exp(logw)
        if final_resample:
            resample(n, logw, rng.random())
            logw = np.zeros(P)
        # occupied slots of every particle, from its z row (every seated row holds a slot id)
        seen = torch.zeros((P, self.K + 1), dtype=torch.int32, device=self.ctx.torch_device)
        seen.scatter_(1, (self.z.clamp(-1, self.K - 1) + 1).long(), 1)
        truncated = bool((seen[:, 1:].sum(1) >= self.K).any().item()) if n else False
        return S.SMCResult(log_evidence=log_evidence, log_weights=logw, weights=S.normalised_weights(logw), ess=ess_list,
                           resampled_at=resampled_at, ancestors=ancestors, truncated=truncated)

    # tempered chains: the drivers ---------------------------------------------------------
    def run_tempered(self, view, niters, seed, betas, sweep=0, order=None, trace_every=None, zmatrix=None, state=None):
        """niters iterations of replica exchange (parallel tempering) -> tempering.TemperedResult.

        betas: the ladder of R temperatures, rung 0 first (tempering.ladder gives such ladders; betas[0] = 1 makes rung 0
        the posterior); nchains must be a multiple of R.  Ladder l owns chains [l R, (l + 1) R) and chain l R + j starts on
        rung j; with state=an earlier TemperedResult the run continues from copies of its beta, rung, proposed and
        accepted (give it the sweep counter the earlier run ended at).  Iteration i, with counter s = sweep + i, is
        exactly these calls in this order, so exactly what they give made by hand:
          self.sweep(view, 1, seed, sweep=s, order=order, beta=beta)
          self.score_joint(out=joint)
          when (i + 1) % trace_every == 0: device copies of ens.z and rung into the next sample of trace and rungs --
              after the sweep and BEFORE the exchange, so a sample belongs to the rung its chain was swept at
          self.exchange(joint, beta, rung, R, parity=s, seed=tempering.exchange_key(seed), sweep=s,
                        counters=(proposed, accepted))
        The loop makes no host synchronisation.  trace_every None: no trace (1 when a zmatrix is given).  zmatrix: a ZMatrix
        over the view's rows that takes tempering.cold_samples(trace, rungs) -- the samples taken on rung 0 -- in one add
        after the loop.
        There is no hyper-parameter step and no split-merge here: as built both take the likelihood at full weight, so
        neither leaves pi_beta invariant.  The swap rule compares the chains' likelihoods under ONE model: all chains of a
        ladder must share hyper-parameters and alpha -- which hp_slice() (and run() with an hp step) ends: every chain
        then holds its own; set them equal again first."""
        self._check_open()
        if self.z is None:
            raise ValueError("no assignment yet: call assign() or seat() first")
        niters, n = int(niters), int(view.nrows)
        if niters < 0:
            raise ValueError("niters must be >= 0")
        ladder = np.asarray(betas, dtype=np.float32).ravel()
        R = int(ladder.size)
        if R < 1 or self.nchains % R:
            raise ValueError("nchains = %d is no whole number of ladders of %d rungs" % (self.nchains, R))
        if state is not None and not isinstance(state, T.TemperedResult):
            raise ValueError("state must be a TemperedResult of an earlier run_tempered")
        if zmatrix is not None and trace_every is None:
            trace_every = 1
        dev, nl = self.ctx.torch_device, self.nchains // R
        trace = rungs = None
        if trace_every is not None:
            shape = trace_shape(niters, trace_every, self.nchains, n)
            if zmatrix is not None and (zmatrix.n != n or zmatrix.ctx is not self.ctx):
                raise ValueError("zmatrix must be over the %d rows of the view, on the ensemble's context" % n)
            trace = torch.empty(shape, dtype=torch.int32, device=dev)
            rungs = torch.empty(shape[:2], dtype=torch.int32, device=dev)
        if state is None:
            beta = torch.from_numpy(np.tile(ladder, nl)).to(dev)
            rung = torch.arange(R, dtype=torch.int32).repeat(nl).to(dev)
            proposed = torch.zeros((nl, R - 1), dtype=torch.int32, device=dev)
            accepted = torch.zeros((nl, R - 1), dtype=torch.int32, device=dev)
        else:
            beta, rung, proposed, accepted = (t.clone() for t in (state.beta, state.rung, state.proposed, state.accepted))
            if tuple(beta.shape) != (self.nchains,) or tuple(rung.shape) != (self.nchains,) or \
                    tuple(proposed.shape) != (nl, R - 1) or tuple(accepted.shape) != (nl, R - 1):
                raise ValueError("state is not that of %d ladders of %d rungs" % (nl, R))
        joint = torch.empty((self.nchains, len(self.features) + 3), dtype=torch.float64, device=dev)
        key = T.exchange_key(seed)
        for i in range(niters):
            s = sweep + i
            self.sweep(view, 1, seed, sweep=s, order=order, beta=beta)
            self.score_joint(out=joint)
            if trace is not None and (i + 1) % trace_every == 0:
                trace[:, (i + 1) // trace_every - 1, :].copy_(self.z)
                rungs[:, (i + 1) // trace_every - 1].copy_(rung)
            self.exchange(joint, beta, rung, R, parity=s, seed=key, sweep=s, counters=(proposed, accepted))
        if zmatrix is not None and trace.shape[1] > 0:
            cold = T.cold_samples(trace, rungs)
            if cold.shape[0] > 0:
                zmatrix.add(cold)
        return T.TemperedResult(trace=trace, rungs=rungs, beta=beta, rung=rung, proposed=proposed, accepted=accepted,
                                joint=joint)

    def ais(self, view, betas, seed, sweeps_per_temp=1, order=None, sweep=0):
        """Annealed importance sampling (Neal 2001), the chains as independent runs -> tempering.AISResult, whose
        log_evidence estimates log p(X | hp, alpha) -- a second unbiased estimator beside smc().

        betas: a non-decreasing host array of T temperatures with betas[0] == 0 and betas[-1] == 1 (as float32, what the
        device sees); anything else is a ValueError before the device is touched.  The steps: seat(view), which zeroes
        ens.logw; one sweep at beta = 0 with counter `sweep`, a draw from the CRP prior; then for t = 1 .. T - 1
        score_joint, anneal_weights(joint, betas[t - 1], betas[t]) and sweeps_per_temp sweeps at betas[t], the counters
        running on from sweep + 1.  One synchronisation, at the end, brings ens.logw to the host; log_evidence =
        smc.log_mean_exp(logw).  exp(log_evidence) is unbiased provided all chains share hyper-parameters and alpha (see
        smc()).
        result.truncated: True when some chain had all ngroups slots occupied at the END of some sweep (the occupied
        counts of sweep(want_occupied=True), reduced on the device): a new group may have been refused there, and the
        estimate is for the mixture truncated to ngroups slots.  It is an end-of-sweep check: a chain that filled every
        slot within a sweep and emptied one again before its end is not seen."""
        b = T.ais_betas(betas)
        self._check_open()
        spt = int(sweeps_per_temp)
        if spt < 0:
            raise ValueError("sweeps_per_temp must be >= 0")
        seeds = chain_seeds(seed, self.nchains)
        dev = self.ctx.torch_device
        self.seat(view)
        joint = torch.empty((self.nchains, len(self.features) + 3), dtype=torch.float64, device=dev)
        full = torch.zeros((), dtype=torch.bool, device=dev)
        counter = [int(sweep)]

        def at(value):
            return torch.full((self.nchains,), float(value), dtype=torch.float32, device=dev)

        def one_sweep(beta):
            _, occupied = self.sweep(view, 1, seeds, sweep=counter[0], order=order, want_occupied=True, beta=beta)
            if occupied.numel() and int(view.nrows):          # (no row, no visit: nothing was written)
                full.logical_or_((occupied >= self.K).any())
            counter[0] += 1

        one_sweep(at(b[0]))
        for t in range(1, len(b)):
            self.score_joint(out=joint)
            now = at(b[t])
            self.anneal_weights(joint, at(b[t - 1]), now)
            for _ in range(spt):
                one_sweep(now)
        down = torch.cat([self.logw, full.to(torch.float64).reshape(1)]).cpu().numpy()      # the one synchronisation
        logw, truncated = down[:-1].copy(), bool(down[-1] != 0.0)
        return T.AISResult(log_evidence=S.log_mean_exp(logw), log_weights=logw, weights=S.normalised_weights(logw),
                           ess=S.ess(logw), truncated=truncated)

    # the posterior-averaged row predictive density ---------------------------------
    def _feature_list(self, what, feats):
        """a sorted list of distinct feature indices of the states"""
        out = sorted(int(f) for f in feats)
        for i, f in enumerate(out):
            if not 0 <= f < len(self.features):
                raise ValueError("%s: feature %d outside the states (%d features)" % (what, f, len(self.features)))
            if i and f == out[i - 1]:
                raise ValueError("%s names feature %d twice" % (what, f))
        return out

    def predictive_logp(self, view, weights=None, features=None, given=None, per_chain=False, row0=0, nrows=None,
                        cols=None, out=None):
        """log p(x_r | data) ~ log sum_c w_c p(x_r | state_c) of rows [row0, row0 + nrows) of the view, averaged over
        the chains in one pass (msc_chains_score_marginal; asynchronous) -> mix, a float32 device tensor [nrows]; with
        per_chain -> (mix, chain_logp), chain_logp float32 [nchains, nrows] holding what ens.states[c].predictive_logp
        defines for each chain.  The sum over the chains is taken in double in a fixed order: a call repeats its bits,
        and a call over a sub-range gives the whole call's.
        weights: None (equal), or float64 [nchains] LOG weights on the host or the device, normalised or not; -inf
        leaves a chain out.  ens.logw after ens.smc(...) is the intended argument.
        features=[f, ...]: only these features' entries are scored (default: all).
        given=[f, ...]: -> mix(the selected features) - mix(given), the model-averaged CONDITIONAL log density of the
        other selected entries given those of `given` (two calls of the entry point).  This is the ratio of two averages
        over the chains -- log (sum_c w_c p_c(all)) / (sum_c w_c p_c(given)) -- not an average of per-chain ratios:
        the chains that explain the given entries well count for more, as they should.  chain_logp stays the per-chain
        log density of ALL selected entries.  given must be a subset of the selected features.
        out: a float32 device tensor of at least nrows entries that receives mix."""
        self._check_open()
        dev = self.ctx.torch_device
        row0, n = A.rows(int(view.nrows), row0, nrows)
        if row0 + n > view.nrows:                      # (outputs are sized before the call: not left to the library)
            raise ValueError("rows [%d, %d) outside the view (%d rows)" % (row0, row0 + n, view.nrows))
        sel = None
        if features is not None:
            sel = self._feature_list("features", features)
            if not sel:
                raise ValueError("features must name at least one feature (None: all)")
        giv = None
        if given is not None:
            giv = self._feature_list("given", given)
            if not set(giv) <= set(range(len(self.features)) if sel is None else sel):
                raise ValueError("given must be a subset of the selected features")
        w = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
            if w.dtype != torch.float64 or tuple(w.shape) != (self.nchains,):
                raise ValueError("weights must be float64 [nchains = %d] log weights" % self.nchains)
        if out is not None:
            A.flat(out, torch.float32, n, dev, "out")
        # every argument is checked: from here on the device is used
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=dev)
        op = A.ptr(out)
        wp = None
        if w is not None:
            w = w.to(dev).contiguous()
            wp = A.ptr(w)
        logp = torch.empty((self.nchains, n), dtype=torch.float32, device=dev) if per_chain else None
        for st in self.states:
            st._bound_view = view        # (the library keeps no reference to a view: the states do, for the last one bound)
        cp = self.states[0]._cols(cols)

        def call(feats, mix_ptr, logp_t):
            fa = (C.c_uint32 * len(feats))(*feats) if feats else None
            L.check(self.ctx.lib.msc_chains_score_marginal(
                self._h, view._h, cp, row0, n, fa, len(feats) if feats else 0, wp, 0, mix_ptr,
                A.ptr(logp_t) if logp_t is not None and logp_t.numel() else None, n))

        if n:
            call(sel, op, logp)
            if giv:
                denom = torch.empty(n, dtype=torch.float32, device=dev)
                call(giv, A.ptr(denom), None)
                out[:n] -= denom
        return (out, logp) if per_chain else out

    # posterior predictive draws from the model average --------------------------------
    def sample_predictive(self, view, weights=None, seed=0, sweep=0, masked_only=False, features=None, row0=0, nrows=None,
                          row_id0=None, cols=None, out=None):
        """Posterior predictive draws for rows [row0, row0 + nrows) of the view from the MODEL AVERAGE over the chains, in
        one pass (msc_chains_sample_predictive; asynchronous): every row draws a chain with probability ~ w_c p(the row's
        observed entries | state_c), a group of that chain, and its entries from that group's predictive
        -> (dict feature -> device tensor of nrows values, chains int32 [nrows], groups int32 [nrows]).
        A row no chain of finite weight can hold is skipped: chains = groups = -1 and its entries keep what `out` held.
        weights: None (equal), or float64 [nchains] LOG weights on the host or the device, normalised or not; -inf leaves a
        chain out.  ens.logw after ens.smc(...) is the intended argument.
        features: state feature indices to draw (default: every feature but the noop ones, which have no values; whatever
        is drawn, a row's chain and group are conditioned on all its observed entries).  out: optional
        dict feature -> device tensor to write into.
        Every drawn entry is, bit for bit, what ens.states[c].sample_predictive(view, z=groups, seed, sweep, ...) writes
        for the rows with chains == c.  The draws are a fixed function of (seed, sweep, row_id0 + row): a call repeats its
        bits and a call over a sub-range gives the whole call's; m independent draws of every row -- m imputations of a
        data set -- are m calls with sweep = 0 .. m - 1."""
        self._check_open()
        dev = self.ctx.torch_device
        row0, n = A.rows(int(view.nrows), row0, nrows)
        if row0 + n > view.nrows:                      # (outputs are sized before the call: not left to the library)
            raise ValueError("rows [%d, %d) outside the view (%d rows)" % (row0, row0 + n, view.nrows))
        dtypes = State._PRED_DTYPES
        feats = [f for f, (fam, _) in enumerate(self.features) if fam in dtypes] if features is None else [int(f) for f in features]
        for f in feats:
            if not 0 <= f < len(self.features):
                raise ValueError("feature %d outside the states (%d features)" % (f, len(self.features)))
            if self.features[f][0] not in dtypes:
                raise L.MicroscopesHipError(-4, "feature %d: the family has no values to draw" % f)
        w = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
            if w.dtype != torch.float64 or tuple(w.shape) != (self.nchains,):
                raise ValueError("weights must be float64 [nchains = %d] log weights" % self.nchains)
        seed, sweep = int(seed), int(sweep)
        if not 0 <= seed <= _U64 or not 0 <= sweep <= _U64:
            raise ValueError("seed and sweep must lie in [0, 2^64)")
        out = dict(out or {})
        for f in feats:
            t = out.get(f)
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (n,)):
                raise ValueError("out[%d] must be a contiguous %s device tensor of shape %s" % (f, dtypes[self.features[f][0]], (n,)))
            if t is not None:
                A.flat(t, dtypes[self.features[f][0]], 0, dev, "out[%d]" % f)
        # every argument is checked: from here on the device is used
        ptrs = (C.c_void_p * len(self.features))()
        for f in feats:
            if out.get(f) is None:
                out[f] = torch.empty((n,), dtype=dtypes[self.features[f][0]], device=dev)
            ptrs[f] = A.ptr(out[f]) if n else None
        chains = torch.full((n,), -1, dtype=torch.int32, device=dev)
        groups = torch.full((n,), -1, dtype=torch.int32, device=dev)
        wp = None
        if w is not None:
            w = w.to(dev).contiguous()
            wp = A.ptr(w)
        for st in self.states:
            st._bound_view = view        # (the library keeps no reference to a view: the states do, for the last one bound)
        L.check(self.ctx.lib.msc_chains_sample_predictive(
            self._h, view._h, self.states[0]._cols(cols), row0, n, row0 if row_id0 is None else int(row_id0), wp,
            L.PRED_MASKED_ONLY if masked_only else 0, seed, sweep, A.ptr(chains) if n else None,
            A.ptr(groups) if n else None, ptrs))
        return {f: out[f] for f in feats}, chains, groups

    def impute(self, view, **kw):
        """sample_predictive with masked_only=True: masked entries drawn, observed ones copied (the completed columns).
        m imputations of the data set are m calls with sweep = 0 .. m - 1."""
        return self.sample_predictive(view, masked_only=True, **kw)

    # lifetime -----------------------------------------------------------------
    def _check_open(self):
        if not getattr(self, "_h", None):
            raise ValueError("ChainEnsemble is closed")

    def close(self):
        """the handle first (a member state cannot be destroyed while it lives), then the states"""
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self.ctx.lib.msc_chains_destroy(self._h)
            self._h = None
        for st in getattr(self, "states", ()):
            st.close()
        self.states = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def joint_tracker_args(every, keep_best):
    """the argument checks of JointTracker that need no device -> (every, keep_best)"""
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError("every must be an int >= 1")
    if not isinstance(keep_best, (bool, np.bool_)):
        raise ValueError("keep_best must be True or False")
    return int(every), bool(keep_best)


class JointTracker(object):
    """The trace of every chain's log joint over the iterations of ChainEnsemble.run(..., joint=tracker), and every
    chain's best sample so far, all on the device: nothing is copied to the host and nothing waits until a result is read.

    every: a sample after each every-th iteration, counted over all the runs the tracker sees.  keep_best: keep each
    chain's highest-scoring z (msc_chains_keep_best: strictly greater wins, so the first of equal maxima stays; NaN never
    wins).  priors: ChainEnsemble.score_joint's -- with them the total is log p(X, z, hp, alpha) up to the flat priors.
      joint       float64 device tensor [nchains, samples, nfeatures + 3], ChainEnsemble.score_joint's rows
      best_joint  float64 [nchains], -inf until a sample has been kept
      best_z      int32 [nchains, nrows]
      best_iter   int64 [nchains], the iteration (run's sweep + i numbering) of the best sample, -1 until one is kept
    A tracker persists across run calls: a run that continues the numbering continues the trace and keeps an earlier
    best that it does not beat."""

    def __init__(self, ens, every=1, keep_best=True, priors=None):
        self.every, self.keep_best = joint_tracker_args(every, keep_best)
        if not isinstance(ens, ChainEnsemble):
            raise ValueError("ens must be a ChainEnsemble")
        State._joint_priors(priors)                       # (checked here, built at every call)
        self.ens, self.priors = ens, priors
        self.nsamples, self._seen = 0, 0
        self._buf = self._best = self._best_z = self._best_iter = None

    def _state(self):
        """the device tensors, made when first needed (best_z needs the assignment's rows)"""
        if self._best is None:
            ens = self.ens
            ens._check_open()
            if ens.z is None:
                raise ValueError("no assignment yet: call assign() or seat() on the ensemble first")
            dev = ens.ctx.torch_device
            self._buf = torch.empty((ens.nchains, 0, len(ens.features) + 3), dtype=torch.float64, device=dev)
            self._best = torch.full((ens.nchains,), float("-inf"), dtype=torch.float64, device=dev)
            self._best_z = torch.full((ens.nchains, int(ens.z.shape[1])), -1, dtype=torch.int32, device=dev)
            self._best_iter = torch.full((ens.nchains,), -1, dtype=torch.int64, device=dev)
        return self

    joint = property(lambda self: self._state()._buf[:, :self.nsamples])
    best_joint = property(lambda self: self._state()._best)
    best_z = property(lambda self: self._state()._best_z)
    best_iter = property(lambda self: self._state()._best_iter)

    def _iteration(self, it, left):
        """run's hook at the end of iteration number `it`, `left` iterations of the run still to come (this one
        included): room for their samples is made at once, so a run grows the trace at most once"""
        self._seen += 1
        if self._seen % self.every:
            return
        self._state()
        ens = self.ens
        if self.nsamples == self._buf.shape[1]:
            room = max(1, (self._seen - 1 + int(left)) // self.every - (self._seen // self.every - 1))
            grown = torch.empty((ens.nchains, self.nsamples + room, self._buf.shape[2]), dtype=torch.float64,
                                device=self._buf.device)
            grown[:, :self.nsamples].copy_(self._buf[:, :self.nsamples])
            self._buf = grown
        row = self._buf[:, self.nsamples]
        ens.score_joint(priors=self.priors, out=row)
        if self.keep_best:
            z = ens.z
            L.check(ens.ctx.lib.msc_chains_keep_best(ens._h, A.ptr(row), int(self._buf.stride(0)), A.ptr(z), int(z.stride(0)),
                                                     int(z.shape[1]), int(it), A.ptr(self._best), A.ptr(self._best_z),
                                                     int(self._best_z.stride(0)), A.ptr(self._best_iter)))
        self.nsamples += 1

    def totals(self):
        """the totals' trace as a host array [nchains, samples] (one synchronisation)"""
        return self.joint[:, :, 0].cpu().numpy()

    def map(self):
        """(chain, z row, joint) of the best sample kept over all chains: the MAP sample of the run (one
        synchronisation); z row an int32 device tensor [nrows]"""
        if not self.keep_best:
            raise ValueError("the tracker was made with keep_best=False")
        best = self.best_joint.cpu().numpy()
        kept = self.best_iter.cpu().numpy() >= 0
        if not kept.any():
            raise ValueError("no sample has been kept yet")
        c = int(np.argmax(np.where(kept, best, -np.inf)))
        return c, self.best_z[c], float(best[c])

    def rhat(self):
        """split-R-hat of the totals over the chains (diagnostics.split_rhat)"""
        from . import diagnostics
        return diagnostics.split_rhat(self.totals())

    def ess(self):
        """effective sample size of the totals over the chains (diagnostics.ess)"""
        from . import diagnostics
        return diagnostics.ess(self.totals())


def _create(ctx, states):
    hs = (C.c_void_p * len(states))(*[st._h.value for st in states])
    h = C.c_void_p()
    L.check(ctx.lib.msc_chains_create(hs, len(states), C.byref(h)))
    return h
