"""Posterior summaries of assignment samples: the interface of the reference's ``microscopes.common.query``.

``groups``, ``zmatrix``, ``zmatrix_reorder`` and ``zmatrix_heuristic_block_ordering`` take the same arguments, return the
same values and raise the same ``ValueError``s.  Numpy input runs a vectorised numpy path.  Device tensors (or numpy input
with ``ctx=``) build the z-matrix on the device (``ZMatrix``, ``msc_zmatrix_*``) and return a device tensor bit-equal to
the numpy path.  The block ordering is the leaf order of scipy's single linkage over the condensed upper triangle: scipy
itself for numpy input, ``msc_linkage_single`` for a float32 device tensor (the same dendrogram, bit for bit).
``zmatrix_linkage`` returns that dendrogram and ``zmatrix_clusters`` cuts a consensus partition out of it; the reference
exposes neither.  ``partition_sums``, ``partition_loss`` and ``point_estimate`` choose ONE clustering by posterior expected
loss (Binder's loss, which is Dahl's least-squares clustering, or the variation-of-information lower bound of Wade and
Ghahramani) among candidate partitions, from exact integer sums over the co-clustering counts: numpy on the host,
``msc_zmatrix_partition_*`` on the device, the same integers on both.  ``refine_partition`` takes partitions further by
greedy row moves under Binder's loss until no single move helps (``msc_zmatrix_partition_refine`` on the device, plain
numpy on the host, the same trajectory bit for bit), and ``point_estimate(refine=...)`` refines the best candidates.
``refine_partition_vi`` and ``vi_estimate(refine=...)`` do the same under the exact expected variation of information,
with integer gains from a fixed-point table of n log2 n (``vi_table``, ``msc_partition_refine_vi``).
``partition_distances`` is what the counts cannot give: Binder's distance and the variation of information between every
partition of one set and every partition of another (``msc_partition_distances`` on the device, ``np.unique`` and a
contingency table per pair on the host, the same integers on both).  ``adjusted_rand``, ``expected_loss`` (the EXACT
posterior expected VI of candidates, where ``partition_loss`` has a bound), ``vi_estimate`` and ``credible_ball`` (Wade and
Ghahramani's credible ball around an estimate) are built on it; they take the samples themselves.
"""
import math
import collections

import numpy as np
import torch

from . import _lib
from ._lib import (DISTANCES_MAX_CLUSTERS, LINKAGE_MAX_N, REFINE_VI_MAX_CLUSTERS, VI_TABLE_SCALE, ZMATRIX_MAX_LABELS,
                   ZMATRIX_REFINE_MAX_CLUSTERS)
from .runtime import Context, ZMatrix

_HOST_CHUNK_FLOATS = 1 << 23      # one-hot block of the numpy path: at most 64 MiB of float64


def groups(avec, sort=False):
    """The clustering of one assignment vector: a list of lists of row indices, one per distinct label, in the order the
    labels first appear (``sort``: by descending size, ties in that order)."""
    a = np.asarray(avec.cpu() if isinstance(avec, torch.Tensor) else avec)
    if a.size == 0:
        return []
    a = a.reshape(-1)
    _, first, inv = np.unique(a, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    rows = np.argsort(inv, kind="stable")              # rows of each label, ascending, label after label
    sizes = np.bincount(inv, minlength=first.size)
    parts = np.split(rows, np.cumsum(sizes)[:-1])
    by_appearance = np.argsort(first, kind="stable")
    if sort:
        by_appearance = by_appearance[np.argsort(-sizes[by_appearance], kind="stable")]
    return [parts[k].tolist() for k in by_appearance]


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def _check_assignments(assignments):
    if not len(assignments):
        raise ValueError("empty assignments list")
    if len(set(len(a) for a in assignments)) != 1:
        raise ValueError("assignment vectors should all be same size")


def _dense_labels(a):
    """[S, n] of any labels -> the same partitions with labels in [0, K) per sample, and K"""
    out = np.empty(a.shape, dtype=np.int32)
    K = 1
    for s in range(a.shape[0]):
        u, inv = np.unique(a[s], return_inverse=True)
        out[s] = inv.reshape(-1)
        K = max(K, u.size)
    return out, K


def _counts_host(a):
    """float64 [n, n] co-clustering counts: sums of one-hot products (exact in float64), a block of samples at a time"""
    S, n = a.shape
    dense, K = _dense_labels(a)
    counts = np.zeros((n, n), dtype=np.float64)
    step = max(1, _HOST_CHUNK_FLOATS // max(1, n * K))
    eye = np.eye(K, dtype=np.float64)
    for s0 in range(0, S, step):
        blk = dense[s0:s0 + step]
        H = eye[blk].transpose(1, 0, 2).reshape(n, -1)   # [n, samples x K]: row i's label of each sample, one-hot
        counts += H @ H.T
    return counts


def _zmatrix_host(a):
    """float32 count / S"""
    return _counts_host(a).astype(np.float32) / np.float32(a.shape[0])


def _open_zmatrix(a, ctx):
    """a: int32 device tensor [S, n] -> (an accumulator holding the samples, the samples as it took them)"""
    S, n = int(a.shape[0]), int(a.shape[1])
    lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= ZMATRIX_MAX_LABELS:
        a = torch.stack([torch.unique(a[s], return_inverse=True)[1] for s in range(S)]).to(torch.int32)
        hi = int(a.max())
    a = a.contiguous()
    zm = ZMatrix(ctx, n, hi + 1)
    try:
        zm.add(a)
    except Exception:
        zm.close()
        raise
    return zm, a


def _zmatrix_device(a, ctx):
    """a: int32 device tensor [S, n]"""
    zm, _ = _open_zmatrix(a, ctx)
    try:
        return zm.result()
    finally:
        zm.close()


def _host_samples(assignments):
    a = np.asarray([np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in assignments])
    return a.reshape(len(assignments), -1)


def _on_device(assignments, ctx):
    return ctx is not None or _is_device(assignments) or \
        (not isinstance(assignments, (np.ndarray, torch.Tensor)) and any(_is_device(a) for a in assignments))


def _device_samples(assignments, ctx):
    """(int32 device tensor [S, n], context) of assignment vectors given as zmatrix takes them"""
    if ctx is None:
        dev = assignments.device if isinstance(assignments, torch.Tensor) else \
            next(a.device for a in assignments if _is_device(a))
        ctx = Context(device=dev.index if dev.index is not None else torch.cuda.current_device())
    if isinstance(assignments, torch.Tensor):
        a = assignments.to(device=ctx.torch_device)
    else:
        rows = []
        for v in assignments:
            if isinstance(v, torch.Tensor):
                rows.append(v.to(device=ctx.torch_device).reshape(-1))
            else:
                rows.append(torch.from_numpy(np.asarray(v).reshape(-1).astype(np.int64)).to(ctx.torch_device))
        a = torch.stack([r.to(torch.int64) for r in rows])
    if a.dtype.is_floating_point or a.dtype == torch.bool:
        raise ValueError("assignment vectors must hold integer labels")
    if a.dtype != torch.int32:
        a64 = a.to(torch.int64)
        if int(a64.min()) < 0 or int(a64.max()) >= ZMATRIX_MAX_LABELS:
            a64 = torch.stack([torch.unique(a64[s], return_inverse=True)[1] for s in range(a64.shape[0])])
        a = a64.to(torch.int32)
    return a.reshape(a.shape[0], -1), ctx


def zmatrix(assignments, ctx=None):
    """Z[i, j] = the fraction of the assignment vectors in which rows i and j share a label (float32 [n, n]).

    ``assignments``: a list (or [S, n] array) of assignment vectors of equal length.  Numpy input returns a numpy array;
    a device tensor, a list of device tensors, or any input with ``ctx`` (a ``Context``) runs on the device and returns a
    float32 device tensor with the same bits."""
    _check_assignments(assignments)
    if not _on_device(assignments, ctx):
        return _zmatrix_host(_host_samples(assignments))
    return _zmatrix_device(*_device_samples(assignments, ctx))


def _is_square(z):
    return len(z.shape) == 2 and z.shape[0] == z.shape[1]


def _is_permutation(pi, n):
    if len(pi.shape) != 1 or pi.shape[0] != n:
        return False
    if not np.issubdtype(pi.dtype, np.integer):
        return False
    return np.unique(pi).size == n


def zmatrix_reorder(zmat, order):
    """zmat with rows and columns permuted by ``order``: out[a, b] = zmat[order[a], order[b]].  A device tensor stays on
    the device."""
    o = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order)
    if not _is_square(zmat):
        raise ValueError("not a zmatrix")
    if not _is_permutation(o, zmat.shape[0]):
        raise ValueError("not a valid permutation")
    if isinstance(zmat, torch.Tensor):
        idx = torch.from_numpy(o.astype(np.int64)).to(zmat.device)
        return zmat.index_select(0, idx).index_select(1, idx)
    zmat = np.asarray(zmat)
    return zmat[o][:, o]


_NONFINITE = "The condensed distance matrix must contain only finite values."     # scipy's linkage says so
_contexts = {}


def _context_of(zmat, ctx):
    """the caller's context, or one kept per device that follows torch's current stream"""
    if ctx is not None:
        return ctx
    index = zmat.device.index if zmat.device.index is not None else torch.cuda.current_device()
    c = _contexts.get(index)
    if c is None or not getattr(c, "_h", None):
        c = _contexts[index] = Context(device=index)
    else:
        c.set_stream(torch.cuda.current_stream(index))
    return c


def _device_linkage(zmat, ctx, linkage, order):
    """(linkage, order) of a float32 device tensor by msc_linkage_single, or None where the tensor goes the host way.
    The reference looks at the strict upper triangle alone; the kernel reads whole rows of a symmetric matrix, so a
    tensor that is not symmetric is replaced by the mirror image of its upper triangle."""
    if not (_is_device(zmat) and zmat.dtype == torch.float32):
        return None
    n = int(zmat.shape[0])
    if n < 2 or n > LINKAGE_MAX_N:
        return None
    ctx = _context_of(zmat, ctx)
    z = zmat.to(ctx.torch_device)
    if not (bool(torch.isfinite(z).all()) and torch.equal(z, z.T)):
        upper = torch.triu(z, diagonal=1)            # (zeros elsewhere, whatever was there)
        if not bool(torch.isfinite(upper).all()):
            raise ValueError(_NONFINITE)
        z = upper + upper.T
        del upper
    if z.stride(1) != 1 or z.stride(0) < n:
        z = z.contiguous()
    return ctx.linkage_single(z, linkage=linkage, order=order)


def _condensed_distances(zmat):
    z = np.asarray(zmat.cpu() if isinstance(zmat, torch.Tensor) else zmat)
    return 1. - np.array(z[np.triu_indices(z.shape[0], k=1)])


def zmatrix_linkage(zmat, ctx=None):
    """scipy's single linkage of the distances 1 - Z over the condensed upper triangle: the float64 [n - 1, 4] matrix
    ``scipy.cluster.hierarchy.linkage(1. - zmat[np.triu_indices(n, 1)])`` returns.  A float32 device tensor of 2 <= n <=
    65536 rows is linked on the device (msc_linkage_single: the same matrix, bit for bit); a view with contiguous rows
    is read in place.  Everything else takes scipy on the host."""
    import scipy.cluster.hierarchy as hier
    if not _is_square(zmat):
        raise ValueError("not a zmat")
    got = _device_linkage(zmat, ctx, True, False)
    if got is not None:
        return got[0]
    return hier.linkage(_condensed_distances(zmat))


def zmatrix_heuristic_block_ordering(zmat, ctx=None):
    """A permutation of the rows that puts co-clustered rows next to each other: the leaves of scipy's single linkage of
    the distances 1 - Z over the condensed upper triangle.  A float32 device tensor stays on the device (see
    ``zmatrix_linkage``); the permutation is a numpy array either way."""
    import scipy.cluster.hierarchy as hier
    if not _is_square(zmat):
        raise ValueError("not a zmat")
    got = _device_linkage(zmat, ctx, True, True)
    if got is not None:
        if (got[0][:, 2] < 0).any():                  # (an entry above 1: scipy's leaves_list refuses such a linkage)
            raise ValueError("Linkage 'Z' contains negative distances.")
        return got[1]
    return np.array(hier.leaves_list(hier.linkage(_condensed_distances(zmat))))


def zmatrix_clusters(zmat, threshold, ctx=None):
    """The consensus partition at ``threshold``: rows i and j share a label when a chain of pairs with Z >= threshold
    (1 - Z <= 1 - threshold) leads from one to the other -- the single linkage cut at the distance 1 - threshold,
    ``fcluster(zmatrix_linkage(zmat), 1 - threshold, 'distance')`` as a partition.  Returns an integer array of n labels,
    numbered from 0 in the order of their first row."""
    import scipy.cluster.hierarchy as hier
    flat = hier.fcluster(zmatrix_linkage(zmat, ctx=ctx), 1. - threshold, criterion="distance")
    _, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inv.reshape(-1)]


# ---- one clustering out of the samples: posterior expected loss of candidate partitions ----------------------------
PointEstimate = collections.namedtuple("PointEstimate", ["labels", "index", "losses", "confidence"])
_LOSSES = ("binder", "vi")


def _renumber(labels):
    """the same partition, numbered from 0 in the order of each label's first row (as zmatrix_clusters numbers)"""
    _, first, inv = np.unique(np.asarray(labels), return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inv.reshape(-1)]


def _host_candidates(candidates, n):
    c = np.asarray(candidates.cpu() if isinstance(candidates, torch.Tensor) else candidates)
    if c.ndim == 1:
        c = c.reshape(1, -1)
    if c.ndim != 2 or c.shape[0] == 0:
        raise ValueError("empty candidates list")
    if c.shape[1] != n:
        raise ValueError("candidate vectors should be the size of the assignment vectors")
    if not np.issubdtype(c.dtype, np.integer):
        raise ValueError("candidate vectors must hold integer labels")
    return c


def _sums_of_counts(C, c):
    """C: int64 [m, m] counts; c: [ncand, m] labels -> (w int64 [ncand, m], size int32 [ncand, m])"""
    nc, m = c.shape
    w = np.empty((nc, m), dtype=np.int64)
    size = np.empty((nc, m), dtype=np.int32)
    for k in range(nc):
        _, inv = np.unique(c[k], return_inverse=True)
        inv = inv.reshape(-1)
        by_label = np.argsort(inv, kind="stable")
        sizes = np.bincount(inv)
        starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
        per_label = np.add.reduceat(C[:, by_label], starts, axis=1)     # [m, labels]: row a's counts over each cluster
        w[k] = per_label[np.arange(m), inv]
        size[k] = sizes[inv]
    return w, size


def _loss_of_sums(C, w, size):
    """(binder_num int64 [ncand], vi_lb float64 [ncand], V) by the definitions of msc_zmatrix_partition_loss"""
    m = C.shape[0]
    V = int(C[0, 0])
    T = (int(C.sum()) - int(np.trace(C))) // 2
    P = (size.astype(np.int64) - 1).sum(axis=1) // 2
    Q2 = (w - V).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        vi = (np.log2(size.astype(np.float64)) - 2. * np.log2(w.astype(np.float64))).sum(axis=1) / m + 2. * np.log2(float(V))
    return T + V * P - Q2, vi, V


def _host_counts_of(assignments):
    _check_assignments(assignments)
    a = _host_samples(assignments)
    return a, np.rint(_counts_host(a)).astype(np.int64)


def partition_sums(assignments, candidates):
    """The integer sums behind both losses, on the host (the yardstick of ``ZMatrix.partition_sums``).  With C the
    co-clustering counts of the assignment vectors, for every candidate c and row a: ``size[c, a]`` = the rows that c puts
    with a (a itself included), ``w[c, a]`` = the sum of C[a, b] over those rows.  Only equality of labels is used.
    Returns ``(w int64 [ncand, n], size int32 [ncand, n])``."""
    a, C = _host_counts_of(assignments)
    return _sums_of_counts(C, _host_candidates(candidates, a.shape[1]))


def _device_candidates(candidates, ctx, n):
    """an int32 tensor [ncand, n] on the context's device; labels that do not fit an int32 are renumbered row by row"""
    if isinstance(candidates, torch.Tensor):
        c = candidates.to(ctx.torch_device)
        if c.dtype.is_floating_point or c.dtype == torch.bool:
            raise ValueError("candidate vectors must hold integer labels")
        c = c.reshape(1, -1) if c.dim() == 1 else c
        if c.dim() != 2 or c.shape[0] == 0:
            raise ValueError("empty candidates list")
        if c.shape[1] != n:
            raise ValueError("candidate vectors should be the size of the assignment vectors")
        if c.dtype != torch.int32:
            c64 = c.to(torch.int64)
            if int(c64.min()) < -2 ** 31 or int(c64.max()) >= 2 ** 31:
                c64 = torch.stack([torch.unique(c64[k], return_inverse=True)[1] for k in range(c64.shape[0])])
            c = c64.to(torch.int32)
        return c.contiguous()
    if not isinstance(candidates, np.ndarray):
        candidates = [np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in candidates]
    c = _host_candidates(candidates, n)
    if c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31):
        c = _dense_labels(c)[0]
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(ctx.torch_device)


class _Scorer(object):
    """candidates against one set of samples, on the host (C: int64 counts) or on the device (zm: a ZMatrix)"""

    def __init__(self, assignments, ctx):
        self.zm = self.C = self.samples = None
        self.owned = False
        if isinstance(assignments, ZMatrix):
            if ctx is not None and ctx is not assignments.ctx:
                raise ValueError("ctx is not the accumulator's context")
            self.zm, self.n = assignments, assignments.n
            return
        _check_assignments(assignments)
        if _on_device(assignments, ctx):
            a, ctx = _device_samples(assignments, ctx)
            self.zm, self.samples = _open_zmatrix(a, ctx)
            self.owned, self.n = True, self.zm.n
        else:
            self.samples, self.C = _host_counts_of(assignments)
            self.n = self.samples.shape[1]

    def candidates(self, candidates):
        if candidates is None:
            if self.samples is None:
                raise ValueError("an accumulator keeps no samples: candidates must be given")
            return self.samples
        if self.zm is not None:
            return _device_candidates(candidates, self.zm.ctx, self.n)
        return _host_candidates(candidates, self.n)

    def loss(self, c):
        if self.zm is not None:
            return self.zm.partition_loss(c)
        return _loss_of_sums(self.C, *_sums_of_counts(self.C, c))

    def sums(self, c):
        """(w, size) as numpy arrays"""
        if self.zm is not None:
            w, size = self.zm.partition_sums(c)
            return w.cpu().numpy(), size.cpu().numpy()
        return _sums_of_counts(self.C, c)

    def refine(self, starts, max_sweeps, max_clusters, order):
        """(labels, binder_num, sweeps, moves) of starts given as candidates are"""
        if self.zm is not None:
            return self.zm.partition_refine(starts, max_sweeps, max_clusters, order)
        m = self.C.shape[0]
        return _refine_host(self.C, starts, max_sweeps, m if max_clusters is None else max_clusters, order)

    def sums_of_positions(self, labels):
        """(w, size) as numpy arrays of one partition given over the rows the sums run over"""
        labels = np.asarray(labels).reshape(-1)
        if self.zm is None:
            return _sums_of_counts(self.C, labels[None])
        full = np.zeros(self.n, dtype=np.int32)
        if self.zm._rows is None:
            full[:] = labels
        else:
            rows = self.zm._rows.astype(np.int64)
            full[rows] = labels
            if not np.array_equal(full[rows], labels):
                raise ValueError("a row selected twice ended in two clusters: no vector of n labels holds this partition")
        return self.sums(torch.from_numpy(full).to(self.zm.ctx.torch_device)[None])

    def selected(self, labels):
        """a candidate's labels over the rows the sums run over"""
        labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        if self.zm is not None and self.zm._rows is not None:
            return labels[self.zm._rows.astype(np.int64)]
        return labels

    def close(self):
        if self.owned:
            self.zm.close()


def partition_loss(assignments, candidates, ctx=None):
    """Posterior expected losses of candidate partitions: ``(binder_num int64 [ncand], vi_lb float64 [ncand], valid)``.

    ``binder_num[c] = valid * sum_{a<b} |[c puts a with b] - Z[a, b]|``, an exact integer: ``binder_num / valid`` is the
    expected number of mis-paired pairs under Binder's loss.  Dahl's least-squares criterion ``sum_{a<b} ([..] - Z)^2``
    differs from it by a term that does not depend on the candidate, so both have the same argmin.  ``vi_lb[c] =
    (1 / m) sum_a (log2 size_c[a] - 2 log2 w_c[a]) + 2 log2 valid`` is Wade and Ghahramani's lower bound on the expected
    variation of information less its candidate-independent term ``(1 / m) sum_a E[log2 size_sample(a)]``, which the
    counts do not determine; it is 0 for all singletons.  ``valid`` is the number of samples counted.

    ``assignments`` as for ``zmatrix``, or an open ``ZMatrix`` (the sums then run over its selected rows, the candidates
    are vectors of its n labels).  Numpy input without ``ctx`` runs on the host and returns numpy arrays; device tensors,
    ``ctx=`` or a ``ZMatrix`` run on the device (``msc_zmatrix_partition_loss``) and return device tensors holding the same
    integers."""
    sc = _Scorer(assignments, ctx)
    try:
        return sc.loss(sc.candidates(candidates))
    finally:
        sc.close()


# ---- greedy refinement under Binder's loss ---------------------------------------------------------------------------
RefinedPartitions = collections.namedtuple("RefinedPartitions", ["labels", "binder_num", "sweeps", "moves", "valid"])
_INT64_MIN = np.iinfo(np.int64).min


def _row_sums(C_row, ids, K, exact_in_float):
    """s_k = the sum of C_row over the positions with id k, int64 [K]"""
    if exact_in_float:
        return np.bincount(ids, weights=C_row, minlength=K).astype(np.int64)
    s = np.zeros(K, dtype=np.int64)
    np.add.at(s, ids, C_row)
    return s


def _refine_host(C, starts, max_sweeps, max_clusters, order):
    """The rule of msc_zmatrix_partition_refine (include/microscopes_hip.h) in plain numpy over the int64 counts C:
    starts [nstarts, m] over the positions -> (labels int32 [nstarts, m], binder_num int64, sweeps int32, moves int64)"""
    starts = np.asarray(starts)
    ns, m = starts.shape
    K = int(max_clusters)
    if K < 1 or K > m:
        raise ValueError("max_clusters must lie in [1, m = %d]" % m)
    if int(max_sweeps) < 0:
        raise ValueError("max_sweeps must not be negative")
    visit = np.arange(m) if order is None else np.asarray(order).astype(np.int64)
    if order is not None and not _is_permutation(np.asarray(order), m):
        raise ValueError("not a valid permutation")
    V = int(C[0, 0])
    exact_in_float = V * m < 2 ** 53                   # bincount adds in float64
    Cf = C.astype(np.float64) if exact_in_float else C
    binder0 = _loss_of_sums(C, *_sums_of_counts(C, starts))[0]
    labels = np.empty((ns, m), dtype=np.int32)
    binder = np.empty(ns, dtype=np.int64)
    sweeps = np.zeros(ns, dtype=np.int32)
    moves = np.zeros(ns, dtype=np.int64)
    for i in range(ns):
        ids = _renumber(starts[i]).astype(np.int64)
        if int(ids.max()) + 1 > K:
            raise ValueError("a start holds %d clusters, more than max_clusters = %d" % (int(ids.max()) + 1, K))
        n = np.bincount(ids, minlength=K).astype(np.int64)
        dec = 0
        for _ in range(int(max_sweeps)):
            moved = 0
            for a in visit:
                c = int(ids[a])
                s = _row_sums(Cf[a], ids, K, exact_in_float)
                s[c] -= int(C[a, a])
                n[c] -= 1                              # n' from here on
                g = 2 * s - V * n
                g_cur = int(g[c]) if n[c] > 0 else 0
                k = int(np.argmax(np.where(n > 0, g, _INT64_MIN)))      # the first of the largest: the lowest id
                target, gain = -1, 0
                if n[k] > 0 and int(g[k]) > g_cur:
                    target, gain = k, int(g[k])
                elif n[c] > 0 and 0 > g_cur:
                    free = np.flatnonzero(n == 0)      # (n[c] > 0 here: c is not among them)
                    if free.size:
                        target = int(free[0])
                if target < 0:
                    n[c] += 1
                    continue
                n[target] += 1
                ids[a] = target
                dec += gain - g_cur
                moved += 1
            sweeps[i] += 1
            moves[i] += moved
            if moved == 0:
                break
        labels[i] = _renumber(ids)
        binder[i] = int(binder0[i]) - dec
    return labels, binder, sweeps, moves


def refine_partition(assignments, starts, max_sweeps=20, max_clusters=None, order=None, ctx=None):
    """Partitions taken to a local optimum of Binder's posterior expected loss by greedy row moves.

    From each start, rows are visited in ascending order (or in ``order``, a permutation of the rows scored) and each
    moves to the cluster -- or alone into a new one -- that lowers ``binder_num`` most; a row stays on a tie, and an
    existing cluster is preferred to a new one at equal gain.  Sweeps repeat until one moves nothing or ``max_sweeps``
    have run (include/microscopes_hip.h states the rule in full under msc_zmatrix_partition_refine).  Every move lowers
    ``binder_num`` strictly, so the result is never worse than its start, and a result with ``sweeps < max_sweeps`` is a
    local optimum: no single row move lowers it.  ``max_clusters``: the most clusters a partition may hold on the way
    (``None``: the number of rows scored, at most %d on the device); a start that holds more raises ``ValueError``.

    ``assignments`` and ``starts`` as ``partition_loss`` takes assignments and candidates.  Returns a named tuple
    ``(labels [nstarts, m] int32, numbered from 0 in the order of first row; binder_num int64 [nstarts]; sweeps int32
    [nstarts], the last one that moved nothing included; moves int64 [nstarts]; valid)``.  Numpy input without ``ctx``
    runs the host implementation, plain numpy over the int64 counts; device tensors, ``ctx=`` or an open ``ZMatrix`` run
    ``msc_zmatrix_partition_refine`` and return device tensors holding the same integers, bit for bit.  The
    variation-of-information bound is not refined.""" % ZMATRIX_REFINE_MAX_CLUSTERS
    sc = _Scorer(assignments, ctx)
    try:
        c = sc.candidates(starts)
        if sc.zm is not None:
            out = sc.refine(c, max_sweeps, max_clusters, order)
            sc.zm.ctx.synchronize()
            valid = sc.zm.partition_loss(c[:1])[2]
        else:
            out = sc.refine(c, max_sweeps, max_clusters, order)
            valid = int(sc.C[0, 0])
        return RefinedPartitions(out[0], out[1], out[2], out[3], valid)
    finally:
        sc.close()


def point_estimate(assignments, loss="binder", candidates=None, ctx=None, refine=0, starts=8):
    """ONE clustering out of posterior samples: the candidate of the lowest posterior expected loss.

    ``loss``: ``"binder"`` (Binder's loss: Dahl's least-squares clustering) or ``"vi"`` (the variation-of-information lower
    bound); see ``partition_loss``.  ``candidates``: the partitions to choose among, ``None`` for the samples themselves
    (an open ``ZMatrix`` keeps none, so it needs them).  Runs where ``partition_loss`` would.  Returns a named tuple of
    numpy values: ``labels`` (the winner over the rows scored, numbered from 0 in the order of first row), ``index`` (the
    winner; the lowest index among equal losses), ``losses`` (``binder_num`` int64 or ``vi_lb`` float64 of every
    candidate) and ``confidence`` (float64: ``w[a] / (valid * size[a])``, the mean posterior probability that row a is
    with a row of its own cluster, itself included; in (0, 1]).

    ``refine > 0`` (Binder's loss only; ``"vi"`` raises ``ValueError``): the ``starts`` candidates of lowest loss (ties
    to the lowest index) are each refined by greedy row moves for at most ``refine`` sweeps (``refine_partition``) and
    the best refined partition is returned (ties to the better-ranked start): ``labels`` and ``confidence`` are its own,
    ``index`` is the candidate it grew from, ``losses`` stay the candidates' own."""
    if loss not in _LOSSES:
        raise ValueError("loss must be one of %s" % (_LOSSES,))
    refine, starts = int(refine), int(starts)
    if refine < 0 or starts < 1:
        raise ValueError("refine must not be negative and starts must be at least 1")
    if refine > 0 and loss != "binder":
        raise ValueError("refine > 0 needs loss='binder': the variation-of-information bound is not refined")
    sc = _Scorer(assignments, ctx)
    try:
        c = sc.candidates(candidates)
        binder, vi, valid = sc.loss(c)
        losses = binder if loss == "binder" else vi
        losses = losses.cpu().numpy() if isinstance(losses, torch.Tensor) else np.asarray(losses)
        if refine > 0:
            top = np.argsort(losses, kind="stable")[:starts]
            if isinstance(c, torch.Tensor):
                picked = c[torch.from_numpy(top).to(c.device)]
            else:
                picked = c[top]
            m = sc.zm.m if sc.zm is not None else sc.C.shape[0]
            cap = min(m, ZMATRIX_REFINE_MAX_CLUSTERS) if sc.zm is not None else m
            got = sc.refine(picked, refine, cap, None)
            rb = got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else got[1]
            best = int(np.argmin(rb))
            labels = got[0][best]
            labels = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels
            w, size = sc.sums_of_positions(labels)
            confidence = w[0].astype(np.float64) / (float(valid) * size[0].astype(np.float64))
            return PointEstimate(_renumber(labels), int(top[best]), losses, confidence)
        index = int(np.argmin(losses))
        w, size = sc.sums(c[index:index + 1])
        confidence = w[0].astype(np.float64) / (float(valid) * size[0].astype(np.float64))
        return PointEstimate(_renumber(sc.selected(c[index])), index, losses, confidence)
    finally:
        sc.close()


# ---- distances between partitions: the exact expected VI, credible balls, adjusted Rand ---------------------------------
PartitionDistances = collections.namedtuple("PartitionDistances", ["binder", "vi", "pairs_ab", "nclusters_a", "nclusters_b"])
ExpectedLoss = collections.namedtuple("ExpectedLoss", ["binder_num", "vi", "valid"])
CredibleBall = collections.namedtuple("CredibleBall", ["distances", "radius", "members", "horizontal", "upper", "lower",
                                                       "nclusters"])
_METRICS = ("vi", "binder")
_HOST_TABLE_CELLS = 1 << 16       # a pair's contingency table is a bincount up to this many cells (or 8 m), np.unique beyond


def _host_partitions(p, name="partitions"):
    """an integer array [count, m], neither 0, of partitions given as a vector, a list of vectors or an array"""
    if not isinstance(p, (np.ndarray, torch.Tensor)):
        p = [np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in p]
    p = np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p)
    if p.ndim == 1:
        p = p.reshape(1, -1)
    if p.ndim != 2 or p.shape[0] == 0 or p.shape[1] == 0:
        raise ValueError("empty %s" % name)
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError("%s must hold integer labels" % name)
    return p


def _nlogn(counts):
    """sum n log2 n over positive counts, ascending: the same bits for a pair and for the pair the other way round"""
    c = np.sort(counts).astype(np.float64)
    return float(np.sum(c * np.log2(c)))


def _pairs(counts):
    c = counts.astype(np.int64)
    return int(np.sum(c * (c - 1) // 2))


def _canon_host(p):
    """per partition: (ids int64 [m], K, pairs, nlogn)"""
    out = []
    for row in p:
        u, inv = np.unique(row, return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        sizes = np.bincount(inv, minlength=u.size)
        out.append((inv, int(u.size), _pairs(sizes), _nlogn(sizes)))
    return out


def _sums_host(a, b):
    """the outputs of msc_partition_distances in plain numpy (b None: a against itself); no cap on clusters or rows"""
    ca = _canon_host(a)
    cb = ca if b is None else _canon_host(b)
    m = a.shape[1]
    pairs_ab = np.empty((len(ca), len(cb)), dtype=np.int64)
    nlogn_ab = np.empty((len(ca), len(cb)), dtype=np.float64)
    for i, (ia, ka, _, _) in enumerate(ca):
        for j, (ib, kb, _, _) in enumerate(cb):
            if b is None and j < i:
                pairs_ab[i, j], nlogn_ab[i, j] = pairs_ab[j, i], nlogn_ab[j, i]
                continue
            key = ia * kb + ib
            if ka * kb <= max(_HOST_TABLE_CELLS, 8 * m):
                cells = np.bincount(key, minlength=ka * kb)
                cells = cells[cells > 0]
            else:
                cells = np.unique(key, return_counts=True)[1]
            pairs_ab[i, j], nlogn_ab[i, j] = _pairs(cells), _nlogn(cells)
    per = lambda c: (np.array([x[2] for x in c], dtype=np.int64), np.array([x[3] for x in c], dtype=np.float64),
                     np.array([x[1] for x in c], dtype=np.int32))
    return (pairs_ab, nlogn_ab) + per(ca) + per(cb)


def _distance_sums(a, b, ctx):
    """(the eight outputs of msc_partition_distances, m, on the device?) of partitions given as partition_distances takes
    them"""
    device = ctx is not None or _is_device(a) or _is_device(b) or \
        any(not isinstance(x, (np.ndarray, torch.Tensor)) and x is not None and any(_is_device(v) for v in x) for x in (a, b))
    if not device:
        a = _host_partitions(a)
        if b is not None:
            b = _host_partitions(b)
            if b.shape[1] != a.shape[1]:
                raise ValueError("partitions of different numbers of rows: %d and %d" % (a.shape[1], b.shape[1]))
        return _sums_host(a, b), a.shape[1], False
    if ctx is None:
        first = next(x for x in (a, b) if x is not None and (_is_device(x) or not isinstance(x, (np.ndarray, torch.Tensor))))
        t = first if isinstance(first, torch.Tensor) else next(v for v in first if _is_device(v))
        ctx = _context_of(t, None)
    m = int(a.shape[-1]) if isinstance(a, (np.ndarray, torch.Tensor)) else len(a[0])
    da = _device_candidates(a, ctx, m)
    db = None
    if b is not None:
        mb = int(b.shape[-1]) if isinstance(b, (np.ndarray, torch.Tensor)) else len(b[0])
        if mb != m:
            raise ValueError("partitions of different numbers of rows: %d and %d" % (m, mb))
        db = _device_candidates(b, ctx, m)
    return ctx.partition_distances(da, db), m, True


def _binder_vi(sums, m):
    pairs_ab, nlogn_ab, pairs_a, nlogn_a, _, pairs_b, nlogn_b, _ = sums
    binder = pairs_a[:, None] + pairs_b[None, :] - 2 * pairs_ab
    vi = (nlogn_a[:, None] + nlogn_b[None, :] - 2. * nlogn_ab) / float(m)
    return binder, vi


def partition_distances(a, b=None, ctx=None):
    """Distances between every partition of ``a`` and every partition of ``b`` (``None``: of ``a`` again), all labelling
    the same m rows: vectors, lists of vectors or [count, m] arrays of integer labels; only equality of labels is used.

    With n_ij the contingency counts of a pair, a_i and b_j the cluster sizes and C(n, 2) = n (n - 1) / 2:
    ``pairs_ab = sum C(n_ij, 2)``; ``binder = sum C(a_i, 2) + sum C(b_j, 2) - 2 pairs_ab``, the row pairs that one
    partition joins and the other separates, an exact integer; ``vi = (sum a_i log2 a_i + sum b_j log2 b_j -
    2 sum n_ij log2 n_ij) / m``, the variation of information in bits, a metric, 0 iff the partitions are equal.
    Returns a named tuple ``(binder int64 [na, nb], vi float64 [na, nb], pairs_ab int64 [na, nb], nclusters_a int32 [na],
    nclusters_b int32 [nb])``.

    Numpy input without ``ctx`` runs on the host -- ``np.unique`` per partition and a contingency table per pair, no cap
    on clusters or rows -- and returns numpy arrays.  Device tensors, or ``ctx=``, run ``msc_partition_distances`` (at most
    %d clusters a partition, more raise ``ValueError``; at most 32768 rows) and return device tensors: the same integers,
    ``vi`` within rounding of the host's (the sum of m terms log2 n, each within an ulp)."""
    sums, m, _ = _distance_sums(a, b, ctx)
    binder, vi = _binder_vi(sums, m)
    return PartitionDistances(binder, vi, sums[0], sums[4], sums[7])


partition_distances.__doc__ %= DISTANCES_MAX_CLUSTERS


def adjusted_rand(a, b=None, ctx=None):
    """The adjusted Rand index of every partition of ``a`` against every partition of ``b`` (as ``partition_distances``
    takes them; typically ``b`` is one known labelling): float64 [na, nb], ``(pairs_ab - E) / ((pairs_a + pairs_b) / 2 -
    E)`` with ``E = pairs_a pairs_b / C(m, 2)``, in float64 from the exact integers of ``partition_distances``; 1.0 where
    the denominator is 0 (both partitions all-in-one, or both all singletons).  1 for equal partitions, about 0 for
    independent ones."""
    sums, m, device = _distance_sums(a, b, ctx)
    pairs_ab, pairs_a, pairs_b = sums[0], sums[2], sums[5]
    total = m * (m - 1) // 2
    if device:
        f = lambda x: x.to(torch.float64)
        where, full = torch.where, torch.ones_like(f(pairs_ab))
    else:
        f = lambda x: x.astype(np.float64)
        where, full = np.where, np.ones(pairs_ab.shape, dtype=np.float64)
    pa, pb = f(pairs_a)[:, None], f(pairs_b)[None, :]
    E = pa * pb / float(total) if total > 0 else 0. * pa * pb
    den = (pa + pb) / 2. - E
    safe = where(den == 0, full, den)
    return where(den == 0, full, (f(pairs_ab) - E) / safe)


def _samples_for_distances(assignments, ctx):
    """(samples [S, m], the context or None) of assignment vectors given as zmatrix takes them"""
    if isinstance(assignments, ZMatrix):
        raise ValueError("a ZMatrix keeps counts, not samples: the exact expected losses need the assignment vectors")
    _check_assignments(assignments)
    if _on_device(assignments, ctx):
        if ctx is None:
            t = assignments if isinstance(assignments, torch.Tensor) else next(a for a in assignments if _is_device(a))
            ctx = _context_of(t, None)
        return _device_samples(assignments, ctx)
    a = _host_samples(assignments)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("assignment vectors must hold integer labels")
    return a, None


def _expected(samples, cands, ctx):
    """ExpectedLoss of candidates against samples, both already where they run"""
    S = int(samples.shape[0])
    d = partition_distances(cands, None if cands is samples else samples, ctx=ctx)
    if ctx is None:
        return ExpectedLoss(d.binder.sum(axis=1), np.cumsum(d.vi, axis=1)[:, -1] / float(S), S)
    # the sum over the samples in sample order, as the host adds: a running sum in float64 (a device scan has its own tree)
    vi = np.cumsum(d.vi.cpu().numpy(), axis=1)[:, -1] / float(S)
    return ExpectedLoss(d.binder.sum(dim=1), torch.from_numpy(vi).to(d.vi.device), S)


def expected_loss(assignments, candidates=None, ctx=None):
    """The EXACT posterior expected losses of candidate partitions, from the samples themselves: a named tuple
    ``(binder_num int64 [ncand], vi float64 [ncand], valid)``.

    ``binder_num[c] = sum_s binder(c, s)`` -- the integer ``partition_loss`` gives, from another direction -- and ``vi[c] =
    (1 / S) sum_s vi(c, s)``, the posterior expected variation of information in bits (``partition_loss`` has only its
    Jensen bound ``vi_lb``: ``vi[c] >= vi_lb[c] + (1 / (m S)) sum_s sum_i s_i log2 s_i`` over the samples' cluster sizes).
    The sum over the samples runs in sample order and the division by S = ``valid`` last, in float64.
    ``assignments`` as for ``zmatrix`` (an open ``ZMatrix`` keeps no samples and raises ``ValueError``); ``candidates``
    as for ``partition_loss``, ``None`` for the samples themselves.  Runs and returns where ``partition_distances`` would."""
    samples, ctx = _samples_for_distances(assignments, ctx)
    m = int(samples.shape[1])
    if candidates is None:
        cands = samples
    else:
        cands = _device_candidates(candidates, ctx, m) if ctx is not None else _host_candidates(candidates, m)
    return _expected(samples, cands, ctx)


def vi_estimate(assignments, candidates=None, ctx=None, refine=0, starts=8):
    """ONE clustering out of posterior samples by the exact expected variation of information: ``point_estimate`` with
    ``expected_loss``'s ``vi`` where ``loss="vi"`` has the bound.  Returns the same ``PointEstimate`` tuple of numpy
    values: ``labels`` of the winner (numbered by first row), ``index`` (the lowest among equal losses), ``losses`` (the
    expected VI of every candidate, bits) and ``confidence`` as ``point_estimate`` computes it.

    ``refine > 0``: the ``starts`` candidates of lowest expected VI (ties to the lowest index) are each refined by greedy
    row moves for at most ``refine`` sweeps (``refine_partition_vi``) and the best refined partition by its exact float64
    expected VI is returned (ties to the better-ranked start): ``labels`` and ``confidence`` are its own, ``index`` is the
    candidate it grew from, ``losses`` stay the candidates' own."""
    refine, starts = int(refine), int(starts)
    if refine < 0 or starts < 1:
        raise ValueError("refine must not be negative and starts must be at least 1")
    samples, ctx = _samples_for_distances(assignments, ctx)
    sc = _Scorer(samples, ctx)
    try:
        c = sc.candidates(candidates)
        vi = _expected(samples, c, ctx).vi
        losses = vi.cpu().numpy() if isinstance(vi, torch.Tensor) else np.asarray(vi)
        valid = int(samples.shape[0])
        if refine > 0:
            top = np.argsort(losses, kind="stable")[:starts]
            picked = c[torch.from_numpy(top).to(c.device)] if isinstance(c, torch.Tensor) else c[top]
            got = _refine_vi(samples, picked, refine, None, None, ctx)
            rvi = _expected(samples, got[0], ctx).vi
            rvi = rvi.cpu().numpy() if isinstance(rvi, torch.Tensor) else np.asarray(rvi)
            best = int(np.argmin(rvi))
            labels = got[0][best]
            labels = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else labels
            w, size = sc.sums_of_positions(labels)
            confidence = w[0].astype(np.float64) / (float(valid) * size[0].astype(np.float64))
            return PointEstimate(_renumber(labels), int(top[best]), losses, confidence)
        index = int(np.argmin(losses))
        w, size = sc.sums(c[index:index + 1])
        confidence = w[0].astype(np.float64) / (float(valid) * size[0].astype(np.float64))
        return PointEstimate(_renumber(sc.selected(c[index])), index, losses, confidence)
    finally:
        sc.close()


# ---- greedy refinement under the exact expected VI --------------------------------------------------------------------
RefinedVI = collections.namedtuple("RefinedVI", ["labels", "vi", "vi_start", "decrease", "sweeps", "moves", "valid"])
_INT64_MAX = np.iinfo(np.int64).max


def vi_table(m):
    """``F[0..m]`` of ``msc_vi_table``: int64, ``F(0) = 0`` and ``F(n) = rint(n log2(n) 2^24)``, computed by the library on
    the host (no GPU is needed).  The one table that the host path and the kernels of ``refine_partition_vi`` share."""
    m = int(m)
    if m < 0 or m >= 2 ** 32:
        raise ValueError("m must lie in [0, 2^32)")
    F = np.empty(m + 1, dtype=np.int64)
    _lib.check(_lib.load().msc_vi_table(m, F.ctypes.data))
    return F


def _refine_vi_host(samples, starts, max_sweeps, max_clusters, order):
    """The rule of msc_partition_refine_vi (include/microscopes_hip.h) in plain numpy, all int64: samples [S, m], starts
    [nstarts, m] -> (labels int32 [nstarts, m], decrease int64, sweeps int32, moves int64)"""
    samples, starts = np.asarray(samples), np.asarray(starts)
    S, m = samples.shape
    ns = starts.shape[0]
    K = int(max_clusters)
    if K < 1 or K > m:
        raise ValueError("max_clusters must lie in [1, m = %d]" % m)
    if int(max_sweeps) < 0:
        raise ValueError("max_sweeps must not be negative")
    if order is not None and not _is_permutation(np.asarray(order), m):
        raise ValueError("not a valid permutation")
    visit = np.arange(m) if order is None else np.asarray(order).astype(np.int64)
    G = np.diff(vi_table(m))                           # G[n] = F(n + 1) - F(n), 0 <= n < m
    sid, _ = _dense_labels(samples)                    # per sample, ids in [0, L_s)
    L = sid.max(axis=1).astype(np.int64) + 1
    off = np.concatenate(([0], np.cumsum(L)[:-1]))
    stretch = off[:, None] + sid                       # [S, m]: the row of cells that row a touches in sample s
    labels = np.empty((ns, m), dtype=np.int32)
    decrease = np.zeros(ns, dtype=np.int64)
    sweeps = np.zeros(ns, dtype=np.int32)
    moves = np.zeros(ns, dtype=np.int64)
    for i in range(ns):
        ids = _renumber(starts[i]).astype(np.int64)
        if int(ids.max()) + 1 > K:
            raise ValueError("a start holds %d clusters, more than max_clusters = %d" % (int(ids.max()) + 1, K))
        n = np.bincount(ids, minlength=K).astype(np.int64)
        N = np.zeros((int(L.sum()), K), dtype=np.int64)
        np.add.at(N, (stretch, np.broadcast_to(ids, (S, m))), 1)
        dec = 0
        for _ in range(int(max_sweeps)):
            moved = 0
            for a in visit:
                c = int(ids[a])
                r = stretch[:, a]
                n[c] -= 1                              # n' from here on
                N[r, c] -= 1
                D = S * G[n] - 2 * G[N[r]].sum(axis=0)
                there = n > 0
                d_cur = int(D[c]) if there[c] else 0
                target, d_target = -1, 0
                if there.any():
                    target = int(np.argmin(np.where(there, D, _INT64_MAX)))     # the first of the smallest: the lowest id
                    d_target = int(D[target])
                    if there[c] and d_target > 0:
                        free = np.flatnonzero(n == 0)
                        if free.size:
                            target, d_target = int(free[0]), 0
                if target < 0 or not d_target < d_cur:
                    target = c
                else:
                    dec += d_cur - d_target
                    moved += 1
                n[target] += 1
                N[r, target] += 1
                ids[a] = target
            sweeps[i] += 1
            moves[i] += moved
            if moved == 0:
                break
        labels[i] = _renumber(ids)
        decrease[i] = dec
    return labels, decrease, sweeps, moves


def _refine_vi(samples, starts, max_sweeps, max_clusters, order, ctx):
    """(labels, decrease, sweeps, moves) of starts against samples, both already where they run"""
    m = int(samples.shape[1])
    if max_clusters is None:
        max_clusters = min(m, REFINE_VI_MAX_CLUSTERS)
    if ctx is None:
        return _refine_vi_host(samples, starts, max_sweeps, max_clusters, order)
    return ctx.partition_refine_vi(samples.contiguous(), starts.contiguous(), max_sweeps, max_clusters, order)


def refine_partition_vi(assignments, starts=None, nstarts=8, max_sweeps=20, max_clusters=None, order=None, ctx=None):
    """Partitions taken to a local optimum of the EXACT posterior expected variation of information by greedy row moves.

    From each start, rows are visited in ascending order (or in ``order``, a permutation of the rows) and each moves to
    the cluster -- or alone into a new one -- that lowers the expected VI most; a row stays on a tie, and an existing
    cluster is preferred to a new one at equal gain.  Sweeps repeat until one moves nothing or ``max_sweeps`` have run.
    The gains are integers, read from ``vi_table`` (n log2 n in fixed point, scale 2^%d), which the host path and the
    kernel share (include/microscopes_hip.h states the rule in full under msc_partition_refine_vi): ``decrease /
    (valid m 2^%d)`` is the expected VI lost, in bits, up to the table's rounding.  Every move lowers the integer
    objective strictly, and a result with ``sweeps < max_sweeps`` is a local optimum of it: no single row move lowers it.

    ``assignments`` as for ``expected_loss`` (an open ``ZMatrix`` keeps no samples and raises ``ValueError``); ``starts``
    as ``partition_loss`` takes candidates, ``None`` for the ``nstarts`` samples of lowest exact expected VI (ties to the
    lowest index).  ``max_clusters``: the most clusters a partition may hold on the way (``None``: ``min(m, %d)``); a start
    that holds more raises ``ValueError``.  Returns a named tuple ``(labels [nstarts, m] int32, numbered from 0 in the
    order of first row; vi float64 [nstarts], the exact expected VI of the results, and vi_start, of the starts, both from
    expected_loss; decrease int64 [nstarts]; sweeps int32 [nstarts], the last one that moved nothing included; moves
    int64 [nstarts]; valid)``.  Numpy input without ``ctx`` runs the host implementation, plain numpy; device tensors or
    ``ctx=`` run ``msc_partition_refine_vi`` and return device tensors holding the same integers, bit for bit."""
    samples, ctx = _samples_for_distances(assignments, ctx)
    m, S = int(samples.shape[1]), int(samples.shape[0])
    if starts is None:
        nstarts = int(nstarts)
        if nstarts < 1:
            raise ValueError("nstarts must be at least 1")
        vi_all = _expected(samples, samples, ctx).vi
        vi_all = vi_all.cpu().numpy() if isinstance(vi_all, torch.Tensor) else np.asarray(vi_all)
        top = np.argsort(vi_all, kind="stable")[:nstarts]
        c = samples[torch.from_numpy(top).to(samples.device)] if isinstance(samples, torch.Tensor) else samples[top]
    else:
        c = _device_candidates(starts, ctx, m) if ctx is not None else _host_candidates(starts, m)
    labels, decrease, sweeps, moves = _refine_vi(samples, c, max_sweeps, max_clusters, order, ctx)
    return RefinedVI(labels, _expected(samples, labels, ctx).vi, _expected(samples, c, ctx).vi, decrease, sweeps, moves, S)


refine_partition_vi.__doc__ %= (24, 24, REFINE_VI_MAX_CLUSTERS)
assert VI_TABLE_SCALE == 1 << 24


def credible_ball(assignments, estimate, level=0.95, metric="vi", ctx=None):
    """Wade and Ghahramani's credible ball around ``estimate`` (``mcclust.ext::credibleball``): the smallest ball, in the
    ``metric`` (``"vi"`` in bits or ``"binder"`` in row pairs), that holds at least ``level`` of the samples.

    With ``d[s]`` the distance from ``estimate`` to sample s: ``radius`` is the ceil(level S)-th smallest ``d`` (1-based);
    ``members`` is ``d <= radius``; ``horizontal`` the members at the largest distance; ``upper`` the members with the
    fewest clusters and, among those, the largest distance; ``lower`` the members with the most clusters and, among
    those, the largest distance -- each an ascending array of sample indices.  Returns a named tuple of numpy values
    ``(distances [S], radius, members bool [S], horizontal, upper, lower, nclusters int32 [S])``.  ``assignments`` as for
    ``expected_loss``; ``estimate``: one vector of m labels.  Runs where ``partition_distances`` would."""
    if metric not in _METRICS:
        raise ValueError("metric must be one of %s" % (_METRICS,))
    level = float(level)
    if not (0. < level <= 1.):
        raise ValueError("level must lie in (0, 1]")
    samples, ctx = _samples_for_distances(assignments, ctx)
    m, S = int(samples.shape[1]), int(samples.shape[0])
    est = _device_candidates(estimate, ctx, m) if ctx is not None else _host_candidates(estimate, m)
    if est.shape[0] != 1:
        raise ValueError("estimate must be one vector of labels")
    got = partition_distances(est, samples, ctx=ctx)
    d, k = (got.vi if metric == "vi" else got.binder)[0], got.nclusters_b
    d = d.cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
    k = k.cpu().numpy() if isinstance(k, torch.Tensor) else np.asarray(k)
    rank = min(S, max(1, int(math.ceil(level * S))))
    radius = np.sort(d)[rank - 1]
    members = d <= radius
    idx = np.flatnonzero(members)
    farthest = lambda sel: sel[d[sel] == d[sel].max()]
    return CredibleBall(d, radius, members, farthest(idx), farthest(idx[k[idx] == k[idx].min()]),
                        farthest(idx[k[idx] == k[idx].max()]), k)
