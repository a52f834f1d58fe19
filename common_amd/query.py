"""Posterior summaries of assignment samples: the interface of the reference's ``microscopes.common.query``.

``groups``, ``zmatrix``, ``zmatrix_reorder`` and ``zmatrix_heuristic_block_ordering`` take the same arguments, return the
same values and raise the same ``ValueError``s.  Numpy input runs a vectorised numpy path.  Device tensors (or numpy input
with ``ctx=``) build the z-matrix on the device (``ZMatrix``, ``msc_zmatrix_*``) and return a device tensor bit-equal to
the numpy path.  The block ordering is the leaf order of scipy's single linkage over the condensed upper triangle: scipy
itself for numpy input, ``msc_linkage_single`` for a float32 device tensor (the same dendrogram, bit for bit).
``zmatrix_linkage`` returns that dendrogram and ``zmatrix_clusters`` cuts a consensus partition out of it; the reference
exposes neither.
"""
import numpy as np
import torch

from ._lib import LINKAGE_MAX_N, ZMATRIX_MAX_LABELS
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


def _zmatrix_host(a):
    """float32 count / S: the counts as sums of one-hot products (exact in float64), a block of samples at a time"""
    S, n = a.shape
    dense, K = _dense_labels(a)
    counts = np.zeros((n, n), dtype=np.float64)
    step = max(1, _HOST_CHUNK_FLOATS // max(1, n * K))
    eye = np.eye(K, dtype=np.float64)
    for s0 in range(0, S, step):
        blk = dense[s0:s0 + step]
        H = eye[blk].transpose(1, 0, 2).reshape(n, -1)   # [n, samples x K]: row i's label of each sample, one-hot
        counts += H @ H.T
    return counts.astype(np.float32) / np.float32(S)


def _zmatrix_device(a, ctx):
    """a: int32 device tensor [S, n]"""
    S, n = int(a.shape[0]), int(a.shape[1])
    lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= ZMATRIX_MAX_LABELS:
        a = torch.stack([torch.unique(a[s], return_inverse=True)[1] for s in range(S)]).to(torch.int32)
        hi = int(a.max())
    zm = ZMatrix(ctx, n, hi + 1)
    try:
        zm.add(a.contiguous())
        return zm.result()
    finally:
        zm.close()


def zmatrix(assignments, ctx=None):
    """Z[i, j] = the fraction of the assignment vectors in which rows i and j share a label (float32 [n, n]).

    ``assignments``: a list (or [S, n] array) of assignment vectors of equal length.  Numpy input returns a numpy array;
    a device tensor, a list of device tensors, or any input with ``ctx`` (a ``Context``) runs on the device and returns a
    float32 device tensor with the same bits."""
    _check_assignments(assignments)
    on_device = ctx is not None or _is_device(assignments) or \
        (not isinstance(assignments, (np.ndarray, torch.Tensor)) and any(_is_device(a) for a in assignments))
    if not on_device:
        a = np.asarray([np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in assignments])
        return _zmatrix_host(a.reshape(len(assignments), -1))
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
    return _zmatrix_device(a.reshape(a.shape[0], -1), ctx)


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
