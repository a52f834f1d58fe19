"""Host-side objects over the C-ABI: Context, DataView, State.

PyTorch is used here only as the owner of device memory (tensors hold the
columns, assignment vectors and score matrices) and of the HIP stream; every
computation is a call into libmicroscopes_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _args as A
from . import _lib as L

_NP_OF_TYPE = {L.TYPE_B: np.bool_, L.TYPE_I8: np.int8, L.TYPE_U8: np.uint8, L.TYPE_I16: np.int16,
               L.TYPE_U16: np.uint16, L.TYPE_I32: np.int32, L.TYPE_U32: np.uint32,
               L.TYPE_I64: np.int64, L.TYPE_U64: np.uint64, L.TYPE_F32: np.float32,
               L.TYPE_F64: np.float64}
_TORCH_OF_TYPE = {L.TYPE_B: torch.bool, L.TYPE_I8: torch.int8, L.TYPE_U8: torch.uint8,
                  L.TYPE_I16: torch.int16, L.TYPE_I32: torch.int32, L.TYPE_I64: torch.int64,
                  L.TYPE_F32: torch.float32, L.TYPE_F64: torch.float64}
_TYPE_OF_TORCH = {torch.bool: L.TYPE_B, torch.int8: L.TYPE_I8, torch.uint8: L.TYPE_U8,
                  torch.int16: L.TYPE_I16, torch.int32: L.TYPE_I32, torch.int64: L.TYPE_I64,
                  torch.float32: L.TYPE_F32, torch.float64: L.TYPE_F64}
for _n, _t in (("uint16", L.TYPE_U16), ("uint32", L.TYPE_U32), ("uint64", L.TYPE_U64)):
    if hasattr(torch, _n):
        _TYPE_OF_TORCH[getattr(torch, _n)] = _t
        _TORCH_OF_TYPE[_t] = getattr(torch, _n)

_I32_U32 = (torch.int32, _TORCH_OF_TYPE.get(L.TYPE_U32, torch.int32))      # what an `order` tensor may hold

VALUE_TYPE = {L.BB: L.TYPE_B, L.BBNC: L.TYPE_B, L.GP: L.TYPE_U32, L.DD: L.TYPE_I32, L.NICH: L.TYPE_F32,
              L.NIW: L.TYPE_F32, L.NOOP: L.TYPE_B, L.BNB: L.TYPE_U32, L.DM: L.TYPE_I32}


def type_of_numpy(dt):
    """numpy scalar dtype -> primitive type (microscopes/common/_dataview.pyx:6-36)."""
    dt = np.dtype(dt)
    for t, npt in _NP_OF_TYPE.items():
        if np.dtype(npt) == dt:
            return t
    raise ValueError("Unknown type: %s" % dt)


def runtime_types_of(dtype):
    """structured dtype -> [(primitive type, count)] (_dataview.pyx:27-44)."""
    dtype = np.dtype(dtype)
    if len(dtype) == 0:
        raise ValueError("structural arrays only")
    out = []
    for i in range(len(dtype)):
        ft = dtype[i]
        if ft.subdtype is None:
            out.append((type_of_numpy(ft), 1))
        else:
            sub, shape = ft.subdtype
            if len(shape) != 1:
                raise ValueError("unsupported shape: %s" % (shape,))
            out.append((type_of_numpy(sub), int(shape[0])))
    return out


class Context(object):
    """One per process and GPU.  Kernels are enqueued on torch's current stream."""

    def __init__(self, device=0, stream=None):
        if not torch.cuda.is_available():
            raise L.MicroscopesHipError(-3, "no GPU visible to torch; common_amd has no CPU path")
        self.lib = L.load()
        self.device = int(device)
        torch.cuda.set_device(self.device)
        torch.cuda.init()
        self.torch_device = torch.device("cuda", self.device)
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        self._stream = s
        h = C.c_void_p()
        L.check(self.lib.msc_context_create(self.device, C.c_void_p(s.cuda_stream), C.byref(h)))
        self._h = h
        import weakref
        self._buffers = weakref.WeakSet()      # live msc_device_alloc* buffers that tensors alias (alloc / alloc_probed)

    def set_stream(self, stream):
        self._stream = stream
        L.check(self.lib.msc_context_set_stream(self._h, C.c_void_p(stream.cuda_stream)))

    def synchronize(self):
        L.check(self.lib.msc_context_synchronize(self._h))

    def build_info(self):
        return self.lib.msc_build_info().decode()

    def last_kernel(self, which="score"):
        """the kernel instantiation of this process's most recent scoring ("score") or fused assignment ("sweep") pass, or
        z-matrix, linkage or partition-distance kernel ("zmatrix"), as rocprofv3 spells it (msc_last_kernel): what bench.py keys the committed counter
        summaries by"""
        return self.lib.msc_last_kernel({"score": 0, "zmatrix": 2, "marginal": 3}.get(which, 1)).decode()

    def linkage_single(self, z, linkage=True, order=True):
        """scipy's single linkage of the distances 1 - z and / or its leaf order (msc_linkage_single): z a float32
        [n, n] tensor on this device, 2 <= n, with contiguous rows (any row stride >= n), SYMMETRIC and finite off the
        diagonal (the diagonal's value is never used).  Returns (float64 [n - 1, 4] or None, int32 [n] or None).  Synchronous."""
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[0] != z.shape[1]:
            raise ValueError("z must be a square float32 tensor on %s with contiguous rows" % self.torch_device)
        n = int(z.shape[0])
        zp, ld = A.matrix(z, torch.float32, n, n, self.torch_device, "z")
        # rows that start on 16 bytes are read 16 bytes a lane, up to 3 floats past column n - 1 inside the row's ld: a
        # view whose storage ends before that in its last row (as_strided can make one) is copied first
        if (n - 1) * int(z.stride(0)) + (n + 3) // 4 * 4 > z.untyped_storage().nbytes() // 4 - int(z.storage_offset()):
            z = z.contiguous()
            zp, ld = A.ptr(z), n
        lk = np.empty((max(n - 1, 0), 4), dtype=np.float64) if linkage else None
        od = np.empty(n, dtype=np.uint32) if order else None
        L.check(self.lib.msc_linkage_single(self._h, zp, ld, n, 0,
                                            None if lk is None else lk.ctypes.data_as(C.c_void_p),
                                            None if od is None else od.ctypes.data_as(C.c_void_p)))
        return lk, (None if od is None else od.astype(np.int32))

    def partition_distances(self, a, b=None):
        """The contingency sums of every partition of a against every partition of b (msc_partition_distances): int32
        tensors [m] or [count, m] on this device whose rows are contiguous (any row stride >= m); any int32 value is a
        label.  b None: a against itself.  Returns device tensors (pairs_ab int64 [na, nb], nlogn_ab float64 [na, nb],
        pairs_a int64 [na], nlogn_a float64 [na], nclusters_a int32 [na], pairs_b, nlogn_b, nclusters_b), as
        include/microscopes_hip.h defines them; common_amd.query makes Binder's distance, the variation of information
        and the adjusted Rand index of them.  At most %d clusters a partition: counted before anything is launched, more
        raise ValueError.  More than %d rows: MicroscopesHipError (MSC_EUNSUPPORTED)."""
        a2, na, lda = A.vectors(a, self.torch_device, "a")
        m = int(a2.shape[-1])
        if b is None:
            b2, nb, ldb = None, na, lda
        else:
            b2, nb, ldb = A.vectors(b, self.torch_device, "b")
            if b2.shape[-1] != m:
                raise ValueError("a and b must label the same rows: m = %d and %d" % (m, b2.shape[-1]))
        if m <= L.DISTANCES_MAX_ROWS:
            for p in (a2,) if b2 is None else (a2, b2):
                srt = torch.sort(p.reshape(-1, m), dim=1).values
                most = int(((srt[:, 1:] != srt[:, :-1]).sum(dim=1) + 1).max())
                if most > L.DISTANCES_MAX_CLUSTERS:
                    raise ValueError("a partition holds %d clusters, more than %d" % (most, L.DISTANCES_MAX_CLUSTERS))
        dev = self.torch_device
        pairs_ab = torch.empty((na, nb), dtype=torch.int64, device=dev)
        nlogn_ab = torch.empty((na, nb), dtype=torch.float64, device=dev)
        per = []
        for n in (na, nb):
            per += [torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                    torch.empty(n, dtype=torch.int32, device=dev)]
        L.check(self.lib.msc_partition_distances(
            self._h, A.ptr(a2), lda, na, None if b2 is None else A.ptr(b2), ldb, nb, m, 0, A.ptr(pairs_ab), A.ptr(nlogn_ab),
            *[A.ptr(t) for t in per]))
        return (pairs_ab, nlogn_ab) + tuple(per)
    partition_distances.__doc__ %= (L.DISTANCES_MAX_CLUSTERS, L.DISTANCES_MAX_ROWS)

    def partition_refine_vi(self, samples, starts, max_sweeps=20, max_clusters=None, order=None, workspace_bytes=0):
        """Greedy refinement of partitions under the exact posterior expected variation of information
        (msc_partition_refine_vi; include/microscopes_hip.h states the rule).  samples, starts: int32 tensors [m] or
        [count, m] on this device whose rows are contiguous (any row stride >= m); any int32 value is a label.  From each
        start rows move one at a time to the cluster, or into a new one, that lowers the expected VI most, sweep after
        sweep (rows ascending, or in `order`, a permutation of [0, m)), until a sweep moves nothing or max_sweeps have
        run.  max_clusters: the most clusters a partition may hold on the way (None: min(m, %d)).  The clusters are
        counted before anything is launched: a start with more than max_clusters, or a sample with more than %d, raises
        ValueError.  workspace_bytes (0: 2 GiB) bounds the contingency cells of the starts refined at a time; the outputs
        do not depend on it.  Returns device tensors (labels int32 [nstarts, m], numbered by first row; decrease int64
        [nstarts], in units of 1 / (S m 2^24) bits; sweeps int32 [nstarts], the last one that moved nothing included;
        moves int64 [nstarts]), bit-equal to common_amd.query's host path.  Asynchronous after one wait."""
        dev = self.torch_device
        s2, S, lds = A.vectors(samples, dev, "samples")
        m = int(s2.shape[-1])
        c2, ns, ld = A.vectors(starts, dev, "starts", m)
        if ns == 0:
            raise ValueError("starts must be [m] or [count, m], neither 0")
        if max_clusters is None:
            max_clusters = min(m, L.REFINE_VI_MAX_CLUSTERS)
        max_sweeps, max_clusters, workspace_bytes = int(max_sweeps), int(max_clusters), int(workspace_bytes)
        if max_sweeps < 0 or max_sweeps >= 2 ** 32:
            raise ValueError("max_sweeps must lie in [0, 2^32)")
        if max_clusters < 1 or max_clusters > m:
            raise ValueError("max_clusters must lie in [1, m = %d]" % m)
        if workspace_bytes < 0:
            raise ValueError("workspace_bytes must not be negative")
        o = None
        if order is not None:
            o = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order)
            if o.shape != (m,) or not np.issubdtype(o.dtype, np.integer) or (o.min() < 0 or o.max() >= m) or \
                    np.unique(o).size != m:
                raise ValueError("not a valid permutation")
            o = np.ascontiguousarray(o, dtype=np.uint32)
        if m <= L.REFINE_VI_MAX_ROWS and S <= L.REFINE_VI_MAX_SAMPLES and max_clusters <= L.REFINE_VI_MAX_CLUSTERS:
            for p, cap, what in ((s2, L.REFINE_VI_MAX_CLUSTERS, "sample"), (c2, max_clusters, "start")):
                srt = torch.sort(p.reshape(-1, m), dim=1).values
                most = int(((srt[:, 1:] != srt[:, :-1]).sum(dim=1) + 1).max())
                if most > cap:
                    raise ValueError("a %s holds %d clusters, more than %d" % (what, most, cap))
        labels = torch.empty((ns, m), dtype=torch.int32, device=dev)
        decrease = torch.empty(ns, dtype=torch.int64, device=dev)
        sweeps = torch.empty(ns, dtype=torch.int32, device=dev)
        moves = torch.empty(ns, dtype=torch.int64, device=dev)
        L.check(self.lib.msc_partition_refine_vi(
            self._h, A.ptr(s2), lds, S, m, A.ptr(c2), ld, ns, max_sweeps, max_clusters,
            None if o is None else o.ctypes.data_as(C.c_void_p), workspace_bytes, 0,
            A.flat(labels, torch.int32, ns * m, dev, "labels"), A.flat(decrease, torch.int64, ns, dev, "decrease"),
            A.flat(sweeps, torch.int32, ns, dev, "sweeps"), A.flat(moves, torch.int64, ns, dev, "moves")))
        return labels, decrease, sweeps, moves
    partition_refine_vi.__doc__ %= (L.REFINE_VI_MAX_CLUSTERS, L.REFINE_VI_MAX_CLUSTERS)

    def value_op(self, family, dim, op, hp, ss_record, value=None):
        """One group::{add_value, remove_value, score_value, score_data} call (base.hpp:25-28) as a batch
        of one on the device.  op: "add" | "remove" | "score_value" | "score_data".  `ss_record` is a
        1-element array of ss_dtype(family, dim), updated in place by add/remove; returns the score."""
        code = {"add": 0, "remove": 1, "score_value": 2, "score_data": 3}[op]
        hpb = pack_hp(family, hp, dim)
        assert ss_record.dtype == ss_dtype(family, dim) and ss_record.size == 1 and ss_record.flags.c_contiguous
        vb = None
        if value is not None:
            vb = np.ascontiguousarray(value, dtype={L.TYPE_B: np.uint8, L.TYPE_U32: np.uint32, L.TYPE_I32: np.int32,
                                                    L.TYPE_F32: np.float32}[VALUE_TYPE[family]])
        score = C.c_float(0)
        L.check(self.lib.msc_value_op_single(self._h, int(family), int(dim), code, hpb.ctypes.data_as(C.c_void_p),
                                             ss_record.ctypes.data_as(C.c_void_p),
                                             vb.ctypes.data_as(C.c_void_p) if vb is not None else None,
                                             C.byref(score)))
        return float(score.value)

    def alloc(self, shape, dtype=torch.float32):
        """A zero-filled device tensor from msc_device_alloc -- the library's default allocator: from 64 MiB on the buffer
        is placed for the write stream of a score matrix (include/microscopes_hip.h).  The tensor owns the buffer."""
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        p = C.c_void_p()
        L.check(self.lib.msc_device_alloc(self._h, nbytes, C.byref(p)))
        return _alias_tensor(p.value, n, dtype, self.torch_device, owner=_DeviceBuffer(self, p.value)).reshape(*shape)

    def alloc_stats(self):
        """([GB/s fill rate of every candidate the most recent placed allocation tried], index kept)"""
        rates, n, chosen = (C.c_float * 64)(), C.c_uint32(), C.c_uint32()
        L.check(self.lib.msc_device_alloc_stats(self._h, rates, 64, C.byref(n), C.byref(chosen)))
        return [float(rates[i]) for i in range(min(n.value, 64))], int(chosen.value)

    def alloc_probed(self, shape, dtype=torch.float32, candidates=8):
        """A zero-filled device tensor in the best-placed of `candidates` allocations (msc_device_alloc_probed; the
        write stream of a large score matrix runs 5.6 or 7.0 TB/s depending on where the driver put it).
        -> (tensor, [GB/s of every candidate], index kept).  The tensor owns the buffer (freed with it)."""
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        p, rates, chosen = C.c_void_p(), (C.c_float * candidates)(), C.c_uint32()
        L.check(self.lib.msc_device_alloc_probed(self._h, nbytes, candidates, C.byref(p), rates, C.byref(chosen)))
        t = _alias_tensor(p.value, n, dtype, self.torch_device, owner=_DeviceBuffer(self, p.value)).reshape(*shape)
        return t, [float(r) for r in rates], int(chosen.value)

    def close(self):
        """destroy the context.  Refused while tensors from alloc() / alloc_probed() are alive: destroying the context
        unmaps their memory (the buffers hold a reference to the context, so garbage collection never gets here first)"""
        if getattr(self, "_h", None):
            live = [b for b in getattr(self, "_buffers", ()) if b.ptr]
            if live:
                raise RuntimeError("Context.close(): %d device buffer(s) from alloc()/alloc_probed() are still referenced "
                                   "by tensors; drop those first" % len(live))
            self.lib.msc_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DataView(object):
    """Columnar device copy of a packed recarray (replaces recarray numpy_dataview)."""

    def __init__(self, ctx, handle, keepalive=None):
        self.ctx, self._h, self._keep = ctx, handle, keepalive
        n, f = C.c_uint64(), C.c_uint32()
        L.check(ctx.lib.msc_dataview_size(handle, C.byref(n), C.byref(f)))
        self.nrows, self.nfeatures = n.value, f.value

    @classmethod
    def from_recarray(cls, ctx, npd, col_types=None):
        """numpy structured (optionally masked) 1-D array, as recarray/_dataview.pyx:61-92."""
        if npd is None:
            raise ValueError("npd is None")
        if len(npd.shape) != 1:
            raise ValueError("1D (structural) arrays only")
        types = runtime_types_of(npd.dtype)
        if hasattr(npd, "mask"):
            data = np.ascontiguousarray(npd.data)
            mask = np.ascontiguousarray(np.ma.getmaskarray(npd))
            mask = mask.view(np.uint8).reshape(-1)
        else:
            data, mask = np.ascontiguousarray(npd), None
        if data.dtype.itemsize != sum(np.dtype(_NP_OF_TYPE[t]).itemsize * c for t, c in types):
            data = np.ascontiguousarray(data.astype(np.dtype([("f%d" % i, _NP_OF_TYPE[t], (c,)) if c > 1
                                                              else ("f%d" % i, _NP_OF_TYPE[t])
                                                              for i, (t, c) in enumerate(types)])))
        rt = (L.RuntimeType * len(types))(*[L.RuntimeType(t, c) for t, c in types])
        ct = None
        if col_types is not None:
            ct = (C.c_int32 * len(types))(*[int(t) for t in col_types])
        h = C.c_void_p()
        L.check(ctx.lib.msc_dataview_from_records(
            ctx._h, data.ctypes.data_as(C.c_void_p),
            mask.ctypes.data_as(C.c_void_p) if mask is not None else None,
            data.shape[0], rt, len(types), ct, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_tensors(cls, ctx, columns, masks=None):
        """Adopt device tensors as columns (no copy).  [N] scalars or [N, d] vector features."""
        cols, dev = list(columns), ctx.torch_device
        ptrs = (C.c_void_p * len(cols))(*[A.flat(c, tuple(_TYPE_OF_TORCH), 0, dev, "a column") for c in cols])
        n = cols[0].shape[0]
        types = []
        for c in cols:
            if c.shape[0] != n or c.dim() > 2:
                raise ValueError("column shapes must be [N] or [N, d] with one N")
            types.append((_TYPE_OF_TORCH[c.dtype], 1 if c.dim() == 1 else int(c.shape[1])))
        rt = (L.RuntimeType * len(types))(*[L.RuntimeType(t, k) for t, k in types])
        mptr = None
        if masks is not None:
            masks = list(masks)
            if len(masks) != len(cols):
                raise ValueError("masks must hold one entry (a tensor or None) per column")
            mptr = (C.c_void_p * len(cols))(*[A.flat(m, (torch.uint8, torch.bool), n * k, dev, "a mask", True)
                                              for m, (_, k) in zip(masks, types)])
        h = C.c_void_p()
        L.check(ctx.lib.msc_dataview_from_device_columns(ctx._h, n, rt, len(types), ptrs, mptr, C.byref(h)))
        return cls(ctx, h, keepalive=(cols, masks))

    def column_type(self, f):
        p, t = C.c_void_p(), L.RuntimeType()
        L.check(self.ctx.lib.msc_dataview_column(self._h, f, C.byref(p), C.byref(t)))
        return t.type, t.count, p.value

    def column_to_numpy(self, f):
        """Device column -> numpy (tests / debugging)."""
        t, cnt, ptr = self.column_type(f)
        npt = np.dtype(_NP_OF_TYPE[t])
        nbytes = self.nrows * cnt * npt.itemsize
        self.ctx.synchronize()
        if nbytes == 0:
            return np.zeros((0, cnt) if cnt > 1 else (0,), dtype=npt)
        buf = _alias_tensor(ptr, nbytes, torch.uint8, self.ctx.torch_device)
        out = buf.cpu().numpy().view(npt)
        return out.reshape(self.nrows, cnt) if cnt > 1 else out

    def __len__(self):
        return self.nrows

    def size(self):
        return self.nrows

    def invalidate(self):
        """the adopted tensors were rewritten in place: drop what the library derived from them (msc_dataview_invalidate)"""
        L.check(self.ctx.lib.msc_dataview_invalidate(self._h))

    def close(self):
        if getattr(self, "_h", None):
            # (a view that outlives its context -- kept alive by a traceback, say -- must not hand the library a handle whose
            # context is gone: the context's destruction already released the device)
            if getattr(self.ctx, "_h", None):
                self.ctx.lib.msc_dataview_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ss_dtype(family, dim=0):
    """numpy record of one group's suff-stats as msc_state_set_ss / get_ss exchange it."""
    if family == L.BB:
        return np.dtype([("heads", np.uint32), ("tails", np.uint32)])
    if family == L.BBNC:
        return np.dtype([("heads", np.uint32), ("tails", np.uint32), ("p", np.float32)])
    if family == L.GP:
        return np.dtype([("count", np.uint32), ("sum", np.uint32), ("log_prod", np.float32)])
    if family == L.DD:
        return np.dtype([("count_sum", np.uint32), ("counts", np.uint32, (dim,))])
    if family == L.BNB:
        return np.dtype([("count", np.uint32), ("sum", np.uint32)])
    if family == L.DM:
        return np.dtype([("counts", np.uint32, (dim,)), ("ratio", np.float32)])
    if family == L.NICH:
        return np.dtype([("count", np.uint32), ("mean", np.float32), ("count_times_variance", np.float32)])
    if family == L.NIW:
        return np.dtype([("count", np.uint32), ("sum_x", np.float32, (dim,)),
                         ("sum_xxT", np.float32, (dim, dim))])
    return np.dtype([("unused", np.uint32)])


def pack_hp(family, hp, dim=0):
    """dict keyed as microscopes/models.pyx:185-290 -> the flat float block of the ABI."""
    if isinstance(hp, np.ndarray):
        return np.ascontiguousarray(hp, dtype=np.float32)
    if family in (L.BB, L.BBNC):
        v = [hp["alpha"], hp["beta"]]
    elif family == L.GP:
        v = [hp["alpha"], hp["inv_beta"]]
    elif family in (L.DD, L.DM):
        v = list(hp["alphas"])
    elif family == L.BNB:
        v = [hp["alpha"], hp["beta"], hp["r"]]
    elif family == L.NICH:
        v = [hp["mu"], hp["kappa"], hp["sigmasq"], hp["nu"]]
    elif family == L.NIW:
        v = [hp["kappa"], hp["nu"]] + list(np.asarray(hp["mu"]).ravel()) + list(np.asarray(hp["psi"]).ravel())
    else:
        v = []
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


class State(object):
    """hypers + K groups of suff-stats per feature + CRP counts, resident in HBM."""

    def __init__(self, ctx, features, ngroups):
        """features: list of (family, dim) or model descriptors with .family/.dim."""
        self.ctx = ctx
        feats = []
        for f in features:
            if isinstance(f, tuple):
                feats.append((int(f[0]), int(f[1])))
            else:
                feats.append((int(f.family), int(f.dim)))
        self.features, self.K = feats, int(ngroups)
        spec = (L.FeatureSpec * len(feats))(*[L.FeatureSpec(a, b) for a, b in feats])
        h = C.c_void_p()
        L.check(ctx.lib.msc_state_create(ctx._h, spec, len(feats), self.K, C.byref(h)))
        self._h = h

    # hypers -----------------------------------------------------------------
    def set_hp(self, f, hp):
        self._drop_subsets()
        fam, dim = self.features[f]
        a = pack_hp(fam, hp, dim)
        L.check(self.ctx.lib.msc_state_set_hp(self._h, f, a.ctypes.data_as(C.c_void_p), a.size))

    def get_hp(self, f):
        fam, dim = self.features[f]
        a = np.empty(self.ctx.lib.msc_hp_floats(fam, dim), dtype=np.float32)
        L.check(self.ctx.lib.msc_state_get_hp(self._h, f, a.ctypes.data_as(C.c_void_p), a.size))
        return a

    # suff-stats -------------------------------------------------------------
    def set_ss(self, f, records, first_group=0):
        self._drop_subsets()
        fam, dim = self.features[f]
        r = np.ascontiguousarray(records, dtype=ss_dtype(fam, dim))
        L.check(self.ctx.lib.msc_state_set_ss(self._h, f, first_group, r.shape[0],
                                              r.ctypes.data_as(C.c_void_p), r.nbytes))

    def get_ss(self, f, first_group=0, ngroups=None):
        fam, dim = self.features[f]
        n = self.K - first_group if ngroups is None else ngroups
        r = np.zeros(n, dtype=ss_dtype(fam, dim))
        L.check(self.ctx.lib.msc_state_get_ss(self._h, f, first_group, n, r.ctypes.data_as(C.c_void_p), r.nbytes))
        return r

    def set_alpha(self, alpha):
        self._drop_subsets()
        L.check(self.ctx.lib.msc_state_set_alpha(self._h, float(alpha)))

    def set_group_counts(self, counts):
        self._drop_subsets()
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        L.check(self.ctx.lib.msc_state_set_group_counts(self._h, c.ctypes.data_as(C.c_void_p), c.size))

    def get_alpha(self):
        a = C.c_float()
        L.check(self.ctx.lib.msc_state_get_alpha(self._h, C.byref(a)))
        return a.value

    def get_group_counts(self):
        c = np.zeros(self.K, dtype=np.uint32)
        L.check(self.ctx.lib.msc_state_get_group_counts(self._h, c.ctypes.data_as(C.c_void_p), c.size))
        return c

    # hot path ---------------------------------------------------------------
    def _cols(self, cols):
        if cols is None:
            return None
        return (C.c_uint32 * len(cols))(*[int(c) for c in cols])

    def _slots(self, slots):
        return A.flat(slots, torch.uint8, self.K, self.ctx.torch_device, "slots", True)

    def _bind(self, view, row0, nrows, z, optional=False):
        """what every call over a view's rows starts with -> (row0, n, z's pointer).  The library keeps no reference to a
        view: this object does, for the last one bound."""
        self._bound_view = view
        row0, n = A.rows(view.nrows, row0, nrows)
        return row0, n, A.flat(z, torch.int32, n, self.ctx.torch_device, "z", optional)

    def score_value(self, view, out=None, row0=0, nrows=None, z=None, crp_prior=False, cols=None,
                    niw_f32=False):
        """[nrows, K] float32 device tensor of summed score_value (see msc_score_value)."""
        row0, n, zp = self._bind(view, row0, nrows, z, True)
        if out is None:
            out = torch.empty((n, self.K), dtype=torch.float32, device=self.ctx.torch_device)
        op, ld = A.matrix(out, torch.float32, n, self.K, self.ctx.torch_device, "out")
        L.check(self.ctx.lib.msc_score_value(self._h, view._h, self._cols(cols), row0, n, zp,
                                             (L.SCORE_CRP_PRIOR if crp_prior else 0) |
                                             (L.SCORE_NIW_F32 if niw_f32 else 0), op, ld))
        return out

    def score_tune(self, view, out, row0=0, nrows=None, cols=None):
        """Settle the single-nich pass's launch shape for passes like this one (synchronous, ~10 ms; msc_score_tune).
        -> (shape index or -1, ms per pass)."""
        row0, n, _ = self._bind(view, row0, nrows, None, True)
        op, ld = A.matrix(out, torch.float32, n, self.K, self.ctx.torch_device, "out")
        shape, ms = C.c_int(-1), C.c_float(0)
        L.check(self.ctx.lib.msc_score_tune(self._h, view._h, self._cols(cols), row0, n, op, ld, C.byref(shape),
                                            C.byref(ms)))
        return shape.value, ms.value

    def accumulate(self, view, z, row0=0, nrows=None, reset=True, subtract=False, commit=True, cols=None):
        self._drop_subsets()
        row0, n, zp = self._bind(view, row0, nrows, z)
        flags = (L.ACC_RESET if reset else 0) | (L.ACC_SUBTRACT if subtract else 0) | \
                (0 if commit else L.ACC_NO_COMMIT)
        L.check(self.ctx.lib.msc_accumulate(self._h, view._h, self._cols(cols), row0, n, zp, flags))

    def entity_op(self, view, row, group, join=True, z=None, cols=None):
        """one entity joins / leaves one group, the group by value (msc_entity_op): every table stays current"""
        self._drop_subsets()
        self._bound_view = view          # (as _bind)
        row, _ = A.rows(view.nrows, row, 1)
        zp = A.flat(z, torch.int32, row + 1, self.ctx.torch_device, "z", True)
        L.check(self.ctx.lib.msc_entity_op(self._h, view._h, self._cols(cols), row, int(group), 1 if join else -1, zp))

    def score_data(self, out=None):
        if out is None:
            out = torch.empty((len(self.features), self.K), dtype=torch.float32, device=self.ctx.torch_device)
        op, ld = A.matrix(out, torch.float32, len(self.features), self.K, self.ctx.torch_device, "out")
        if ld != self.K:
            raise ValueError("out must be a contiguous [nfeatures, K] tensor: msc_score_data takes no row stride")
        L.check(self.ctx.lib.msc_score_data(self._h, op))
        return out

    def _rows_call(self, fn, view, z, seed, sweep, row0, nrows, row_id0, cols):
        """the calls that take (view, cols, row0, nrows, row_id0, z, seed, sweep) and nothing else"""
        row0, n, zp = self._bind(view, row0, nrows, z)
        L.check(fn(self._h, view._h, self._cols(cols), row0, n, row0 if row_id0 is None else row_id0, zp, int(seed),
                   int(sweep)))

    def sweep_assign(self, view, z, seed, sweep, row0=0, nrows=None, row_id0=None, cols=None):
        self._rows_call(self.ctx.lib.msc_sweep_assign, view, z, seed, sweep, row0, nrows, row_id0, cols)

    def sweep_step(self, view, z, seed, sweep, row0=0, nrows=None, row_id0=None, cols=None):
        """sweep_assign + accumulate(reset) in one call; repeated steps replay as a HIP graph (msc_sweep_step)."""
        self._drop_subsets()
        self._rows_call(self.ctx.lib.msc_sweep_step, view, z, seed, sweep, row0, nrows, row_id0, cols)

    def sweep_step_begin(self, view, z, seed, sweep, row0=0, nrows=None, row_id0=None, cols=None):
        """the sharded step up to the exchange: follow with all-reduce of reduce_buffers() and commit_reduce()"""
        self._drop_subsets()
        self._rows_call(self.ctx.lib.msc_sweep_step_begin, view, z, seed, sweep, row0, nrows, row_id0, cols)

    def sweep_sequential(self, view, z, seed, sweep, nsweeps=1, order=None, trace=None, row0=0, nrows=None,
                         row_id0=None, cols=None):
        """nsweeps sequential collapsed Gibbs sweeps over the rows, each row scored against the tables the row before it
        left (msc_sweep_sequential).  order: uint32 (or int32) device tensor of nrows offsets from row0, the visiting
        order of every sweep (None: ascending); trace: int32 device tensor of nsweeps x nrows, z after every sweep."""
        self._drop_subsets()
        row0, n, zp = self._bind(view, row0, nrows, z)
        if not 0 <= int(nsweeps) < (1 << 32):
            raise ValueError("nsweeps must be in [0, 2^32)")
        dev = self.ctx.torch_device
        op = A.flat(order, _I32_U32, n, dev, "order", True)
        tp = A.flat(trace, torch.int32, int(nsweeps) * n, dev, "trace", True)
        L.check(self.ctx.lib.msc_sweep_sequential(self._h, view._h, self._cols(cols), row0, n,
                                                  row0 if row_id0 is None else row_id0, zp, op,
                                                  int(nsweeps), int(seed), int(sweep), tp))

    # the blocked (uncollapsed) Gibbs sampler ---------------------------------
    def blocked_draw(self, seed, sweep):
        """draw every slot's parameters and the stick weights from the tables as they stand (msc_blocked_draw)"""
        L.check(self.ctx.lib.msc_blocked_draw(self._h, int(seed), int(sweep)))

    def _tables(self, fn, ncols):
        """{"logw": float32[ncols], feature index: float32[nslices, ncols]}: views onto the device tables fn describes"""
        out = {}
        for f in [None] + list(range(len(self.features))):
            p, ns, ld = C.c_void_p(), C.c_uint32(), C.c_uint32()
            L.check(fn(self._h, 0xffffffff if f is None else f, C.byref(p), C.byref(ns), C.byref(ld)))
            if ns.value == 0:
                t = torch.empty((0, ncols), dtype=torch.float32, device=self.ctx.torch_device)
            else:
                t = _alias_tensor(p.value, ns.value * ld.value, torch.float32, self.ctx.torch_device,
                                  self).view(ns.value, ld.value)[:, :ncols]
            out["logw" if f is None else f] = t[0] if f is None else t
        return out

    def blocked_tables(self):
        """{"logw": float32[K], feature index: float32[nslices, K]}: views onto the device tables of the latest draw
        (msc_blocked_tables; the slices per family are listed in include/microscopes_hip.h)"""
        return self._tables(self.ctx.lib.msc_blocked_tables, self.K)

    def blocked_niw_params(self, f=0):
        """{"mean": float64[K, d], "whiten": float64[K, d (d + 1) / 2]}: views onto the matrices of the latest draw of a
        state of one niw feature -- the slot's mean and its lower-triangular whitening matrix V packed by rows, entry
        (i, j) at i (i + 1) / 2 + j (msc_blocked_niw_params)"""
        f = A.index(f, len(self.features), "feature")
        pm, pw, d = C.c_void_p(), C.c_void_p(), C.c_uint32()
        L.check(self.ctx.lib.msc_blocked_niw_params(self._h, f, C.byref(pm), C.byref(pw), C.byref(d)))
        dev, d = self.ctx.torch_device, d.value
        nt = d * (d + 1) // 2
        return {"mean": _alias_tensor(pm.value, self.K * d, torch.float64, dev, self).view(self.K, d),
                "whiten": _alias_tensor(pw.value, self.K * nt, torch.float64, dev, self).view(self.K, nt)}

    def blocked_assign(self, view, z, seed, sweep, row0=0, nrows=None, row_id0=None, cols=None):
        """every row's slot drawn independently under the parameters of the latest blocked_draw (msc_blocked_assign)"""
        self._rows_call(self.ctx.lib.msc_blocked_assign, view, z, seed, sweep, row0, nrows, row_id0, cols)

    def sweep_blocked(self, view, z, seed, sweep, nsweeps=1, trace=None, top_slot=None, row0=0, nrows=None,
                      row_id0=None, cols=None):
        """nsweeps blocked Gibbs sweeps: draw the parameters, draw every row's slot, accumulate (msc_sweep_blocked).
        trace: int32 device tensor of nsweeps x nrows, z after every sweep; top_slot: int32 / uint32 device tensor of
        nsweeps entries, the highest occupied slot after every sweep (K - 1: raise K)."""
        self._drop_subsets()
        row0, n, zp = self._bind(view, row0, nrows, z)
        if not 0 <= int(nsweeps) < (1 << 32):
            raise ValueError("nsweeps must be in [0, 2^32)")
        dev = self.ctx.torch_device
        tp = A.flat(trace, torch.int32, int(nsweeps) * n, dev, "trace", True)
        sp = A.flat(top_slot, 4, int(nsweeps), dev, "top_slot", True)
        L.check(self.ctx.lib.msc_sweep_blocked(self._h, view._h, self._cols(cols), row0, n,
                                               row0 if row_id0 is None else row_id0, zp,
                                               int(nsweeps), int(seed), int(sweep), tp, sp))

    # split-merge Metropolis-Hastings proposals --------------------------------
    def split_merge(self, view, z, seed, sweep, nproposals=1, launch_iters=2, log=None, trace=None, proposed=None,
                    counters=None, row0=0, nrows=None, row_id0=None, cols=None):
        """nproposals split-merge proposals on the device, proposal p with the sweep counter sweep + p
        (msc_split_merge).  All outputs are optional device tensors: log float64 [nproposals, 8] = {i, j, kind (0 split,
        1 merge, 2 void), n_0, n_1, log q, log A, accepted}; trace int32 [nproposals, nrows], z after every proposal;
        proposed int32 [nproposals, nrows], the proposed pair labels (-1 outside the two groups); counters 64-bit integer
        [5] = {splits proposed, accepted, merges proposed, accepted, void}, added to."""
        self._drop_subsets()
        row0, n, zp = self._bind(view, row0, nrows, z, True)      # (a null z is the library's to refuse)
        if not 0 <= int(nproposals) < (1 << 32) or not 0 <= int(launch_iters) < (1 << 32):
            raise ValueError("nproposals and launch_iters must be in [0, 2^32)")
        dev, np_ = self.ctx.torch_device, int(nproposals)
        L.check(self.ctx.lib.msc_split_merge(self._h, view._h, self._cols(cols), row0, n,
                                             row0 if row_id0 is None else row_id0, zp, np_, int(launch_iters),
                                             int(seed), int(sweep), A.flat(log, torch.float64, 8 * np_, dev, "log", True),
                                             A.flat(trace, torch.int32, np_ * n, dev, "trace", True),
                                             A.flat(proposed, torch.int32, np_ * n, dev, "proposed", True),
                                             A.flat(counters, 8, 5, dev, "counters", True)))

    def split_merge_tables(self):
        """{"logw": float32[2], feature index: float32[nslices, 2]}: views onto theta* of the last proposal made -- the
        two pair slots' log weights and slices (msc_split_merge_tables; the slices are blocked_tables()'s)"""
        return self._tables(self.ctx.lib.msc_split_merge_tables, 2)

    def sweep_step_stats(self):
        """(steps run launch by launch, steps run as one graph launch)"""
        e, g = C.c_uint64(), C.c_uint64()
        L.check(self.ctx.lib.msc_sweep_step_stats(self._h, C.byref(e), C.byref(g)))
        return e.value, g.value

    # multi-GPU hook ---------------------------------------------------------
    def reduce_buffers(self):
        """(int64 tensor, float64 tensor) aliasing the additive tables, for all_reduce(SUM)."""
        pi, ni, pf, nf = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        L.check(self.ctx.lib.msc_state_reduce_buffers(self._h, C.byref(pi), C.byref(ni), C.byref(pf), C.byref(nf)))
        return (_alias_tensor(pi.value, ni.value, torch.int64, self.ctx.torch_device),
                _alias_tensor(pf.value, nf.value, torch.float64, self.ctx.torch_device))

    def commit_reduce(self):
        self._drop_subsets()
        L.check(self.ctx.lib.msc_state_commit_reduce(self._h))

    def reduce_pack(self):
        """both additive tables as ONE float64 tensor (a copy the state owns; one launch): all_reduce it in place, then
        reduce_unpack() and commit_reduce()"""
        p, n = C.c_void_p(), C.c_size_t()
        L.check(self.ctx.lib.msc_state_reduce_pack(self._h, C.byref(p), C.byref(n)))
        return _alias_tensor(p.value, n.value, torch.float64, self.ctx.torch_device)

    def reduce_unpack(self):
        self._drop_subsets()
        L.check(self.ctx.lib.msc_state_reduce_unpack(self._h))

    def set_sweep_rows(self, global_rows):
        """rows of the WHOLE dataset when this state sweeps a shard through a view of its own (msc_state_set_sweep_rows)"""
        L.check(self.ctx.lib.msc_state_set_sweep_rows(self._h, int(global_rows)))

    def col_bound_count(self):
        """how many column bounds the features take: gp / bnb one, dm dim + 1, every other family none"""
        return sum(1 if fam in (L.GP, L.BNB) else dim + 1 if fam == L.DM else 0 for fam, dim in self.features)

    def col_bounds(self, view, cols=None):
        """this view's column bounds for the state's features, in feature order (msc_state_col_bounds): uint32 array of
        col_bound_count() values -- a gp / bnb column's maximum; a dm column's category maxima, then its largest row total"""
        self._bound_view = view          # (the library keeps no reference to a view: this object does, for the last one bound)
        out = np.zeros(self.col_bound_count(), dtype=np.uint32)
        L.check(self.ctx.lib.msc_state_col_bounds(self._h, view._h, self._cols(cols), out.ctypes.data_as(C.c_void_p),
                                                  out.size))
        return out

    def set_col_bounds(self, bounds):
        """the WHOLE dataset's column bounds (the elementwise max of every shard view's col_bounds) when this state sweeps
        a shard through a view of its own (msc_state_set_col_bounds); None restores the view's own"""
        if bounds is None:
            L.check(self.ctx.lib.msc_state_set_col_bounds(self._h, None, 0))
            return
        b = np.ascontiguousarray(np.asarray(bounds), dtype=np.uint32)
        L.check(self.ctx.lib.msc_state_set_col_bounds(self._h, b.ctypes.data_as(C.c_void_p), b.size))

    # grid hyper-parameter inference (msc_hp_grid_*; common_amd/hypers.py builds the grids upstream's way) -----------
    def hp_grid(self, f, blocks, logprior=None):
        """an HpGrid of feature f: `blocks` = [npoints, msc_hp_floats] floats (or a list of hp dicts, packed with
        pack_hp), `logprior` = npoints float64 values or None"""
        fam, dim = self.features[f]
        if not isinstance(blocks, np.ndarray):
            blocks = np.stack([pack_hp(fam, b, dim) for b in blocks]) if len(blocks) else np.zeros((0, 0), np.float32)
        return HpGrid(self, int(f), blocks, logprior)

    def crp_grid(self, alphas, logprior=None):
        """an HpGrid of the CRP concentration alpha (every value > 0)"""
        return HpGrid(self, L.HP_CLUSTER, np.asarray(alphas, dtype=np.float32).reshape(-1, 1), logprior)

    def hp_gibbs(self, grids, seed, sweep, slots=None, want_scores=False):
        """one grid Gibbs step over `grids` (at most one per feature, one crp_grid): score, add the prior, draw, install
        (msc_hp_grid_gibbs; one host synchronisation).  -> chosen indices (numpy uint32, one per grid), and with
        want_scores the float64 tensors of prior + likelihood per grid"""
        self._drop_subsets()
        grids = list(grids)
        for g in grids:
            if g.state is not self or not g._h:
                raise ValueError("every grid must be a live grid of this state")
        hs = (C.c_void_p * len(grids))(*[g._h.value for g in grids])
        chosen = np.zeros(len(grids), dtype=np.uint32)
        scores, sp = None, None
        if want_scores:
            scores = [torch.empty(g.npoints, dtype=torch.float64, device=self.ctx.torch_device) for g in grids]
            sp = (C.c_void_p * len(grids))(*[t.data_ptr() for t in scores])
        L.check(self.ctx.lib.msc_hp_grid_gibbs(self._h, hs, len(grids), self._slots(slots), int(seed), int(sweep),
                                               chosen.ctypes.data_as(C.c_void_p), sp))
        return (chosen, scores) if want_scores else chosen

    # slice sampling (msc_hp_slice / msc_theta_slice; common_amd/hypers.py builds the coordinates upstream's way) -------
    _PRIORS = {"flat": L.PRIOR_FLAT, "exponential": L.PRIOR_EXPONENTIAL, "normal": L.PRIOR_NORMAL,
               "noninf_beta": L.PRIOR_NONINF_BETA}

    @classmethod
    def _slice_coord_array(cls, coords):
        """hp_slice's entry dicts -> the msc_slice_coord array the library takes (ChainEnsemble.hp_slice shares it)"""
        arr = (L.SliceCoord * max(1, len(coords)))()
        for i, c in enumerate(coords):
            f = c["feature"]
            prior = c.get("prior", L.PRIOR_FLAT)
            arr[i] = L.SliceCoord(L.HP_CLUSTER if f in ("alpha", L.HP_CLUSTER) else int(f), int(c.get("coord", 0)),
                                  float(c["width"]), cls._PRIORS.get(prior, prior) if isinstance(prior, str) else
                                  int(prior), float(c.get("a", 0.0)), float(c.get("b", 0.0)), int(c.get("partner", 0)))
        return arr

    def hp_slice(self, coords, seed, sweep, slots=None):
        """one slice step of each entry of `coords` (msc_hp_slice; one host synchronisation).  An entry is a dict with
        "feature" (a state feature, or "alpha" / L.HP_CLUSTER), "coord" (float index in the hp block; 0 for alpha),
        "width", and optionally "prior" ("flat", "exponential", "normal", "noninf_beta" or an L.PRIOR_* value), "a"
        (lambda | mu), "b" (sigma2) and "partner" (noninf_beta).  slots: uint8 device mask of the counted groups (default:
        the non-empty ones).  -> (installed values float32, evaluations uint32), one per entry"""
        self._drop_subsets()
        coords = list(coords)
        arr = self._slice_coord_array(coords)
        values = np.zeros(len(coords), dtype=np.float32)
        evals = np.zeros(len(coords), dtype=np.uint32)
        L.check(self.ctx.lib.msc_hp_slice(self._h, arr, len(coords), self._slots(slots), int(seed), int(sweep),
                                          values.ctypes.data_as(C.c_void_p), evals.ctypes.data_as(C.c_void_p)))
        return values, evals

    def theta_slice(self, tparams, seed, sweep, slots=None):
        """one slice step of the p of every counted slot of the bbnc features in `tparams` = {feature: {"p": width}}, as
        downstream's theta kernel takes it (msc_theta_slice; one host synchronisation).  -> {feature: evaluations}"""
        self._drop_subsets()
        feats = [int(f) for f in tparams]
        for f in feats:
            if set(tparams[f]) != {"p"}:
                raise ValueError("feature %d: a bbnc group has one parameter, 'p'" % f)
        fs = np.array(feats, dtype=np.uint32)
        ws = np.array([tparams[f]["p"] for f in feats], dtype=np.float32)
        evals = np.zeros(len(feats), dtype=np.uint64)
        L.check(self.ctx.lib.msc_theta_slice(self._h, fs.ctypes.data_as(C.c_void_p), ws.ctypes.data_as(C.c_void_p),
                                             len(feats), self._slots(slots), int(seed), int(sweep),
                                             evals.ctypes.data_as(C.c_void_p)))
        return {f: int(e) for f, e in zip(feats, evals)}

    # the log joint (msc_score_joint) ------------------------------------------------------------------------------------
    @classmethod
    def _joint_priors(cls, priors):
        """score_joint's `priors` -> (the msc_slice_coord array or None, its length): None, a list of hp_slice's entry
        dicts (the width may be left out: a prior has none), or what carries one as .coords (hypers.FeatureHpSlice,
        EnsembleHpSlice).  ChainEnsemble.score_joint shares it."""
        if priors is None:
            return None, 0
        coords = list(getattr(priors, "coords", priors))
        for c in coords:
            if not isinstance(c, dict) or "feature" not in c:
                raise ValueError("priors must be hp_slice's entry dicts (or carry them as .coords), not %r" % (c,))
        if not coords:
            return None, 0
        return cls._slice_coord_array([dict(c, width=c.get("width", 1.0)) for c in coords]), len(coords)

    def score_joint(self, priors=None, slots=None, out=None):
        """log p(X, z | hp, alpha) of the state and its parts: a float64 device tensor [nfeatures + 3] = (total,
        score_assignment, the features' summed score_data over the counted groups ..., the hyper-priors' sum), all in
        double on the device (msc_score_joint; asynchronous, changes nothing).  priors: hp_slice's entries whose priors
        are added at the coordinates' current values (default: none, the last part is 0).  slots: uint8 device mask of
        the counted groups (default: the non-empty ones)."""
        arr, n = self._joint_priors(priors)
        width = len(self.features) + 3
        if out is None:
            out = torch.empty(width, dtype=torch.float64, device=self.ctx.torch_device)
        op = A.flat(out, torch.float64, width, self.ctx.torch_device, "out")
        L.check(self.ctx.lib.msc_score_joint(self._h, arr, n, self._slots(slots), op))
        return out

    # posterior predictive sampling -------------------------------------------
    _PRED_DTYPES = {L.BB: torch.uint8, L.BBNC: torch.uint8, L.GP: torch.uint32, L.BNB: torch.uint32, L.DD: torch.int32,
                    L.NICH: torch.float32, L.NIW: torch.float32}

    # row predictive log-density (msc_score_marginal) ---------------------------------------------------------------
    def predictive_logp(self, view, z=None, row0=0, nrows=None, cols=None, out=None, want_map=False, given=None):
        """log p(x_r | state) of rows [row0, row0 + nrows): the log-sum-exp over the groups of log pseudocount + the
        row's summed score_value, minus log(n_r + alpha) -- float32 device tensor of nrows entries (msc_score_marginal;
        the [nrows, K] matrix is not written where a fused kernel takes the state).  z (int32 device tensor): leave-one-out,
        an id outside [0, K) is unassigned.  want_map: -> (logp, map, map_logresp), the arg-max group of every row (lowest
        index among exact ties) and its log responsibility.
        given=[f, ...]: the CONDITIONAL log density of the row's other observed entries given features f, ..., as
        logp(all) - logp(subset(given)); the subset state is kept until a table of this state changes.  cols then has to
        be None or list every feature's column (the subset reads the given features' entries of it)."""
        row0, n, zp = self._bind(view, row0, nrows, z, True)
        dev = self.ctx.torch_device
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=dev)
        op = A.flat(out, torch.float32, n, dev, "out")
        mp = lr = None
        if want_map:
            mp = torch.empty(n, dtype=torch.int32, device=dev)
            lr = torch.empty(n, dtype=torch.float32, device=dev)
        L.check(self.ctx.lib.msc_score_marginal(self._h, view._h, self._cols(cols), row0, n, zp, 0, op,
                                                A.ptr(mp) if want_map else None, A.ptr(lr) if want_map else None))
        if given is not None:
            given = [int(f) for f in given]
            sub = self._subset_cached(given)
            all_cols = list(range(len(self.features))) if cols is None else [int(c) for c in cols]
            denom = sub.predictive_logp(view, z=z, row0=row0, nrows=n, cols=[all_cols[f] for f in given])
            out[:n] -= denom
        return (out, mp, lr) if want_map else out

    def subset(self, features):
        """a new State of the same K holding only `features` (indices into this state's, in the order given), with their
        hp, suff-stats (bbnc's p included: it is a field of the record), the group counts and alpha copied (a host round
        trip of K records a feature)"""
        feats = [int(f) for f in features]
        for f in feats:
            if not 0 <= f < len(self.features):
                raise ValueError("feature %d outside the state (%d features)" % (f, len(self.features)))
        sub = State(self.ctx, [self.features[f] for f in feats], self.K)
        for i, f in enumerate(feats):
            a = self.get_hp(f)
            L.check(self.ctx.lib.msc_state_set_hp(sub._h, i, a.ctypes.data_as(C.c_void_p), a.size))
            sub.set_ss(i, self.get_ss(f))
        sub.set_group_counts(self.get_group_counts())
        sub.set_alpha(self.get_alpha())
        return sub

    def _subset_cached(self, feats):
        cache = self.__dict__.setdefault("_subsets", {})
        key = tuple(feats)
        if key not in cache:
            cache[key] = self.subset(feats)
        return cache[key]

    def _drop_subsets(self):
        """every method that changes a table (hp, suff-stats, counts, alpha) calls this first: the subset states that
        predictive_logp(given=) keeps were copies of the tables as they stood"""
        subs = self.__dict__.pop("_subsets", None)
        if subs:
            for sub in subs.values():
                sub.close()

    def sample_predictive(self, view, z=None, seed=0, sweep=0, masked_only=False, features=None, row0=0, nrows=None,
                          row_id0=None, cols=None, out=None):
        """Posterior predictive draws for rows [row0, row0 + nrows) of the view (msc_sample_predictive).
        z: int32 device tensor of the rows' groups, or None to draw each row's group from the CRP term plus the scores of
        its observed entries.  features: state feature indices to draw (default: all).  out: optional dict feature ->
        device tensor to write into (rows that are skipped keep what it held).  -> (dict feature -> device tensor of
        nrows values -- [nrows, dim] for niw --, int32 device tensor of the groups used)."""
        row0, n, zp = self._bind(view, row0, nrows, z, True)
        if row0 + n > view.nrows:                      # (outputs are sized before the call: not left to the library)
            raise ValueError("rows [%d, %d) outside the view (%d rows)" % (row0, row0 + n, view.nrows))
        feats = list(range(len(self.features))) if features is None else [int(f) for f in features]
        for f in feats:
            if not 0 <= f < len(self.features):
                raise ValueError("feature %d outside the state (%d features)" % (f, len(self.features)))
            if self.features[f][0] == L.DM:
                raise L.MicroscopesHipError(-4, "feature %d: dm has no sample_value upstream" % f)
            if self.features[f][0] not in self._PRED_DTYPES:
                raise L.MicroscopesHipError(-4, "feature %d: the family has no values to draw" % f)
        out = dict(out or {})
        ptrs = (C.c_void_p * len(self.features))()
        for f in feats:
            fam, dim = self.features[f]
            shape = (n, dim) if fam == L.NIW else (n,)
            dt = self._PRED_DTYPES[fam]
            t = out.get(f)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=self.ctx.torch_device)
            elif not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError("out[%d] must be a contiguous %s device tensor of shape %s" % (f, dt, shape))
            out[f] = t
            ptrs[f] = A.flat(t, dt, 0, self.ctx.torch_device, "out[%d]" % f) if n else None
        groups = torch.full((n,), -1, dtype=torch.int32, device=self.ctx.torch_device)
        L.check(self.ctx.lib.msc_sample_predictive(self._h, view._h, self._cols(cols), row0, n,
                                                   int(row0 if row_id0 is None else row_id0), zp,
                                                   A.ptr(groups) if n else None,
                                                   L.PRED_MASKED_ONLY if masked_only else 0, int(seed), int(sweep), ptrs))
        return {f: out[f] for f in feats}, groups

    def impute(self, view, z=None, seed=0, sweep=0, **kw):
        """sample_predictive with masked_only=True: masked entries drawn, observed ones copied (the completed columns)."""
        return self.sample_predictive(view, z=z, seed=seed, sweep=sweep, masked_only=True, **kw)

    def close(self):
        self._drop_subsets()                            # (the subset states predictive_logp(given=) kept)
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):           # (see DataView.close)
                # (refused while the state is a member of a live ChainEnsemble's handle: the state stays open)
                L.check(self.ctx.lib.msc_state_destroy(self._h))
            for g in list(getattr(self, "_grids", ())):  # (the library frees a state's grids with it)
                g._h = None
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HpGrid(object):
    """npoints hyper-parameter blocks of one feature (or alpha values, feature = HP_CLUSTER) and their log-prior,
    uploaded once and owned by the state (msc_hp_grid_create)"""

    def __init__(self, state, feature, blocks, logprior=None):
        import weakref
        b = np.ascontiguousarray(blocks, dtype=np.float32)
        if b.ndim != 2:
            raise ValueError("blocks must be [npoints, floats per block]")
        lp = None if logprior is None else np.ascontiguousarray(logprior, dtype=np.float64)
        if lp is not None and lp.shape != (b.shape[0],):
            raise ValueError("logprior must hold one value per grid point")
        self.state, self.feature, self.npoints = state, feature, int(b.shape[0])
        self.blocks, self.logprior = b, lp
        h = C.c_void_p()
        L.check(state.ctx.lib.msc_hp_grid_create(state._h, feature, b.ctypes.data_as(C.c_void_p), b.shape[1],
                                                 self.npoints, None if lp is None else lp.ctypes.data_as(C.c_void_p),
                                                 C.byref(h)))
        self._h = h
        if not hasattr(state, "_grids"):
            state._grids = weakref.WeakSet()
        state._grids.add(self)

    def scores(self, slots=None, out=None):
        """float64 [npoints] device tensor: each point's log marginal likelihood of the groups (no prior); slots: uint8
        device mask of the counted groups (default: the non-empty ones).  Asynchronous (msc_hp_grid_score)."""
        if not self._h:
            raise ValueError("grid is closed")
        if out is None:
            out = torch.empty(self.npoints, dtype=torch.float64, device=self.state.ctx.torch_device)
        op = A.flat(out, torch.float64, self.npoints, self.state.ctx.torch_device, "out")
        L.check(self.state.ctx.lib.msc_hp_grid_score(self._h, self.state._slots(slots), op))
        return out

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.state, "_h", None) and getattr(self.state.ctx, "_h", None):
                self.state.ctx.lib.msc_hp_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZMatrix(object):
    """Co-clustering counts of m chosen rows over assignment samples, accumulated on the device (msc_zmatrix_*): the
    reference's query.zmatrix restricted to `rows` (None: all n, in order).  Every label must lie in [0, nlabels)."""

    def __init__(self, ctx, n, nlabels, rows=None):
        self.ctx, self.n, self.nlabels = ctx, int(n), int(nlabels)
        rp = None
        if rows is None:
            self.m = self.n
        else:
            r = np.asarray(rows)
            if r.ndim != 1 or not (np.issubdtype(r.dtype, np.integer) or r.size == 0):
                raise ValueError("rows must be a 1-D array of row indices")
            if r.size and (r.min() < 0 or r.max() >= self.n):
                raise ValueError("rows must lie in [0, n)")
            rp = np.ascontiguousarray(r, dtype=np.uint32)
            self.m = int(rp.size)
        self._rows = rp
        h = C.c_void_p()
        L.check(ctx.lib.msc_zmatrix_create(ctx._h, self.n, None if rp is None else rp.ctypes.data_as(C.c_void_p), self.m,
                                           self.nlabels, C.byref(h)))
        self._h = h

    def _check_open(self):
        if not getattr(self, "_h", None):
            raise ValueError("ZMatrix is closed")

    def _vectors(self, z, name="z"):
        """(tensor, S, ld) of assignment vectors given as add takes them"""
        self._check_open()
        return A.vectors(z, self.ctx.torch_device, name, self.n)

    def add(self, z):
        """stage assignment vectors: an int32 device tensor [n] or [S, n] whose rows are contiguous (row stride >= n).
        Asynchronous; z may be overwritten by the next work on the stream (msc_zmatrix_add)."""
        z2, S, ld = self._vectors(z)
        if S == 0:
            return
        L.check(self.ctx.lib.msc_zmatrix_add(self._h, A.ptr(z2), S, ld))

    def partition_sums(self, cands):
        """Candidate partitions against the counts (msc_zmatrix_partition_sums).  cands: an int32 device tensor [n] or
        [ncand, n] laid out as add takes samples; only equality of labels matters, any int32 value is a label.  Returns
        (w int64 [ncand, m], size int32 [ncand, m]): size[c, a] = the selected rows that c puts with row a (a included),
        w[c, a] = the sum of counts()[a, b] over those rows.  Exact; flushes the staged samples first."""
        c2, nc, ld = self._vectors(cands, "cands")
        dev = self.ctx.torch_device
        w = torch.empty((nc, self.m), dtype=torch.int64, device=dev)
        size = torch.empty((nc, self.m), dtype=torch.int32, device=dev)
        L.check(self.ctx.lib.msc_zmatrix_partition_sums(self._h, A.ptr(c2), nc, ld, A.ptr(w), A.ptr(size)))
        return w, size

    def partition_loss(self, cands):
        """Posterior expected losses of candidate partitions (msc_zmatrix_partition_loss; cands as for partition_sums).
        Returns (binder_num int64 [ncand], vi_lb float64 [ncand], valid): binder_num / valid is the expected number of
        mis-paired pairs under Binder's loss (the argmin is Dahl's least-squares clustering); vi_lb is Wade and
        Ghahramani's lower bound on the expected variation of information less its candidate-independent term, which
        counts do not determine; valid is the number of valid samples, counts()[0, 0].  Synchronises to read valid."""
        c2, nc, ld = self._vectors(cands, "cands")
        dev = self.ctx.torch_device
        binder = torch.empty(nc, dtype=torch.int64, device=dev)
        vi = torch.empty(nc, dtype=torch.float64, device=dev)
        valid = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(self.ctx.lib.msc_zmatrix_partition_loss(self._h, A.ptr(c2), nc, ld, A.ptr(binder), A.ptr(vi),
                                                        A.ptr(valid)))
        self.ctx.synchronize()
        return binder, vi, int(valid.item())

    def partition_refine(self, starts, max_sweeps=20, max_clusters=None, order=None):
        """Greedy refinement of partitions under Binder's loss (msc_zmatrix_partition_refine; starts as partition_sums
        takes candidates).  From each start rows move one at a time to the cluster, or into a new one, that lowers
        binder_num most, sweep after sweep (positions ascending, or in `order`, a permutation of [0, m)), until a sweep
        moves nothing or max_sweeps have run.  max_clusters: the most clusters a partition may hold on the way (None:
        min(m, ZMATRIX_REFINE_MAX_CLUSTERS)); a start that holds more raises ValueError.  Returns device tensors (labels
        int32 [nstarts, m] over the selected rows, numbered by first row; binder_num int64 [nstarts]; sweeps int32
        [nstarts], the last one that moved nothing included; moves int64 [nstarts]), bit-equal to
        query.refine_partition on the host.  Asynchronous; flushes the staged samples first."""
        s2, ns, ld = self._vectors(starts, "starts")
        if max_clusters is None:
            max_clusters = min(self.m, L.ZMATRIX_REFINE_MAX_CLUSTERS)
        max_sweeps, max_clusters = int(max_sweeps), int(max_clusters)
        if max_sweeps < 0 or max_sweeps >= 2 ** 32:
            raise ValueError("max_sweeps must lie in [0, 2^32)")
        if max_clusters < 1 or max_clusters > self.m:
            raise ValueError("max_clusters must lie in [1, m = %d]" % self.m)
        o = self._order(order)
        dev = self.ctx.torch_device
        if ns and self.m <= L.ZMATRIX_REFINE_MAX_ROWS and max_clusters <= L.ZMATRIX_REFINE_MAX_CLUSTERS:
            # the clusters of every start over the selected rows, counted before anything is launched
            sel = s2.reshape(ns, -1) if self._rows is None else \
                s2.reshape(ns, -1)[:, torch.from_numpy(self._rows.astype(np.int64)).to(dev)]
            srt = torch.sort(sel, dim=1).values
            most = int(((srt[:, 1:] != srt[:, :-1]).sum(dim=1) + 1).max())
            if most > max_clusters:
                raise ValueError("a start holds %d clusters, more than max_clusters = %d" % (most, max_clusters))
        labels = torch.empty((ns, self.m), dtype=torch.int32, device=dev)
        binder = torch.empty(ns, dtype=torch.int64, device=dev)
        sweeps = torch.empty(ns, dtype=torch.int32, device=dev)
        moves = torch.empty(ns, dtype=torch.int64, device=dev)
        L.check(self.ctx.lib.msc_zmatrix_partition_refine(
            self._h, A.ptr(s2), ns, ld, max_sweeps, max_clusters, None if o is None else o.ctypes.data_as(C.c_void_p),
            A.ptr(labels), A.ptr(binder), A.ptr(sweeps), A.ptr(moves)))
        return labels, binder, sweeps, moves

    @property
    def nsamples(self):
        self._check_open()
        v = C.c_uint64()
        L.check(self.ctx.lib.msc_zmatrix_nsamples(self._h, C.byref(v)))
        return int(v.value)

    def _order(self, order):
        if order is None:
            return None
        o = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order)
        if o.shape != (self.m,) or not np.issubdtype(o.dtype, np.integer) or \
                (o.size and (o.min() < 0 or o.max() >= self.m)) or np.unique(o).size != self.m:
            raise ValueError("not a valid permutation")
        return np.ascontiguousarray(o, dtype=np.uint32)

    def _write(self, fn, order, out, dtype):
        self._check_open()
        o = self._order(order)
        m = self.m
        if out is None:
            out = torch.empty((m, m), dtype=dtype, device=self.ctx.torch_device)
        elif not isinstance(out, torch.Tensor) or out.dim() != 2:
            raise ValueError("out must be a 2-D tensor of at least [m, m] = [%d, %d]" % (m, m))
        op, ld = A.matrix(out, dtype, m, m, self.ctx.torch_device, "out")
        L.check(fn(self._h, None if o is None else o.ctypes.data_as(C.c_void_p), op, ld))
        return out[:m, :m] if out.shape != (m, m) else out

    def counts(self, order=None, out=None):
        """int32 [m, m] device tensor holding the exact u32 counts (optionally reordered: out[a, b] = C[order[a], order[b]])"""
        return self._write(self.ctx.lib.msc_zmatrix_counts, order, out, torch.int32)

    def result(self, order=None, out=None):
        """float32 [m, m] device tensor: counts / nsamples, as the reference's zmatrix computes it"""
        return self._write(self.ctx.lib.msc_zmatrix_result, order, out, torch.float32)

    def linkage(self):
        """scipy's single linkage of 1 - result() (query.zmatrix_linkage), float64 [m - 1, 4].  result() is materialised
        into a temporary first: m x m floats on top of the accumulator's tiles."""
        from . import query
        return query.zmatrix_linkage(self.result(), ctx=self.ctx)

    def block_ordering(self):
        """query.zmatrix_heuristic_block_ordering of result(): result(order=zm.block_ordering()) is the matrix in block
        order, with nothing quadratic crossing to the host.  result() is materialised into a temporary first: m x m
        floats on top of the accumulator's tiles."""
        from . import query
        return query.zmatrix_heuristic_block_ordering(self.result(), ctx=self.ctx)

    def reset(self):
        self._check_open()
        L.check(self.ctx.lib.msc_zmatrix_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            # (as DataView.close: a handle whose context is gone is not handed to the library)
            if getattr(self.ctx, "_h", None):
                self.ctx.lib.msc_zmatrix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceBuffer(object):
    """owner of a msc_device_alloc* buffer: freed when the last tensor aliasing it is gone"""

    def __init__(self, ctx, ptr):
        self.ctx, self.ptr = ctx, ptr
        ctx._buffers.add(self)

    def __del__(self):
        try:
            if self.ptr and getattr(self.ctx, "_h", None):
                self.ctx.lib.msc_device_free(self.ctx._h, C.c_void_p(self.ptr))
        except Exception:
            pass
        self.ptr = None


class _CudaArrayView(object):
    def __init__(self, ptr, n, typestr, owner=None):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}
        self._owner = owner          # (torch keeps this object alive as long as the tensor's storage)


def _alias_tensor(ptr, n, dtype, device, owner=None):
    if n == 0:
        return torch.empty(0, dtype=dtype, device=device)
    typestr = {torch.int64: "<i8", torch.float64: "<f8", torch.uint8: "|u1", torch.float32: "<f4",
               torch.int32: "<i4"}[dtype]
    return torch.as_tensor(_CudaArrayView(ptr, n, typestr, owner), device=device)


def _relation_blocks(ctx, shape, zs, ngroups, pos, ncells):
    """msc_relation_blocks for both relation views: pos None = dense"""
    nd = len(shape)
    if len(zs) != nd or len(ngroups) != nd:
        raise ValueError("one assignment vector and one cluster count per dimension")
    zp = (C.c_void_p * nd)(*[A.flat(z, torch.int32, n, ctx.torch_device, "an assignment vector") for z, n in zip(zs, shape)])
    out = torch.empty(max(ncells, 1), dtype=torch.int32, device=ctx.torch_device)
    L.check(ctx.lib.msc_relation_blocks(ctx._h, nd, (C.c_uint64 * nd)(*shape), zp, (C.c_uint32 * nd)(*[int(k) for k in ngroups]),
                                        None if pos is None else A.ptr(pos), ncells, A.ptr(out)))
    return out[:ncells]


def _relation_slice_scores(ctx, shape, scores, off, dim, ngroups, ncells, seg, ids):
    """msc_relation_slice_scores for both relation views: seg = ids = None = dense.  A slice reduction indexes score
    columns up to prod(ngroups): the matrix must have them all (the kernel skips and reports an offset past the row,
    MSC_EDEVICE, but a consistent caller never gets there)"""
    nd, dev = len(shape), ctx.torch_device
    if len(ngroups) != nd or not 0 <= int(dim) < nd:
        raise ValueError("one cluster count per dimension and a dimension inside the relation")
    nblocks = stride = 1
    for d, k in enumerate(ngroups):
        nblocks *= int(k)
        if d > dim:
            stride *= int(k)
    sp, ld = A.matrix(scores, torch.float32, ncells, nblocks, dev, "scores")
    op = A.flat(off, torch.int32, ncells, dev, "off")
    out = torch.empty((shape[dim], int(ngroups[dim])), dtype=torch.float32, device=dev)
    L.check(ctx.lib.msc_relation_slice_scores(ctx._h, sp, ld, nd, (C.c_uint64 * nd)(*shape), dim,
                                              None if seg is None else A.ptr(seg), None if ids is None else A.ptr(ids), op,
                                              int(ngroups[dim]), stride, shape[dim], A.ptr(out), out.stride(0)))
    return out


class RelationView(object):
    """A relation (numpy N-d array, optionally masked) on the device: a one-feature DataView whose rows
    are the relation's cells in row-major order (microscopes/common/relation/dataview.pyx numpy_dataview).
    `blocks(zs, ngroups)` maps per-dimension cluster assignments to the cell's block (= group) index."""

    def __init__(self, ctx, array):
        if array is None or array.ndim < 1:
            raise ValueError("need an N-d array")
        if any(int(d) == 0 for d in array.shape):
            raise ValueError("empty dims not allowed")              # relation/_dataview.pyx:33-34
        self.ctx = ctx
        self.shape = tuple(int(s) for s in array.shape)
        data = np.ascontiguousarray(np.ma.getdata(array)).reshape(-1)
        rec = np.zeros(data.shape[0], dtype=[("f0", data.dtype)])
        rec["f0"] = data
        if hasattr(array, "mask"):
            m = np.zeros(data.shape[0], dtype=[("f0", np.bool_)])
            m["f0"] = np.ascontiguousarray(np.ma.getmaskarray(array)).reshape(-1)
            rec = np.ma.masked_array(rec, mask=m)
        self.cells = DataView.from_recarray(ctx, rec)

    def blocks(self, zs, ngroups):
        """zs: one int32 device tensor per dimension; ngroups: clusters per dimension -> int32 [ncells]"""
        return _relation_blocks(self.ctx, self.shape, zs, ngroups, None, self.cells.nrows)

    def slice_offsets(self, zs, ngroups, dim):
        """block index of every cell with dimension `dim`'s cluster taken as 0 (-1 where another entity of the cell is
        unassigned): the `off` of slice_scores.  zs[dim] is ignored."""
        zs = list(zs)
        zs[dim] = torch.zeros(self.shape[dim], dtype=torch.int32, device=self.ctx.torch_device)
        return self.blocks(zs, ngroups)

    def slice_scores(self, scores, off, dim, ngroups):
        """irm's slice reduction (msc_relation_slice_scores): out[e, g] = sum over the cells of slice (dim, e) of the
        cell's score against block (g, the cell's other clusters).  scores: [ncells, >= prod(ngroups)] from
        State.score_value on self.cells; off: slice_offsets(...).  -> float32 [shape[dim], ngroups[dim]]"""
        return _relation_slice_scores(self.ctx, self.shape, scores, off, dim, ngroups, self.cells.nrows, None, None)


class SparseRelationView(object):
    """A sparse 2-D relation (scipy.sparse matrix) on the device -- microscopes/common/relation/dataview.pyx
    sparse_2d_dataview over compressed_2darray (relation/dataview.hpp:420-578): only the stored entries are cells, in CSR
    order; their (row, column) positions travel with them.  Same operations as RelationView."""

    def __init__(self, ctx, rep):
        rows, cols = rep.shape
        if rows <= 0 or cols <= 0:
            raise ValueError("both dimensions must be positive")
        csr = rep.tocsr()
        csr.sort_indices()
        self.ctx = ctx
        self.shape = (int(rows), int(cols))
        self._csr = csr
        nnz = int(csr.nnz)
        rec = np.zeros(nnz, dtype=[("f0", csr.data.dtype)])
        rec["f0"] = csr.data
        self.cells = DataView.from_recarray(ctx, rec) if nnz else None
        row_of = np.repeat(np.arange(rows, dtype=np.uint32), np.diff(csr.indptr))
        pos = np.stack([row_of, csr.indices.astype(np.uint32)], axis=1)
        dev = ctx.torch_device
        self._pos = torch.from_numpy(np.ascontiguousarray(pos).view(np.int32).reshape(-1).copy()).to(dev)   # uint32 pairs
        # slices: rows of the CSR (dimension 0) and of its transpose (dimension 1), as cell ids
        order = np.argsort(csr.indices, kind="stable").astype(np.int32)
        colptr = np.concatenate([[0], np.cumsum(np.bincount(csr.indices, minlength=cols))]).astype(np.int32)
        self._seg = [torch.from_numpy(csr.indptr.astype(np.int32).copy()).to(dev), torch.from_numpy(colptr).to(dev)]
        self._ids = [torch.arange(nnz, dtype=torch.int32, device=dev), torch.from_numpy(order).to(dev)]

    def tocsr(self):
        return self._csr

    def nnz(self):
        return int(self._csr.nnz)

    def blocks(self, zs, ngroups):
        return _relation_blocks(self.ctx, self.shape, zs, ngroups, self._pos, self.nnz())

    def slice_offsets(self, zs, ngroups, dim):
        zs = list(zs)
        zs[dim] = torch.zeros(self.shape[dim], dtype=torch.int32, device=self.ctx.torch_device)
        return self.blocks(zs, ngroups)

    def slice_scores(self, scores, off, dim, ngroups):
        """out[e, g] = sum over the stored cells of row / column e of the cell's score against block (g, the other
        entity's cluster) -- msc_relation_slice_scores with the CSR rows (dim 0) or the transpose's (dim 1)"""
        return _relation_slice_scores(self.ctx, self.shape, scores, off, dim, ngroups, self.nnz(), self._seg[dim],
                                      self._ids[dim])
