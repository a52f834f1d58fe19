"""GPU: greedy refinement of partitions under the exact expected variation of information (msc_partition_refine_vi,
Context.partition_refine_vi, common_amd.query.refine_partition_vi / vi_estimate(refine=) on device tensors).  The gains
are integers from the table of msc_vi_table, so every comparison is against the plain numpy rule
(common_amd.query._refine_vi_host, which tests/test_refine_vi_cpu.py holds against the float64 expected VI), bit for bit:
labels, decrease, sweeps and moves.

Shapes: small planted data, 3-8 clusters with 0.2-0.3 noise.  m on both sides of a wave (63 | 64 | 65), of the finishing
kernel's workgroup (255 | 257) and of the id capacity (1030), with S = 17; S with a tail behind the sixteen waves'
stride and behind the 2, 4 and 8 samples a wave takes at a time, with m = 130.  Starts of one cluster, of m, of 64 and 65
(the last id of one 64-id slot, the first of the next), of 1024; samples of 1, 65 and 1024 clusters."""
import ctypes as C

import numpy as np
import pytest
import torch

import common_amd
from common_amd import query
from common_amd._lib import REFINE_VI_MAX_CLUSTERS, REFINE_VI_MAX_ROWS, REFINE_VI_MAX_SAMPLES

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
EPS = 2.0 ** -52
NAMES = ("labels", "decrease", "sweeps", "moves")


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def planted(rng, S, m, k, noise):
    truth = rng.integers(0, k, m)
    A = np.tile(truth, (S, 1))
    flip = rng.random(A.shape) < noise
    A[flip] = rng.integers(0, k + 2, int(flip.sum()))
    return A.astype(np.int32)


def with_clusters(rng, m, k):
    """a random partition of m rows with exactly k clusters, labels anywhere around 0"""
    lab = np.concatenate([np.arange(k), rng.integers(0, k, m - k)])
    rng.shuffle(lab)
    names = rng.choice(np.arange(-3 * k, 3 * k), size=k, replace=False)
    return names[lab].astype(np.int32)


def some_starts(A, stripes=(64, 65)):
    """all-in-one, stripes (as many ids as the rows allow), and the first three samples themselves"""
    m = A.shape[1]
    out = [np.full(m, -9), A[0], A[1 % len(A)], A[2 % len(A)]] + [np.arange(m) % min(k, m) for k in stripes]
    return np.array(out, dtype=np.int32)


def against_host(ctx, A, starts, max_sweeps=20, max_clusters=None, order=None, workspace_bytes=0, a_dev=None, s_dev=None):
    """the device's four outputs against the numpy rule's, bit for bit; returns the device's as numpy"""
    A, starts = np.asarray(A), np.asarray(starts)
    got = ctx.partition_refine_vi(dev(ctx, A) if a_dev is None else a_dev, dev(ctx, starts) if s_dev is None else s_dev,
                                  max_sweeps, max_clusters, order, workspace_bytes)
    ctx.synchronize()
    got = [g.cpu().numpy() for g in got]
    cap = min(A.shape[1], REFINE_VI_MAX_CLUSTERS) if max_clusters is None else max_clusters
    want = query._refine_vi_host(A, starts, max_sweeps, cap, order)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.flatnonzero((g != w).reshape(len(starts), -1).any(axis=1)))
    return got


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 255, 257, 1030])
def test_rows(gpu_ctx, m):
    rng = np.random.default_rng(m)
    A = planted(rng, 17, m, min(m, 5), 0.25)
    starts = some_starts(A)
    if m <= 257:
        starts = np.concatenate([starts, np.arange(m, dtype=np.int32)[None]])          # singletons
        got = against_host(gpu_ctx, A, starts, max_clusters=m)
    else:
        got = against_host(gpu_ctx, A, starts, max_clusters=80)
        # a start of 1024 clusters, the most there may be: two sweeps of it
        against_host(gpu_ctx, A, with_clusters(rng, m, 1024)[None], max_sweeps=2, max_clusters=1024)
    if m >= 63:
        assert got[3].max() > 0 and (got[1] > 0).any()
    assert "k_vi_sweep<" in gpu_ctx.last_kernel("zmatrix")


@pytest.mark.parametrize("S", [1, 2, 15, 16, 17, 63, 64, 65, 130])
def test_samples(gpu_ctx, S):
    rng = np.random.default_rng(100 + S)
    m = 130
    A = planted(rng, S, m, 3 + S % 6, 0.2 + 0.1 * (S % 2))
    starts = np.concatenate([some_starts(A), np.arange(m, dtype=np.int32)[None] // 4])   # and 33 clusters
    against_host(gpu_ctx, A, starts)


def test_samples_of_one_65_and_1024_clusters(gpu_ctx):
    rng = np.random.default_rng(7)
    m = 1030
    A = planted(rng, 6, m, 6, 0.2)
    A[1], A[3], A[4] = 12345, with_clusters(rng, m, 65), with_clusters(rng, m, 1024)
    against_host(gpu_ctx, A, np.stack([np.zeros(m, dtype=np.int32), A[0], A[3]]), max_clusters=70)


def test_extreme_labels_padded_rows_and_order(gpu_ctx):
    rng = np.random.default_rng(8)
    S, m = 9, 200
    names = np.array([I32.min, I32.max, -1, 0, 1, I32.min + 1, I32.max - 1, 77, -77, 5], dtype=np.int64)
    A = names[planted(rng, S, m, 8, 0.3)].astype(np.int32)
    starts = some_starts(A)
    starts[4] = names[starts[4] % 10]
    assert A.min() == I32.min and A.max() == I32.max
    plain = against_host(gpu_ctx, A, starts)
    # ld > m with junk behind the rows, on both sides
    wide_a = np.full((S, m + 7), 123456789, dtype=np.int32)
    wide_a[:, :m] = A
    wide_s = np.full((len(starts), m + 3), -5, dtype=np.int32)
    wide_s[:, :m] = starts
    padded = against_host(gpu_ctx, A, starts, a_dev=dev(gpu_ctx, wide_a)[:, :m], s_dev=dev(gpu_ctx, wide_s)[:, :m])
    for x, y in zip(plain, padded):
        assert np.array_equal(x, y)
    order = rng.permutation(m)
    turned = against_host(gpu_ctx, A, starts, order=order)
    against_host(gpu_ctx, A, starts, order=torch.from_numpy(order), max_sweeps=1)
    assert not all(np.array_equal(x, y) for x, y in zip(plain, turned))


def test_capacity_that_binds_and_few_sweeps(gpu_ctx):
    rng = np.random.default_rng(9)
    S, m = 12, 90
    A = planted(rng, S, m, 4, 0.25)
    A[:, -5:] = 1000 + np.arange(5)                                         # alone in every sample: they leave while ids last
    starts = some_starts(A, stripes=(2, 3))
    loose = against_host(gpu_ctx, A, starts)
    few = [0, 4, 5]                                                         # one, two and three clusters
    tight = against_host(gpu_ctx, A, starts[few], max_clusters=4)           # five loners, at most three free ids
    assert (tight[0].max(axis=1) == 3).all() and (loose[0][few].max(axis=1) > 3).all()
    one = against_host(gpu_ctx, A, starts[:1], max_clusters=1)
    assert one[3].tolist() == [0] and one[2].tolist() == [1]
    first = against_host(gpu_ctx, A, starts, max_sweeps=1)
    assert first[2].tolist() == [1] * len(starts) and first[3].max() > 0
    # beyond 64 sweeps the host looks once per 64 whether any start still moves: the same outputs, the sweeps that ran
    late = against_host(gpu_ctx, A, starts, max_sweeps=200)
    for x, y in zip(loose, late):
        assert np.array_equal(x, y)
    none = against_host(gpu_ctx, A, starts, max_sweeps=0)
    assert none[2].tolist() == [0] * len(starts) and not none[3].any() and not none[1].any()
    assert np.array_equal(none[0], np.array([query._renumber(s) for s in starts]))


def cell_bytes(A, max_clusters):
    """what the contingency cells of one start take: 2 bytes x (sum of the samples' cluster counts) x max_clusters
    rounded up to 32, as include/microscopes_hip.h states"""
    return 2 * sum(np.unique(a).size for a in A) * ((max_clusters + 31) // 32 * 32)


def test_determinism_splits_and_budgets(gpu_ctx):
    rng = np.random.default_rng(10)
    S, m = 20, 150
    A = planted(rng, S, m, 6, 0.3)
    starts = np.concatenate([some_starts(A), A[3:6]])
    assert len(starts) == 9
    whole = against_host(gpu_ctx, A, starts)
    again = against_host(gpu_ctx, A, starts)
    for x, y in zip(whole, again):
        assert np.array_equal(x, y)
    ad, sd = dev(gpu_ctx, A), dev(gpu_ctx, starts)
    for cut in range(1, 9):
        lo, hi = gpu_ctx.partition_refine_vi(ad, sd[:cut]), gpu_ctx.partition_refine_vi(ad, sd[cut:])
        gpu_ctx.synchronize()
        for w, x, y in zip(whole, lo, hi):
            assert np.array_equal(w, np.concatenate([x.cpu().numpy(), y.cpu().numpy()])), cut
    one = cell_bytes(A, m)
    for budget in (one, one + 1, 4 * one, 5 * one - 1, 9 * one):
        for w, x in zip(whole, against_host(gpu_ctx, A, starts, workspace_bytes=budget)):
            assert np.array_equal(w, x), budget
    # a budget that one start exceeds: MSC_EUNSUPPORTED naming the bytes, the outputs untouched
    outs = [torch.full((9, m), 77, dtype=torch.int32, device=sd.device), torch.full((9,), 77, dtype=torch.int64, device=sd.device),
            torch.full((9,), 77, dtype=torch.int32, device=sd.device), torch.full((9,), 77, dtype=torch.int64, device=sd.device)]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = gpu_ctx.lib.msc_partition_refine_vi(gpu_ctx._h, ptr(ad), m, S, m, ptr(sd), m, 9, 20, m, None, one - 1, 0,
                                             *[ptr(o) for o in outs])
    assert rc == -4 and str(one) in gpu_ctx.lib.msc_last_error().decode()
    gpu_ctx.synchronize()
    assert all(bool((o == 77).all()) for o in outs)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.partition_refine_vi(ad, sd, workspace_bytes=one - 1)
    assert e.value.code == -4
    against_host(gpu_ctx, A, starts[:2])


def test_the_c_entry_point_itself(gpu_ctx):
    """MSC_EINVAL for what the header lists, MSC_EUNSUPPORTED for the caps before anything is read, nothing done when no
    output is asked for, and a sample of 1025 clusters found on the device: MSC_EDEVICE at the next wait, the context
    good afterwards"""
    rng = np.random.default_rng(2)
    m, S = REFINE_VI_MAX_CLUSTERS + 30, 4
    A = planted(rng, S, m, 5, 0.2)
    starts = some_starts(A)[:3]
    a, s = dev(gpu_ctx, A), dev(gpu_ctx, starts)
    lib, h, ptr = gpu_ctx.lib, gpu_ctx._h, lambda t: C.c_void_p(t.data_ptr())
    lab = torch.full((3, m), 77, dtype=torch.int32, device=a.device)

    def call(h=h, pa=ptr(a), lds=m, ns=S, rows=m, ps=ptr(s), ld=m, nst=3, sweeps=3, kc=40, order=None, ws=0, flags=0,
             outs=(ptr(lab), None, None, None)):
        o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32).ctypes.data_as(C.c_void_p)
        return lib.msc_partition_refine_vi(h, pa, lds, ns, rows, ps, ld, nst, sweeps, kc, o, ws, flags, *outs)
    assert call(h=None) == -1 and call(pa=None) == -1 and call(ps=None) == -1            # null arguments
    assert call(ns=0) == -1 and call(nst=0) == -1 and call(rows=0) == -1           # zero counts
    assert call(lds=m - 1) == -1 and call(ld=m - 1) == -1                                # a leading dimension below m
    bad = np.arange(m)
    bad[5] = 6
    assert call(order=bad) == -1                                                         # not a permutation
    bad[5] = m
    assert call(order=bad) == -1
    assert call(kc=0) == -1 and call(kc=m + 1) == -1                                     # max_clusters 0 or above m
    assert call(flags=1) == -1
    big = 1 << 20
    assert call(rows=REFINE_VI_MAX_ROWS + 1, lds=big, ld=big) == -4                      # the caps: nothing is read
    assert call(ns=REFINE_VI_MAX_SAMPLES + 1) == -4
    assert call(kc=REFINE_VI_MAX_CLUSTERS + 1) == -4
    assert call(outs=(None, None, None, None)) == 0                                      # nothing asked for
    gpu_ctx.synchronize()
    assert bool((lab == 77).all())
    assert call(order=np.arange(m)[::-1]) == 0
    gpu_ctx.synchronize()
    want = query._refine_vi_host(A, starts, 3, 40, np.arange(m)[::-1])
    assert np.array_equal(lab.cpu().numpy(), want[0])
    # the binding's own refusals, before the library is called
    for bad in (a.to(torch.int64), a.cpu(), a.T, a[:, ::2], a.to(torch.float32), a.reshape(2, 2, -1), a[:0], a[:, :0], None):
        with pytest.raises(ValueError):
            gpu_ctx.partition_refine_vi(bad, s)
    for bad in (s.to(torch.int64), s.cpu(), s.T, s[:, ::2], s.to(torch.float32), s[:0], s[:, :-1].contiguous(), None):
        with pytest.raises(ValueError):
            gpu_ctx.partition_refine_vi(a, bad)
    for kw in ({"max_clusters": 0}, {"max_clusters": m + 1}, {"max_sweeps": -1}, {"order": [0] * m}, {"workspace_bytes": -1}):
        with pytest.raises(ValueError):
            gpu_ctx.partition_refine_vi(a, s, **kw)
    with pytest.raises(ValueError, match="start holds 3 clusters, more than 2"):
        gpu_ctx.partition_refine_vi(a, dev(gpu_ctx, (np.arange(m) % 3).astype(np.int32)), max_clusters=2)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.partition_refine_vi(a, s, max_clusters=REFINE_VI_MAX_CLUSTERS + 1)
    assert e.value.code == -4
    # a sample of 1025 clusters
    many = A.copy()
    many[2] = with_clusters(rng, m, REFINE_VI_MAX_CLUSTERS + 1)
    md = dev(gpu_ctx, many)
    with pytest.raises(ValueError, match="sample holds 1025 clusters"):
        gpu_ctx.partition_refine_vi(md, s)
    with pytest.raises(ValueError, match="1025 clusters"):
        query.refine_partition_vi(md, s)
    gpu_ctx.synchronize()                                                                # nothing was launched or reported
    assert call(pa=ptr(md)) == 0
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == -6 and "msc_partition_refine_vi" in str(e.value) and "detail of the first: 2]" in str(e.value)
    gpu_ctx.synchronize()                                                                # (read and cleared)
    # and a start with more clusters than max_clusters, found the same way: it is not refined
    assert call(ps=ptr(dev(gpu_ctx, np.stack([starts[0], (np.arange(m) % 41).astype(np.int32), starts[2]])))) == 0
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == -6 and "detail of the first: 1]" in str(e.value)
    got = lab.cpu().numpy()
    want = query._refine_vi_host(A, starts, 3, 40, None)
    assert np.array_equal(got[[0, 2]], want[0][[0, 2]])
    against_host(gpu_ctx, A, starts, max_clusters=40)                                    # the context is good


def test_query_functions_on_device_tensors(gpu_ctx):
    rng = np.random.default_rng(21)
    S, m = 24, 150
    A = planted(rng, S, m, 5, 0.25)
    gate = EPS * (m + 16) * 4.0 * np.log2(m)
    want = query.refine_partition_vi(list(A))
    # the default starts are picked by the float64 expected VI: the host's are further apart than the gate at the cut
    ranked = np.sort(query.expected_loss(list(A)).vi)
    assert ranked[8] - ranked[7] > 4 * gate
    for got in (query.refine_partition_vi(dev(gpu_ctx, A)), query.refine_partition_vi(A, ctx=gpu_ctx),
                query.refine_partition_vi([dev(gpu_ctx, a) for a in A],
                                          starts=A[np.argsort(query.expected_loss(list(A)).vi, kind="stable")[:8]])):
        assert isinstance(got, query.RefinedVI) and isinstance(got.labels, torch.Tensor) and got.valid == S
        assert got.labels.dtype == torch.int32 and got.decrease.dtype == torch.int64 and got.vi.dtype == torch.float64
        for name in NAMES:
            assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), name
        assert np.abs(got.vi.cpu().numpy() - want.vi).max() <= gate
        assert np.abs(got.vi_start.cpu().numpy() - want.vi_start).max() <= gate
    assert (want.moves > 0).all() and (want.vi < want.vi_start).all()
    # vi_estimate(refine=3): the winner among the refined partitions is decided by the float64 VI too
    host = query.vi_estimate(list(A), refine=3)
    r = query.refine_partition_vi(list(A), max_sweeps=3)
    distinct = np.unique(r.vi)
    assert distinct.size == 1 or np.diff(distinct).min() > 4 * gate
    for got in (query.vi_estimate(dev(gpu_ctx, A), refine=3), query.vi_estimate(list(A), ctx=gpu_ctx, refine=3)):
        assert got.index == host.index and np.array_equal(got.labels, host.labels)
        assert np.abs(got.losses - host.losses).max() <= gate
        assert np.array_equal(got.confidence, host.confidence)
    assert query.expected_loss(list(A), host.labels).vi[0] < host.losses.min()
    plain = query.vi_estimate(dev(gpu_ctx, A), refine=0)
    assert plain.index == query.vi_estimate(list(A)).index
