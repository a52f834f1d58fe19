"""GPU: greedy refinement of partitions against the z-matrix accumulator (msc_zmatrix_partition_refine,
ZMatrix.partition_refine, common_amd.query.refine_partition / point_estimate(refine=) on device tensors).  Every comparison
is against the host path (plain numpy over the int64 counts) and exact: labels, binder_num, sweeps and moves.  Sizes on both
sides of a band, a tile and one pass of the workgroup, all 203 partitions of six rows in one launch; binder_num against
the loss kernel on the device's own labels; one case with a row subset with repeats, 16-bit sample labels, the extreme
int32 labels, ld > n, staged samples, a visiting order, an id capacity that binds, one sweep and no sweep; the same bits
from run to run and under any split of the starts; sums beyond 2^32; the accumulator left as it was; the error paths;
point_estimate with refine on device tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import common_amd
from common_amd import _lib as L
from common_amd import query

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
BATCH16 = 512                    # samples a batch holds at 16 bits (include/microscopes_hip.h)
SMALL, LARGE = "k_zm_refine_sweep<4096, 1, true>", "k_zm_refine_sweep<32768, 4, false>"
SHAPES = {1: (12, 2, 0.3), 2: (12, 2, 0.3), 6: (12, 2, 0.3), 63: (24, 4, 0.25), 64: (24, 4, 0.25), 65: (24, 4, 0.25),
          130: (40, 5, 0.2), 257: (40, 6, 0.3), 300: (40, 6, 0.3)}           # m -> S, Kt, noise


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def planted(rng, m, S, Kt, noise):
    """S samples of one truth of Kt clusters, every row relabelled uniformly in [0, Kt + 2) with probability noise"""
    truth = rng.integers(0, Kt, m)
    A = np.tile(truth, (S, 1))
    flip = rng.random((S, m)) < noise
    A[flip] = rng.integers(0, Kt + 2, int(flip.sum()))
    return A.astype(np.int32)


def some_starts(rng, A):
    """all-in-one, all-singletons, a random 7-labelling, three of the samples"""
    m = A.shape[1]
    return np.stack([np.zeros(m, dtype=np.int32), np.arange(m, dtype=np.int32), rng.integers(0, 7, m).astype(np.int32),
                     A[0], A[1], A[2]])


def set_partitions(n):
    out = []

    def grow(prefix, top):
        if len(prefix) == n:
            out.append(list(prefix))
            return
        for v in range(top + 2):
            grow(prefix + [v], max(top, v))
    grow([0], 0)
    return np.array(out, dtype=np.int32)


def equal(got, want):
    """device outputs (labels, binder_num, sweeps, moves) against the host's, bit for bit"""
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[3].dtype == torch.int64
    for g, w, name in zip(got, want, ("labels", "binder_num", "sweeps", "moves")):
        assert np.array_equal(g.cpu().numpy(), w), name
    return True


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130, 257, 300])
def test_sizes_against_the_host_path(gpu_ctx, m):
    S, Kt, noise = SHAPES[m]
    rng = np.random.default_rng(100 + m)
    A = planted(rng, m, S, Kt, noise)
    starts = some_starts(rng, A)
    want = query.refine_partition(list(A), starts)
    if m >= 63:                                                          # agreement is agreement on something
        assert want.moves[:3].min() > 0 and want.moves.max() > 0 and want.sweeps.max() >= 2
    zm = common_amd.ZMatrix(gpu_ctx, m, Kt + 2)
    zm.add(dev(gpu_ctx, A))
    got = zm.partition_refine(dev(gpu_ctx, starts))
    assert gpu_ctx.last_kernel("zmatrix") == SMALL
    assert equal(got, want[:4])
    assert tuple(got[0].shape) == (len(starts), m)
    # the running total against the loss kernel, on the device's own labels
    assert torch.equal(zm.partition_loss(got[0])[0], got[1])
    whole = query.refine_partition(dev(gpu_ctx, A), starts)              # the query entry, on device tensors
    assert isinstance(whole.labels, torch.Tensor) and whole.valid == want.valid == S
    assert equal(whole[:4], want[:4])
    zm.close()


def test_all_partitions_of_six_rows_in_one_launch(gpu_ctx):
    S, Kt, noise = SHAPES[6]
    rng = np.random.default_rng(106)
    A = planted(rng, 6, S, Kt, noise)
    parts = set_partitions(6)
    assert parts.shape == (203, 6)
    want = query.refine_partition(list(A), parts)
    assert want.moves.max() > 0 and want.sweeps.max() >= 2
    zm = common_amd.ZMatrix(gpu_ctx, 6, Kt + 2)
    zm.add(dev(gpu_ctx, A))
    got = zm.partition_refine(dev(gpu_ctx, parts))
    assert equal(got, want[:4])
    assert torch.equal(zm.partition_loss(got[0])[0], got[1])
    zm.close()


def test_subset_wide_labels_order_capacity_and_sweep_limits(gpu_ctx):
    rng = np.random.default_rng(3)
    n, m, S, ld = 150, 100, BATCH16 + 7, 155
    A = planted(rng, n, S, 5, 0.3)
    loners = rng.permutation(n)[:6]
    A[:, loners] = 290 + np.arange(6)                                    # rows nobody is ever with; labels need 16 bits
    rows = rng.permutation(n)[:m]
    rows[10:20] = rows[:10]                                              # repeats
    rows[20:26] = loners
    zm = common_amd.ZMatrix(gpu_ctx, n, 300, rows=rows)
    zm.add(dev(gpu_ctx, A[:200]))
    zm.add(dev(gpu_ctx, A[200:]))                                        # one full batch counted, seven samples staged
    assert zm.nsamples == S
    starts = np.stack([np.zeros(n, dtype=np.int32),
                       np.array([I32.min, -1, 0, 1, 2, 3, I32.max], dtype=np.int32)[rng.integers(0, 7, n)]])
    order = rng.permutation(m)
    wide = torch.full((2, ld), 12345, dtype=torch.int32, device=gpu_ctx.torch_device)
    wide[:, :n] = dev(gpu_ctx, starts)
    As, st = list(A[:, rows]), starts[:, rows]
    want = query.refine_partition(As, st, max_clusters=7, order=order)
    loose = query.refine_partition(As, st, order=order)
    # the capacity binds: with room the loners end alone, without it they cannot leave
    assert all(len(set(l)) == 7 for l in want.labels.tolist()) and all(len(set(l)) > 7 for l in loose.labels.tolist())
    assert not np.array_equal(want.labels, loose.labels) and want.sweeps.min() >= 3
    got = zm.partition_refine(wide[:, :n], max_clusters=7, order=order)  # the call itself flushes the seven
    assert equal(got, want[:4])
    assert torch.equal(zm.partition_loss(_scatter(gpu_ctx, got[0], rows, n))[0], got[1])
    assert equal(zm.partition_refine(wide[:, :n], order=order), loose[:4])
    # the state after exactly one sweep of a start that needs three or more, and after none
    one = query.refine_partition(As, st, max_sweeps=1, max_clusters=7, order=order)
    assert one.sweeps.tolist() == [1, 1] and one.moves.min() > 0 and (one.binder_num > want.binder_num).all()
    assert equal(zm.partition_refine(wide[:, :n], max_sweeps=1, max_clusters=7, order=order), one[:4])
    none = query.refine_partition(As, st, max_sweeps=0, max_clusters=7, order=order)
    assert none.sweeps.tolist() == [0, 0] and none.moves.tolist() == [0, 0]
    assert np.array_equal(none.binder_num, query.partition_loss(As, st)[0])
    assert equal(zm.partition_refine(wide[:, :n], max_sweeps=0, max_clusters=7, order=order), none[:4])
    zm.close()


def _scatter(ctx, labels, rows, n):
    """labels over the positions as vectors of n labels (the repeated rows of this file's case end together)"""
    lab = labels.cpu().numpy()
    full = np.full((lab.shape[0], n), -1, dtype=np.int32)
    full[:, rows] = lab
    assert np.array_equal(full[:, rows], lab)
    return dev(ctx, full)


def test_same_bits_from_run_to_run_and_under_any_split(gpu_ctx):
    rng = np.random.default_rng(4)
    m, (S, Kt, noise) = 130, SHAPES[130]
    A = planted(rng, m, S, Kt, noise)
    starts = np.concatenate([some_starts(rng, A), rng.integers(0, 9, (64, m)).astype(np.int32)])
    zm = common_amd.ZMatrix(gpu_ctx, m, Kt + 2)
    zm.add(dev(gpu_ctx, A))
    sd = dev(gpu_ctx, starts)
    first = zm.partition_refine(sd)
    assert int(first[3].max()) > 0
    again = zm.partition_refine(sd)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for cut in (1, 3, 64):
        lo, hi = zm.partition_refine(sd[:cut]), zm.partition_refine(sd[cut:])
        assert all(torch.equal(torch.cat([a, b]), c) for a, b, c in zip(lo, hi, first))
    zm.close()


def test_past_one_step_of_columns(gpu_ctx):
    """m = 4100: the sweep kernel that keeps 32768 ids and four loads a thread, with 32-bit bins (S m < 2^32)"""
    rng = np.random.default_rng(41)
    m, S, Kt = 4100, 24, 6
    A = planted(rng, m, S, Kt, 0.15)
    starts = np.stack([rng.integers(0, 7, m).astype(np.int32), A[0]])
    want = query.refine_partition(list(A), starts, max_clusters=1024)
    assert want.moves.min() > 0 and want.sweeps.max() >= 2
    zm = common_amd.ZMatrix(gpu_ctx, m, Kt + 2)
    zm.add(dev(gpu_ctx, A))
    got = zm.partition_refine(dev(gpu_ctx, starts))                      # None: min(m, 1024)
    assert gpu_ctx.last_kernel("zmatrix") == "k_zm_refine_sweep<32768, 4, true>"
    assert equal(got, want[:4])
    assert torch.equal(zm.partition_loss(got[0])[0], got[1])
    zm.close()


@pytest.mark.parametrize("m", [4096, 5000])
def test_sums_beyond_32_bits(gpu_ctx, m):
    rng = np.random.default_rng(21)
    n, S = 3, (1 << 20) + 8
    A = np.repeat(rng.integers(0, 2, (S, 1)), n, axis=1).astype(np.int32)
    A[:, 1] ^= rng.random(S) < 0.1                                       # three rows that mostly agree
    A[:, 2] ^= rng.random(S) < 0.2
    rows = rng.integers(0, n, m)
    zm = common_amd.ZMatrix(gpu_ctx, n, 2, rows=rows)
    zm.add(dev(gpu_ctx, A))
    C3 = np.array([[int((A[:, i] == A[:, j]).sum()) for j in range(n)] for i in range(n)], dtype=np.int64)
    Cm = C3[rows][:, rows]
    assert S * m >= 1 << 32                                              # the 64-bit bins
    if m == 5000:
        assert (Cm.sum(axis=1) - S).max() > 1 << 32                      # s_0 of all-in-one at the first position and on
    # two starts over the three rows: a two-labelling that parts rows 0 and 1, and all-in-one
    by_row = np.array([[0, 1, 0], [0, 0, 0]], dtype=np.int32)
    want3 = query._refine_host(Cm, by_row[:, rows], 20, 1024, None)
    assert want3[3].max() > 0 and want3[2].max() >= 2
    got = zm.partition_refine(dev(gpu_ctx, by_row), max_clusters=1024)
    assert gpu_ctx.last_kernel("zmatrix") == (LARGE if m > 4096 else "k_zm_refine_sweep<4096, 1, false>")
    assert equal(got, want3)
    zm.close()


def test_the_accumulator_is_left_as_it_was(gpu_ctx):
    rng = np.random.default_rng(5)
    A = planted(rng, 77, 9, 3, 0.3)
    zm = common_amd.ZMatrix(gpu_ctx, 77, 5)
    zm.add(dev(gpu_ctx, A))
    before = zm.counts().clone()
    sd = dev(gpu_ctx, some_starts(rng, A))
    moved = zm.partition_refine(sd)[3]
    assert int(moved.max()) > 0
    assert zm.nsamples == 9 and torch.equal(zm.counts(), before)
    zm.add(dev(gpu_ctx, A[:2]))                                          # and it goes on accumulating
    assert zm.partition_loss(sd)[2] == 11
    zm.close()


def test_error_paths(gpu_ctx):
    n = 20
    lib = gpu_ctx.lib
    zm = common_amd.ZMatrix(gpu_ctx, n, 4)
    sd = torch.zeros((2, n), dtype=torch.int32, device=gpu_ctx.torch_device)
    sd[1] = torch.arange(n, dtype=torch.int32)
    lab = torch.zeros((2, n), dtype=torch.int32, device=gpu_ctx.torch_device)
    ptr = lambda t: C.c_void_p(t.data_ptr())                             # noqa: E731

    def call(h, s, ns, ld, kc, order=None):
        o = None if order is None else np.asarray(order, dtype=np.uint32).ctypes.data_as(C.c_void_p)
        return lib.msc_zmatrix_partition_refine(h, s, ns, ld, 3, kc, o, ptr(lab), None, None, None)
    with pytest.raises(common_amd.MicroscopesHipError) as ei:            # no sample yet
        zm.partition_refine(sd)
    assert ei.value.code == -1                                           # MSC_EINVAL
    zm.add(sd[:1])
    assert call(zm._h, ptr(sd), 0, n, n) == -1                           # nstarts == 0
    assert call(zm._h, ptr(sd), 2, n - 1, n) == -1                       # ld < n
    assert call(zm._h, None, 2, n, n) == -1                              # no starts
    assert call(None, ptr(sd), 2, n, n) == -1                            # no handle
    assert call(zm._h, ptr(sd), 2, n, 0) == -1                           # max_clusters 0
    assert call(zm._h, ptr(sd), 2, n, n + 1) == -1                       # ... above m
    assert call(zm._h, ptr(sd), 2, n, n, order=[0] * n) == -1            # not a permutation
    assert call(zm._h, ptr(sd), 2, n, n, order=list(range(1, n + 1))) == -1
    assert lib.msc_zmatrix_partition_refine(zm._h, ptr(sd), 2, n, 3, n, None, None, None, None, None) == 0   # nothing asked for
    assert call(zm._h, ptr(sd), 2, n, n) == 0
    gpu_ctx.synchronize()
    assert lab[0].tolist() == [0] * n                                    # (all rows together in the one sample)
    # a start with too many clusters: the wrapper says so before the launch; the library finds it on the device
    with pytest.raises(ValueError, match="max_clusters"):
        zm.partition_refine(sd, max_clusters=5)
    for bad in (dict(max_clusters=0), dict(max_clusters=n + 1), dict(max_sweeps=-1), dict(order=[0] * n)):
        with pytest.raises(ValueError):
            zm.partition_refine(sd, **bad)
    assert call(zm._h, ptr(sd), 2, n, 5) == 0
    with pytest.raises(common_amd.MicroscopesHipError) as ei:
        gpu_ctx.synchronize()
    assert ei.value.code == -6 and "max_clusters" in str(ei.value)       # MSC_EDEVICE
    gpu_ctx.synchronize()                                                # (read and cleared)
    assert equal(zm.partition_refine(sd[:1]), query.refine_partition([[0] * n], [[0] * n])[:4])
    zm.close()
    with pytest.raises(ValueError, match="closed"):
        zm.partition_refine(sd)
    # beyond the caps: max_clusters above 1024 on an accumulator that has the rows for it
    m = L.ZMATRIX_REFINE_MAX_CLUSTERS + 76
    big = common_amd.ZMatrix(gpu_ctx, 1, 1, rows=np.zeros(m, dtype=np.int64))
    one = torch.zeros((1, 1), dtype=torch.int32, device=gpu_ctx.torch_device)
    big.add(one)
    out = torch.zeros((1, m), dtype=torch.int32, device=gpu_ctx.torch_device)
    rc = lib.msc_zmatrix_partition_refine(big._h, ptr(one), 1, 1, 3, L.ZMATRIX_REFINE_MAX_CLUSTERS + 1, None, ptr(out),
                                          None, None, None)
    assert rc == -4                                                      # MSC_EUNSUPPORTED
    with pytest.raises(common_amd.MicroscopesHipError) as ei:
        big.partition_refine(one, max_clusters=m)
    assert ei.value.code == -4
    fits = big.partition_refine(one)                                     # None: capped to what the device takes
    assert int(fits[3][0]) == 0 and int(fits[2][0]) == 1 and int(fits[1][0]) == 0
    big.close()


def test_point_estimate_with_refine_on_device_tensors(gpu_ctx):
    rng = np.random.default_rng(9)
    A = planted(rng, 90, 30, 4, 0.3)
    want = query.point_estimate(list(A), refine=5)
    plain = query.point_estimate(list(A))
    assert int(query.partition_loss(list(A), want.labels)[0][0]) < plain.losses.min()
    for arg in (dev(gpu_ctx, A), [dev(gpu_ctx, a) for a in A]):
        got = query.point_estimate(arg, ctx=gpu_ctx, refine=5)
        assert np.array_equal(got.labels, want.labels) and got.index == want.index
        assert np.array_equal(got.confidence, want.confidence) and np.array_equal(got.losses, want.losses)
    got0 = query.point_estimate(dev(gpu_ctx, A), refine=0)
    assert np.array_equal(got0.labels, plain.labels) and got0.index == plain.index
    with pytest.raises(ValueError, match="variation-of-information"):
        query.point_estimate(dev(gpu_ctx, A), loss="vi", refine=2)
