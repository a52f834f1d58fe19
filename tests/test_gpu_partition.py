"""GPU: candidate partitions against the z-matrix accumulator (msc_zmatrix_partition_sums / _loss, ZMatrix.partition_sums /
partition_loss, common_amd.query.partition_loss / point_estimate on device tensors) -- w and size EXACTLY against the
numpy path over every tile shape (a lone row, the last band's padding, a diagonal-only grid, diagonal and off-diagonal
tiles), candidate counts on both sides of the kernel's batch and both label packings; a permuted row subset with repeats,
ld > n and the extreme int32 labels, with the staged samples flushed by the call; binder_num equal and vi_lb within
1e-10 of the host path, the same bits from run to run and under any split of the candidates; sums beyond 2^32 in both
forms of the sums kernel; the accumulator left as it was; the error paths; and point_estimate on device tensors, once on
a ChainEnsemble trace."""
import ctypes as C

import numpy as np
import pytest
import torch

import common_amd
from common_amd import query
from oracle import oracle as orc
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

BATCH8 = 1024                    # samples a batch holds at 8 bits (include/microscopes_hip.h)
CAND_BATCH = 64                  # candidates a workgroup of k_zm_partition_sums<true, 64> takes
I32 = np.iinfo(np.int32)
PACKED, WIDE = "k_zm_partition_sums<true, 64>", "k_zm_partition_sums<false, 32>"


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def samples(rng, S, n, nlabels):
    """a few big groups in half of the samples, the whole range in the others"""
    A = rng.integers(0, nlabels, (S, n)).astype(np.int32)
    A[::2] = A[::2] % min(nlabels, 4)
    return A


def candidates(rng, A, ncand):
    """the samples' own partitions, coarse and fine random ones, negative labels, labels no sample holds"""
    n = A.shape[1]
    out = np.empty((ncand, n), dtype=np.int32)
    for c in range(ncand):
        kind = c % 4
        if kind == 0:
            out[c] = A[(c // 4) % A.shape[0]]
        elif kind == 1:
            out[c] = rng.integers(-2, 2, n)
        elif kind == 2:
            out[c] = rng.integers(1000, 1000 + max(2, n // 3), n)
        elif c < 8:
            out[c] = 0 if c == 3 else np.arange(n)              # all in one, all singletons
        else:
            out[c] = rng.integers(0, c, n)
    return out


def accumulator(ctx, A, nlabels, rows=None):
    zm = common_amd.ZMatrix(ctx, A.shape[1], nlabels, rows=rows)
    zm.add(dev(ctx, A))
    return zm


@pytest.mark.parametrize("nlabels", [3, 300])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130, 200])
def test_exact_sums_against_the_numpy_path(gpu_ctx, m, nlabels):
    rng = np.random.default_rng(1000 * m + nlabels)
    A = samples(rng, 11, m, nlabels)
    zm = accumulator(gpu_ctx, A, nlabels)
    for ncand in (1, 5, CAND_BATCH + 1):
        cands = candidates(rng, A, ncand)
        w, size = zm.partition_sums(dev(gpu_ctx, cands))
        assert gpu_ctx.last_kernel("zmatrix") == PACKED
        assert w.dtype == torch.int64 and size.dtype == torch.int32 and tuple(w.shape) == tuple(size.shape) == (ncand, m)
        hw, hs = query.partition_sums(list(A), cands)
        assert np.array_equal(size.cpu().numpy(), hs), (m, ncand)
        assert np.array_equal(w.cpu().numpy(), hw), (m, ncand)
    one = zm.partition_sums(dev(gpu_ctx, cands[2]))                      # a plain vector is one candidate
    assert np.array_equal(one[0].cpu().numpy(), hw[2:3]) and np.array_equal(one[1].cpu().numpy(), hs[2:3])
    zm.close()


def test_row_subset_with_repeats_wide_rows_extreme_labels_and_the_flush(gpu_ctx):
    rng = np.random.default_rng(7)
    n, m, K, S = 150, 100, 40, BATCH8 + 7
    rows = rng.permutation(n)[:m]
    rows[10:20] = rows[:10]                                              # repeats
    A = samples(rng, S, n, K)
    zm = common_amd.ZMatrix(gpu_ctx, n, K, rows=rows)
    zm.add(dev(gpu_ctx, A[:500]))
    zm.add(dev(gpu_ctx, A[500:]))                                        # one full batch counted, seven samples staged
    assert zm.nsamples == S
    ncand, ld = 9, n + 5
    cands = candidates(rng, A, ncand)
    cands[1] = np.array([I32.min, -1, I32.max], dtype=np.int32)[rng.integers(0, 3, n)]
    cands[5] = np.where(rng.random(n) < 0.5, I32.min, I32.max)
    wide = torch.full((ncand, ld), 12345, dtype=torch.int32, device=gpu_ctx.torch_device)
    wide[:, :n] = dev(gpu_ctx, cands)
    w, size = zm.partition_sums(wide[:, :n])                             # the call itself flushes the seven
    hw, hs = query.partition_sums(list(A[:, rows]), cands[:, rows])
    assert np.array_equal(size.cpu().numpy(), hs) and np.array_equal(w.cpu().numpy(), hw)
    assert (hw >= S).all() and hw[:, 0].max() > S
    binder, vi, valid = zm.partition_loss(wide[:, :n])
    hb, hv, hvalid = query.partition_loss(list(A[:, rows]), cands[:, rows])
    assert valid == hvalid == S
    assert np.array_equal(binder.cpu().numpy(), hb)
    assert np.abs(vi.cpu().numpy() - hv).max() <= 1e-10
    zm.close()


@pytest.mark.parametrize("seed", [3, 4])
def test_partition_loss(gpu_ctx, seed):
    rng = np.random.default_rng(seed)
    m, K, S, ncand = 130, 12, 40, CAND_BATCH + 6
    A = samples(rng, S, m, K)
    cands = candidates(rng, A, ncand)
    zm = accumulator(gpu_ctx, A, K)
    cd = dev(gpu_ctx, cands)
    binder, vi, valid = zm.partition_loss(cd)
    assert binder.dtype == torch.int64 and vi.dtype == torch.float64 and tuple(binder.shape) == tuple(vi.shape) == (ncand,)
    hb, hv, hvalid = query.partition_loss(list(A), cands)
    assert valid == hvalid == S
    b, v = binder.cpu().numpy(), vi.cpu().numpy()
    print("binder_num equal: %s; max |vi_lb - host| = %.3g" % (np.array_equal(b, hb), np.abs(v - hv).max()))
    assert np.array_equal(b, hb) and (b >= 0).all()
    assert np.abs(v - hv).max() <= 1e-10
    best = np.sort(hv)[:2]
    assert best[1] - best[0] > 1e-9                                      # (the seeds are chosen for this)
    assert int(np.argmin(v)) == int(np.argmin(hv))
    assert int(np.argmin(b)) == int(np.argmin(hb))
    # the same bits from run to run, and under any split of the candidates over calls
    again = zm.partition_loss(cd)
    assert torch.equal(again[0], binder) and torch.equal(again[1].view(torch.int64), vi.view(torch.int64))
    for cut in (1, 3, CAND_BATCH):
        lo, hi = zm.partition_loss(cd[:cut]), zm.partition_loss(cd[cut:])
        assert torch.equal(torch.cat([lo[0], hi[0]]), binder)
        assert torch.equal(torch.cat([lo[1], hi[1]]).view(torch.int64), vi.view(torch.int64))
    zm.close()


def test_sums_beyond_32_bits(gpu_ctx):
    m, S = 8192, (1 << 19) + 8
    assert m * S > 1 << 32
    zm = common_amd.ZMatrix(gpu_ctx, 1, 1, rows=np.zeros(m, dtype=np.int64))
    zm.add(torch.zeros((S, 1), dtype=torch.int32, device=gpu_ctx.torch_device))
    cand = torch.full((1,), 5, dtype=torch.int32, device=gpu_ctx.torch_device)
    w, size = zm.partition_sums(cand)
    assert gpu_ctx.last_kernel("zmatrix") == PACKED
    assert bool((w == m * S).all()) and bool((size == m).all())
    binder, vi, valid = zm.partition_loss(cand)
    assert valid == S and int(binder[0]) == 0
    assert abs(float(vi[0]) + np.log2(m)) <= 1e-10                       # log2 m - 2 log2 (m S) + 2 log2 S
    zm.close()


def test_sums_of_a_million_samples_take_the_64_bit_form(gpu_ctx):
    rng = np.random.default_rng(21)
    n, m, S = 3, 5000, (1 << 20) + 8                                     # counts reach 2^20: no packed partial sums
    A = np.repeat(rng.integers(0, 2, (S, 1)), n, axis=1).astype(np.int32)
    A[:, 1] ^= rng.random(S) < 0.1                                       # three rows that mostly agree
    A[:, 2] ^= rng.random(S) < 0.2
    rows = rng.integers(0, n, m)
    zm = common_amd.ZMatrix(gpu_ctx, n, 2, rows=rows)
    zm.add(dev(gpu_ctx, A))
    C3 = np.array([[int((A[:, i] == A[:, j]).sum()) for j in range(n)] for i in range(n)], dtype=np.int64)
    mult = np.bincount(rows, minlength=n).astype(np.int64)               # positions that carry each of the three rows
    cands = np.array([[0, 0, 0], [0, 1, 2], [4, 4, -9], [I32.min, I32.max, I32.max]], dtype=np.int32)
    cands = np.concatenate([cands, rng.integers(0, 2, (CAND_BATCH // 2 + 1 - 4, n)).astype(np.int32)])
    w, size = zm.partition_sums(dev(gpu_ctx, cands))
    assert gpu_ctx.last_kernel("zmatrix") == WIDE
    same3 = cands[:, :, None] == cands[:, None, :]                       # by the definition, over the three rows
    hw = (same3 * (C3 * mult[None, :])[None]).sum(axis=2)[:, rows]
    hs = (same3 * mult[None, None, :]).sum(axis=2)[:, rows]
    assert hw.max() > 1 << 32
    assert np.array_equal(w.cpu().numpy(), hw) and np.array_equal(size.cpu().numpy(), hs)
    binder, vi, valid = zm.partition_loss(dev(gpu_ctx, cands))
    assert valid == S
    T = (int(mult @ C3 @ mult) - m * S) // 2
    hb = T + S * ((hs - 1).sum(axis=1) // 2) - (hw - S).sum(axis=1)
    assert np.array_equal(binder.cpu().numpy(), hb) and (hb >= 0).all()
    hv = (np.log2(hs.astype(np.float64)) - 2. * np.log2(hw.astype(np.float64))).sum(axis=1) / m + 2. * np.log2(float(S))
    assert np.abs(vi.cpu().numpy() - hv).max() <= 1e-10
    zm.close()


def test_the_accumulator_is_left_as_it_was(gpu_ctx):
    rng = np.random.default_rng(5)
    A = samples(rng, 9, 77, 5)
    zm = accumulator(gpu_ctx, A, 5)
    before = zm.counts().clone()
    cd = dev(gpu_ctx, candidates(rng, A, 6))
    zm.partition_sums(cd)
    zm.partition_loss(cd)
    assert zm.nsamples == 9 and torch.equal(zm.counts(), before)
    zm.add(dev(gpu_ctx, A[:2]))                                          # and it goes on accumulating
    assert zm.partition_loss(cd)[2] == 11
    zm.close()


def test_error_paths(gpu_ctx):
    n = 20
    lib = gpu_ctx.lib
    zm = common_amd.ZMatrix(gpu_ctx, n, 4)
    cd = torch.zeros((2, n), dtype=torch.int32, device=gpu_ctx.torch_device)
    out = torch.zeros(2 * n, dtype=torch.int64, device=gpu_ctx.torch_device)
    ptr = lambda t: C.c_void_p(t.data_ptr())                             # noqa: E731
    for call in (zm.partition_sums, zm.partition_loss):                  # no sample yet
        with pytest.raises(common_amd.MicroscopesHipError) as ei:
            call(cd)
        assert ei.value.code == -1                                       # MSC_EINVAL
    zm.add(cd)
    zm.partition_loss(cd)
    zm.reset()
    for call in (zm.partition_sums, zm.partition_loss):                  # nor after a reset
        with pytest.raises(common_amd.MicroscopesHipError) as ei:
            call(cd)
        assert ei.value.code == -1
    zm.add(cd)
    assert lib.msc_zmatrix_partition_sums(zm._h, ptr(cd), 0, n, ptr(out), None) == -1          # ncand == 0
    assert lib.msc_zmatrix_partition_sums(zm._h, ptr(cd), 2, n - 1, ptr(out), None) == -1      # ld < n
    assert lib.msc_zmatrix_partition_sums(zm._h, None, 2, n, ptr(out), None) == -1             # no candidates
    assert lib.msc_zmatrix_partition_sums(None, ptr(cd), 2, n, ptr(out), None) == -1           # no handle
    assert lib.msc_zmatrix_partition_loss(zm._h, ptr(cd), 0, n, ptr(out), None, None) == -1
    assert lib.msc_zmatrix_partition_loss(zm._h, ptr(cd), 2, n - 1, ptr(out), None, None) == -1
    assert lib.msc_zmatrix_partition_loss(zm._h, None, 2, n, ptr(out), None, None) == -1
    assert lib.msc_zmatrix_partition_loss(None, ptr(cd), 2, n, ptr(out), None, None) == -1
    assert lib.msc_zmatrix_partition_sums(zm._h, ptr(cd), 2, n, None, None) == 0               # nothing asked for
    assert lib.msc_zmatrix_partition_loss(zm._h, ptr(cd), 2, n, ptr(out), None, None) == 0     # binder_num alone
    gpu_ctx.synchronize()
    assert out[:2].tolist() == [0, 0]                                    # (all rows together in every sample)
    for bad in (torch.zeros((2, n + 1), dtype=torch.int32, device=gpu_ctx.torch_device),
                torch.zeros((2, n), dtype=torch.int64, device=gpu_ctx.torch_device),
                torch.zeros((2, n), dtype=torch.int32), torch.zeros((1, 2, n), dtype=torch.int32, device=gpu_ctx.torch_device),
                torch.zeros((2, 2 * n), dtype=torch.int32, device=gpu_ctx.torch_device)[:, ::2]):
        with pytest.raises(ValueError):
            zm.partition_sums(bad)
        with pytest.raises(ValueError):
            zm.partition_loss(bad)
    zm.close()
    with pytest.raises(ValueError, match="closed"):
        zm.partition_sums(cd)
    with pytest.raises(ValueError, match="closed"):
        zm.partition_loss(cd)


def same(est, want):
    return np.array_equal(est.labels, want.labels) and est.index == want.index and \
        np.array_equal(est.losses, want.losses) and est.losses.dtype == want.losses.dtype


def test_point_estimate_on_device_tensors(gpu_ctx):
    rng = np.random.default_rng(9)
    A = samples(rng, 30, 90, 7)
    want = query.point_estimate(list(A))
    for arg in (dev(gpu_ctx, A), [dev(gpu_ctx, a) for a in A]):
        got = query.point_estimate(arg, ctx=gpu_ctx)
        assert same(got, want) and np.array_equal(got.confidence, want.confidence)
    assert same(query.point_estimate(list(A), ctx=gpu_ctx), want)       # numpy with ctx: the device route
    cands = candidates(rng, A, 12)
    want = query.point_estimate(list(A), candidates=cands)
    assert same(query.point_estimate(dev(gpu_ctx, A), candidates=dev(gpu_ctx, cands)), want)
    assert same(query.point_estimate(dev(gpu_ctx, A), candidates=cands.astype(np.int64)), want)
    want_vi = query.point_estimate(list(A), "vi", candidates=cands)
    got_vi = query.point_estimate(dev(gpu_ctx, A), "vi", candidates=cands)
    best = np.sort(want_vi.losses)[:2]
    assert best[1] - best[0] > 1e-9
    assert got_vi.index == want_vi.index and np.array_equal(got_vi.labels, want_vi.labels)
    assert np.abs(got_vi.losses - want_vi.losses).max() <= 1e-10
    B = A.astype(np.int64) * 100000 - 7                                  # samples renumbered first; they are the candidates
    assert same(query.point_estimate(dev(gpu_ctx, B)), query.point_estimate(list(B)))
    hb, hv, hvalid = query.partition_loss(list(A), cands)
    b, v, valid = query.partition_loss(dev(gpu_ctx, A), dev(gpu_ctx, cands))
    assert isinstance(b, torch.Tensor) and valid == hvalid and np.array_equal(b.cpu().numpy(), hb)
    with pytest.raises(ValueError, match="loss"):
        query.point_estimate(dev(gpu_ctx, A), loss="rand")


def test_point_estimate_of_a_chain_ensemble_trace(gpu_ctx):
    N, K, nchains, nsweeps = 40, 10, 4, 5
    rng = np.random.default_rng(61)
    feats = [make_feature(f, N, 6, rng, 0) for f in (orc.NICH, orc.BB)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    ens = common_amd.ChainEnsemble(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K, nchains, alpha=1.0,
                                   hps=[f["hp"] for f in feats])
    ens.seat(view)
    rows = np.arange(N - 1, 4, -1)                                       # a subset, in another order
    zm = common_amd.ZMatrix(gpu_ctx, N, K, rows=rows)
    trace = ens.sweep(view, nsweeps, 5, zmatrix=zm)
    flat = trace.view(-1, N)
    assert zm.nsamples == flat.shape[0] == nchains * nsweeps
    got = query.point_estimate(zm, candidates=flat)
    host = flat.cpu().numpy()
    want = query.point_estimate(list(host[:, rows]))
    assert same(got, want) and np.array_equal(got.confidence, want.confidence)
    assert got.labels.shape == (rows.size,) and got.labels[0] == 0
    with pytest.raises(ValueError, match="candidates"):
        query.point_estimate(zm)
    zm.close()
    ens.close()
