"""The z-matrix accumulator on the device (msc_zmatrix_*, common_amd.ZMatrix, common_amd.query on device tensors): exact
counts against a numpy restatement for every batch boundary and both label widths, result bits, row subsets, strides,
batching and reset, reordering, the soft report of a bad label, the full size against a one-hot matmul on the device, and a
chain of sweep steps whose z is overwritten in place."""
import numpy as np
import pytest
import torch

import common_amd
from common_amd import query
from oracle import oracle as orc
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

BATCH8, BATCH16 = 1024, 512      # samples a batch holds at 8 and at 16 bits (include/microscopes_hip.h)


def host_counts(A, rows=None):
    """C[a, b] = samples of A ([S, n]) in which rows[a] and rows[b] carry the same label"""
    A = np.asarray(A)
    if rows is not None:
        A = A[:, np.asarray(rows)]
    m = A.shape[1]
    c = np.zeros((m, m), dtype=np.int64)
    for s0 in range(0, A.shape[0], 16):
        blk = A[s0:s0 + 16]
        c += (blk[:, :, None] == blk[:, None, :]).sum(0)
    return c


def labels(rng, S, n, nlabels):
    """samples with structure (a few big groups) and with the whole label range in use, top labels included"""
    out = np.empty((S, n), dtype=np.int32)
    for s in range(S):
        kind = s % 3
        if kind == 0:
            v = rng.integers(0, nlabels, n)
        elif kind == 1:
            few = rng.integers(0, nlabels, min(nlabels, 4))
            v = few[rng.integers(0, few.size, n)]
        else:
            v = np.maximum(nlabels - 1 - rng.integers(0, 8, n), 0)
        if n >= nlabels and s % 2 == 0:
            v[rng.permutation(n)[:nlabels]] = np.arange(nlabels)   # every label of the range in this sample
        out[s] = v
    return out


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def counts_np(zm, **kw):
    return zm.counts(**kw).cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("nlabels", [1, 2, 8, 256, 257, 1024, 65536])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 200, 1000])
def test_exact_counts_across_batches(gpu_ctx, m, nlabels):
    cap = BATCH8 if nlabels <= 256 else BATCH16
    rng = np.random.default_rng(m * 7 + nlabels)
    marks = [1, 3, 4, 5, cap + 1] + ([2 * cap + 3] if m <= 200 else [])
    A = labels(rng, marks[-1], m, nlabels)
    if nlabels == 256 and m >= 256:
        assert len(np.unique(A[0])) == 256
    if nlabels > 256 and m >= 1000:
        assert len(np.unique(A[0])) > 256
    zm = common_amd.ZMatrix(gpu_ctx, m, nlabels)
    prev = 0
    for S in marks:
        zm.add(dev(gpu_ctx, A[prev:S]))
        prev = S
        assert zm.nsamples == S
        got = counts_np(zm)
        assert np.array_equal(got, host_counts(A[:S])), (m, nlabels, S)
    zm.close()


@pytest.mark.parametrize("nlabels,S", [(3, 1), (256, 5), (1024, BATCH16 + 1), (64, BATCH8 + 7)])
def test_result_bits(gpu_ctx, nlabels, S):
    rng = np.random.default_rng(S)
    n = 150
    A = labels(rng, S, n, nlabels)
    zm = common_amd.ZMatrix(gpu_ctx, n, nlabels)
    zm.add(dev(gpu_ctx, A))
    c = host_counts(A)
    want = c.astype(np.float32) / np.float32(S)
    got = zm.result().cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), query.zmatrix(list(A)).view(np.uint32))
    zm.close()


def test_rows_subsets_strides_and_splits(gpu_ctx):
    rng = np.random.default_rng(21)
    n, S, K = 700, 1100, 40
    A = labels(rng, S, n, K)
    rows = rng.integers(0, n, 300)
    rows[:10] = rows[10:20]                        # repeats, unsorted
    want = host_counts(A, rows)
    # one [S, n] add with ld > n
    wide = np.zeros((S, n + 37), dtype=np.int32)
    wide[:, :n] = A
    wide[:, n:] = 99999                            # never read
    wt = dev(gpu_ctx, wide)[:, :n]
    assert wt.stride(0) == n + 37
    one = common_amd.ZMatrix(gpu_ctx, n, K, rows=rows)
    one.add(wt)
    assert np.array_equal(counts_np(one), want)
    # S single adds
    single = common_amd.ZMatrix(gpu_ctx, n, K, rows=rows)
    At = dev(gpu_ctx, A)
    for s in range(S):
        single.add(At[s])
    assert single.nsamples == S and np.array_equal(counts_np(single), want)
    # uneven splits, across the batch boundary
    split = common_amd.ZMatrix(gpu_ctx, n, K, rows=rows)
    cuts = [0, 1, 4, 517, 1023, 1024, 1030, S]
    for a, b in zip(cuts[:-1], cuts[1:]):
        split.add(At[a:b])
    assert np.array_equal(counts_np(split), want)
    # reset: as new
    split.reset()
    assert split.nsamples == 0
    assert np.array_equal(counts_np(split), np.zeros_like(want))
    with pytest.raises(common_amd.MicroscopesHipError):
        split.result()                             # no sample: the reference raises on an empty list
    split.add(At[:3])
    assert np.array_equal(counts_np(split), host_counts(A[:3], rows))
    for zm in (one, single, split):
        zm.close()


def test_reorder_ld_out_symmetry_and_diagonal(gpu_ctx):
    rng = np.random.default_rng(8)
    n, S, K = 333, 77, 300
    A = labels(rng, S, n, K)
    zm = common_amd.ZMatrix(gpu_ctx, n, K)
    zm.add(dev(gpu_ctx, A))
    c = host_counts(A)
    order = rng.permutation(n)
    got = counts_np(zm, order=order)
    assert np.array_equal(got, c[order][:, order])
    plain = counts_np(zm)
    assert np.array_equal(plain, plain.T) and np.all(np.diag(plain) == S)
    out = torch.full((n, n + 13), -7.0, dtype=torch.float32, device=gpu_ctx.torch_device)
    r = zm.result(order=order, out=out)
    want = (c.astype(np.float32) / np.float32(S))[order][:, order]
    assert np.array_equal(r.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.all(out[:, n:] == -7.0)            # nothing past ld_out's m columns is written
    zd = zm.result()
    assert np.array_equal(query.zmatrix_reorder(zd, order).cpu().numpy(), r.cpu().numpy())
    for bad in ([0] * n, np.arange(n - 1), np.arange(1, n + 1)):
        with pytest.raises(ValueError):
            zm.counts(order=bad)
    zm.close()


def test_bad_label_is_reported_and_skipped(gpu_ctx):
    rng = np.random.default_rng(4)
    n, K = 90, 16
    A = labels(rng, 9, n, K)
    bad = A.copy()
    bad[4, 17] = K                                  # one label past the range in sample 4
    bad[6, 3] = -1                                  # and a negative one in sample 6
    gpu_ctx.synchronize()
    zm = common_amd.ZMatrix(gpu_ctx, n, K)
    zm.add(dev(gpu_ctx, bad))
    with pytest.raises(common_amd.MicroscopesHipError) as ei:
        gpu_ctx.synchronize()
    assert ei.value.code == -6                      # MSC_EDEVICE
    good = np.delete(A, [4, 6], axis=0)
    assert np.array_equal(counts_np(zm), host_counts(good))
    gpu_ctx.synchronize()                           # reported once
    zm.close()


def test_full_size_against_one_hot_matmul(gpu_ctx):
    m, S, K = 16384, 256, 64
    g = torch.Generator(device=gpu_ctx.torch_device)
    g.manual_seed(5)
    z = torch.randint(0, K, (S, m), dtype=torch.int32, device=gpu_ctx.torch_device, generator=g)
    z[::2] = z[::2] // 16                          # half of the samples with 4 big groups
    zm = common_amd.ZMatrix(gpu_ctx, m, K)
    zm.add(z)
    got = zm.counts()
    want = torch.zeros((m, m), dtype=torch.float32, device=gpu_ctx.torch_device)
    for s in range(S):
        h = torch.nn.functional.one_hot(z[s].long(), K).to(torch.float32)
        want.addmm_(h, h.T)                        # exact: every partial sum is an integer below 2^24
    assert torch.equal(got.to(torch.float32), want)
    res = zm.result()
    assert torch.equal(res, want / float(S))
    zm.close()


def test_sweep_chain_with_z_overwritten_in_place(gpu_ctx):
    rng = np.random.default_rng(12)
    N, K = 1500, 12
    feats = [make_feature(orc.NICH, N, K, rng), make_feature(orc.BB, N, K, rng)]
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    for i, f in enumerate(feats):
        st.set_hp(i, orc.Family(f["family"], f["hp"], f["dim"], "f64").hp)
    st.set_alpha(1.0)
    z = torch.from_numpy(rng.integers(0, K, N).astype(np.int32)).to(gpu_ctx.torch_device)
    st.accumulate(view, z)
    zm = common_amd.ZMatrix(gpu_ctx, N, K)
    hist = []
    for sweep in range(12):                        # eager steps, a capture, then graph replays rewriting z in place
        st.sweep_step(view, z, seed=3, sweep=sweep)
        zm.add(z)
        hist.append(z.clone())
    got = zm.result().cpu().numpy()
    want = query.zmatrix([h.cpu().numpy() for h in hist])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len({tuple(h.cpu().numpy()[:50]) for h in hist}) > 1   # the chain moved
    zm.close()


def test_query_zmatrix_on_device_tensors(gpu_ctx):
    rng = np.random.default_rng(2)
    A = labels(rng, 30, 257, 40)
    host = query.zmatrix(list(A))
    for arg in (dev(gpu_ctx, A), [dev(gpu_ctx, a) for a in A]):
        got = query.zmatrix(arg, ctx=gpu_ctx)
        assert isinstance(got, torch.Tensor) and got.device == gpu_ctx.torch_device
        assert np.array_equal(got.cpu().numpy().view(np.uint32), host.view(np.uint32))
    got = query.zmatrix(list(A), ctx=gpu_ctx)            # numpy with ctx: the device route
    assert np.array_equal(got.cpu().numpy().view(np.uint32), host.view(np.uint32))
    B = A.astype(np.int64) * 1000 - 5                    # labels outside [0, 65536): renumbered first
    assert np.array_equal(query.zmatrix(dev(gpu_ctx, B), ctx=gpu_ctx).cpu().numpy().view(np.uint32),
                          query.zmatrix(list(B)).view(np.uint32))
    with pytest.raises(ValueError):
        query.zmatrix([], ctx=gpu_ctx)


def test_argument_checks_and_close(gpu_ctx):
    with pytest.raises(ValueError):
        common_amd.ZMatrix(gpu_ctx, 10, 4, rows=[0, 10])
    with pytest.raises(common_amd.MicroscopesHipError):
        common_amd.ZMatrix(gpu_ctx, 10, 65537)
    with pytest.raises(common_amd.MicroscopesHipError):
        common_amd.ZMatrix(gpu_ctx, 10, 0)
    zm = common_amd.ZMatrix(gpu_ctx, 10, 4)
    with pytest.raises(ValueError):
        zm.add(torch.zeros(11, dtype=torch.int32, device=gpu_ctx.torch_device))
    with pytest.raises(ValueError):
        zm.add(torch.zeros(10, dtype=torch.int64, device=gpu_ctx.torch_device))
    zm.close()
    zm.close()
    with pytest.raises(ValueError):
        zm.add(torch.zeros(10, dtype=torch.int32, device=gpu_ctx.torch_device))
    # an accumulator that outlives its context closes without touching the library
    ctx2 = common_amd.Context(device=0)
    zm2 = common_amd.ZMatrix(ctx2, 10, 4)
    zm2.add(torch.zeros(10, dtype=torch.int32, device=ctx2.torch_device))
    ctx2.close()
    zm2.close()
