"""Single linkage of a z-matrix on the device (msc_linkage_single, common_amd.query.zmatrix_linkage /
zmatrix_heuristic_block_ordering on float32 device tensors, ZMatrix.linkage / block_ordering): the float64 linkage
matrix and the leaf order against scipy on the downloaded matrix, EXACTLY, on both sides of every boundary the kernel has
(one wave / several, one column a thread / 2 / 4 / 8); row strides, an unaligned view and the input's bits; the
reference's view of an asymmetric or NaN-holding tensor; the accumulator's methods; the C entry's argument checks; and
the ordering of times against the host route at n = 4096."""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.cluster.hierarchy as hier
import torch

import common_amd
from common_amd import query

pytestmark = pytest.mark.gpu

# 64 | 65: one wave | two; 1024 | 1025: one column a thread | two; 2049: four; 4097: eight (4100: with 16-byte loads)
SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, 4100]


def walk(lk):
    """leaves_list restated (scipy's refuses a linkage with a negative distance)"""
    n = lk.shape[0] + 1
    out, stack = [], [2 * n - 2]
    while stack:
        v = stack.pop()
        if v < n:
            out.append(v)
        else:
            stack += [int(lk[v - n, 1]), int(lk[v - n, 0])]
    return np.array(out)


def reference(z):
    """the parent route on the downloaded matrix: the condensed upper triangle, 1 - z in float32, scipy"""
    z = np.asarray(z)
    n = z.shape[0]
    lk = hier.linkage(1. - np.array(z[np.triu_indices(n, k=1)]))
    return lk, (walk(lk) if (lk[:, 2] < 0).any() else np.array(hier.leaves_list(lk)))


def check(ctx, zd, kernel=None):
    want_lk, want_order = reference(zd.cpu().numpy())
    before = zd.clone()
    lk = query.zmatrix_linkage(zd, ctx=ctx)
    if kernel is not None:
        assert ctx.last_kernel("zmatrix") == kernel
    assert lk.dtype == np.float64 and lk.shape == want_lk.shape
    assert np.array_equal(lk, want_lk)
    lk2, order = ctx.linkage_single(zd)
    assert np.array_equal(lk2, want_lk) and np.array_equal(order, want_order)
    if (want_lk[:, 2] < 0).any():
        with pytest.raises(ValueError, match="negative distances"):
            query.zmatrix_heuristic_block_ordering(zd, ctx=ctx)
    else:
        got = query.zmatrix_heuristic_block_ordering(zd, ctx=ctx)
        assert isinstance(got, np.ndarray) and np.issubdtype(got.dtype, np.integer)
        assert np.array_equal(got, want_order)
    assert torch.equal(zd.view(torch.int32), before.view(torch.int32))         # the input's bits
    return lk, order


def accumulated(ctx, rng, n, S, K):
    zm = common_amd.ZMatrix(ctx, n, K)
    zm.add(torch.from_numpy(rng.integers(0, K, (S, n)).astype(np.int32)).to(ctx.torch_device))
    z = zm.result()
    zm.close()
    return z


def tie_free(rng, n):
    """symmetric, every off-diagonal pair a different multiple of 2^-24 below 1/2: 1 - z is exact and distinct"""
    iu = np.triu_indices(n, k=1)
    assert iu[0].size < 1 << 24
    z = np.eye(n, dtype=np.float32)
    z[iu] = rng.permutation(iu[0].size).astype(np.float32) / np.float32(1 << 24)
    z.T[iu] = z[iu]
    return z


@pytest.mark.parametrize("n", SIZES)
def test_linkage_and_order_against_scipy(gpu_ctx, n):
    rng = np.random.default_rng(n)
    dev = gpu_ctx.torch_device
    cols = 1 if n <= 1024 else 2 if n <= 2048 else 4 if n <= 4096 else 8
    kernel = "k_linkage_prim<%d, %s>" % (cols, "false" if cols == 1 or n % min(cols, 4) else "true")
    for S in (1, 3, 16):                                                     # heavy ties
        check(gpu_ctx, accumulated(gpu_ctx, rng, n, S, 5), kernel)
    check(gpu_ctx, torch.ones((n, n), dtype=torch.float32, device=dev), kernel)      # all equal: every distance 0
    check(gpu_ctx, torch.eye(n, dtype=torch.float32, device=dev), kernel)            # all singletons: every distance 1
    check(gpu_ctx, torch.from_numpy(tie_free(rng, n)).to(dev), kernel)
    above = accumulated(gpu_ctx, rng, n, 3, 4) * 4.0 - 0.5                   # entries up to 3.5: negative distances
    lk, _ = check(gpu_ctx, above, kernel)
    assert n == 2 or lk[0, 2] < 0


@pytest.mark.parametrize("n", [200, 1030, 2052, 2051])
def test_row_strides_and_an_unaligned_view(gpu_ctx, n):
    """ld > n, even and odd, and a view whose rows begin 4 bytes off: the one-float loads give the wide loads' bits"""
    rng = np.random.default_rng(n)
    dev = gpu_ctx.torch_device
    z = accumulated(gpu_ctx, rng, n, 3, 6)
    want = check(gpu_ctx, z)
    cols = 1 if n <= 1024 else 2 if n <= 2048 else 4
    vec = min(cols, 4)
    kernels = set()
    for pad in (4, 8, 13, 6, 7):
        wide = torch.full((n, n + pad), float("nan"), dtype=torch.float32, device=dev)     # (the padding is never used)
        wide[:, :n] = z
        view = wide[:, :n]
        assert view.stride(0) == n + pad and view.data_ptr() % 16 == 0
        got = check(gpu_ctx, view)
        kernels.add(gpu_ctx.last_kernel("zmatrix"))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if cols > 1:
            assert gpu_ctx.last_kernel("zmatrix") == "k_linkage_prim<%d, %s>" % (cols, "false" if (n + pad) % vec else "true")
    big = torch.full((n, n + 8), float("nan"), dtype=torch.float32, device=dev)
    big[:, 1:n + 1] = z
    view = big[:, 1:n + 1]
    assert view.data_ptr() % 16 == 4
    got = check(gpu_ctx, view, "k_linkage_prim<%d, false>" % cols)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if cols > 1:
        assert kernels == {"k_linkage_prim<%d, false>" % cols, "k_linkage_prim<%d, true>" % cols}
    # a view with a column stride goes through a contiguous copy
    t = z.T.contiguous().T
    assert t.stride(1) != 1
    assert np.array_equal(query.zmatrix_linkage(t, ctx=gpu_ctx), want[0])


def test_reference_semantics_of_asymmetric_and_nan_input(gpu_ctx):
    rng = np.random.default_rng(6)
    n = 300
    z = accumulated(gpu_ctx, rng, n, 4, 5)
    want_lk, want_order = reference(z.cpu().numpy())
    lower = torch.tril(torch.ones((n, n), dtype=torch.bool, device=z.device), diagonal=-1)
    # only the strict upper triangle counts
    asym = z.clone()
    asym[lower] = torch.rand(int(lower.sum()), device=z.device)
    assert not torch.equal(asym, asym.T)
    got_lk, got_order = reference(asym.cpu().numpy())
    assert np.array_equal(got_lk, want_lk)                                # (the reference itself ignores the rest)
    assert np.array_equal(query.zmatrix_linkage(asym, ctx=gpu_ctx), want_lk)
    assert np.array_equal(query.zmatrix_heuristic_block_ordering(asym, ctx=gpu_ctx), want_order)
    # NaN strictly below the diagonal and on it is ignored
    nan = z.clone()
    nan[lower] = float("nan")
    nan.fill_diagonal_(float("nan"))
    assert np.array_equal(query.zmatrix_linkage(nan, ctx=gpu_ctx), want_lk)
    assert np.array_equal(query.zmatrix_heuristic_block_ordering(nan, ctx=gpu_ctx), want_order)
    # above it scipy raises
    for bad in (float("nan"), float("inf")):
        up = z.clone()
        up[7, 250] = bad
        with pytest.raises(ValueError, match="finite"):
            reference(up.cpu().numpy())
        with pytest.raises(ValueError, match="finite"):
            query.zmatrix_linkage(up, ctx=gpu_ctx)
        with pytest.raises(ValueError, match="finite"):
            query.zmatrix_heuristic_block_ordering(up, ctx=gpu_ctx)
    # other dtypes and n < 2 go the host way, as before
    assert np.array_equal(query.zmatrix_heuristic_block_ordering(z.double(), ctx=gpu_ctx),
                          np.array(hier.leaves_list(hier.linkage(1. - z.double().cpu().numpy()[np.triu_indices(n, 1)]))))
    with pytest.raises(ValueError):
        query.zmatrix_heuristic_block_ordering(torch.ones((1, 1), device=z.device), ctx=gpu_ctx)
    with pytest.raises(ValueError, match="not a zmat"):
        query.zmatrix_linkage(torch.ones((3, 4), device=z.device), ctx=gpu_ctx)
    # without ctx: the module's own context on the tensor's device
    assert np.array_equal(query.zmatrix_linkage(z), want_lk)
    assert np.array_equal(query.zmatrix_heuristic_block_ordering(z), want_order)


def test_clusters_on_a_device_tensor(gpu_ctx):
    rng = np.random.default_rng(8)
    z = accumulated(gpu_ctx, rng, 500, 4, 6)
    lk, _ = reference(z.cpu().numpy())
    for thr in (0.25, 0.6, 1.0):
        got = query.zmatrix_clusters(z, thr, ctx=gpu_ctx)
        want = hier.fcluster(lk, 1. - thr, criterion="distance")
        assert np.array_equal(got[:, None] == got[None, :], want[:, None] == want[None, :])
        assert np.array_equal(got, query.zmatrix_clusters(z.cpu().numpy(), thr))


def test_accumulator_methods_and_block_diagonal_result(gpu_ctx):
    rng = np.random.default_rng(3)
    n, S, K = 777, 9, 5
    zm = common_amd.ZMatrix(gpu_ctx, n, K)
    zm.add(torch.from_numpy(rng.integers(0, K, (S, n)).astype(np.int32)).to(gpu_ctx.torch_device))
    res = zm.result()
    assert np.array_equal(zm.linkage(), query.zmatrix_linkage(res, ctx=gpu_ctx))
    assert np.array_equal(zm.block_ordering(), query.zmatrix_heuristic_block_ordering(res, ctx=gpu_ctx))
    assert np.array_equal(zm.block_ordering(), reference(res.cpu().numpy())[1])
    zm.close()
    # interleaved blocks: the ordered result is block diagonal (tests/test_query_cpu.py
    # test_heuristic_block_ordering_groups_blocks, on the device from end to end)
    a = np.tile(np.array([0, 1, 0, 1, 0, 1, 2, 2], dtype=np.int32), 40)
    zb = common_amd.ZMatrix(gpu_ctx, a.size, 3)
    at = torch.from_numpy(a).to(gpu_ctx.torch_device)
    for _ in range(3):
        zb.add(at)
    order = zb.block_ordering()
    assert sorted(order.tolist()) == list(range(a.size))
    labels = a[order]
    assert sum(labels[i] != labels[i + 1] for i in range(a.size - 1)) == 2
    block = zb.result(order=order).cpu().numpy()
    assert np.array_equal(block, np.eye(3, dtype=np.float32)[labels][:, labels])
    zb.close()


def test_argument_checks_of_the_c_entry(gpu_ctx):
    buf = torch.ones((4, 4), dtype=torch.float32, device=gpu_ctx.torch_device)
    out = np.zeros((3, 4), dtype=np.float64)
    fn = gpu_ctx.lib.msc_linkage_single

    def call(ptr, ld, n, flags=0):
        return fn(gpu_ctx._h, C.c_void_p(ptr), ld, n, flags, out.ctypes.data_as(C.c_void_p), None)
    assert call(buf.data_ptr(), 4, 4) == 0
    assert call(buf.data_ptr(), 4, 1) == -1                       # MSC_EINVAL: n < 2
    assert call(buf.data_ptr(), 4, 0) == -1
    assert call(buf.data_ptr(), 3, 4) == -1                       # ld < n
    assert call(None, 4, 4) == -1                                 # null z_dev
    assert call(buf.data_ptr(), 4, 4, flags=1) == -1              # no flag is defined
    assert call(buf.data_ptr(), 65537, 65537) == -4               # MSC_EUNSUPPORTED, before anything is launched
    assert "65536" in gpu_ctx.lib.msc_last_error().decode()
    assert call(buf.data_ptr(), 4, 4) == 0
    gpu_ctx.synchronize()
    with pytest.raises(ValueError):
        gpu_ctx.linkage_single(buf.double())


def test_faster_than_the_host_route_at_4096(gpu_ctx):
    """zmatrix_heuristic_block_ordering on a device-resident matrix against the route it took before (download, condensed
    copy, scipy), both wall clock after one warm-up call; no factor, only the order."""
    rng = np.random.default_rng(1)
    n = 4096
    z = accumulated(gpu_ctx, rng, n, 64, 24)

    def device_route():
        return query.zmatrix_heuristic_block_ordering(z, ctx=gpu_ctx)

    def host_route():
        h = z.cpu().numpy()
        dist = 1. - np.array(h[np.triu_indices(n, k=1)])
        return np.array(hier.leaves_list(hier.linkage(dist)))

    device_route()
    host_route()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = device_route()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = host_route()
    t_host = time.perf_counter() - t0
    print("n = 4096: device route %.4f s (%s), host route %.4f s" % (t_dev, gpu_ctx.last_kernel("zmatrix"), t_host))
    assert np.array_equal(got, want)
    assert t_dev < t_host
