"""GPU: distances between partitions (msc_partition_distances, Context.partition_distances, common_amd.query's
partition_distances / adjusted_rand / expected_loss / vi_estimate / credible_ball on device tensors) against the host path
of the same module, which tests/test_distances_cpu.py holds against first principles.

Gates.  Every integer is bit-equal.  |nlogn_dev - nlogn_host| <= 2^-52 (m + 16) max(1, nlogn_host): an ulp for each log2
and a sum of m non-negative terms in any order; vi at the same factor times (nlogn_a + nlogn_b + 2 nlogn_ab) / m.  Every
comparison prints its largest error as a share of the gate.

Shapes: every m at which the pair kernel changes its instantiation (1024 | 1025, 4096 | 4097, 16384 | 16385) and the
wave and block edges below; ld > m with junk behind the rows; the extreme int32 labels; all-in-one partitions (the
wave-uniform add), singletons, exactly 1024 clusters; cluster counts on both sides of the LDS / global boundary of the
table (K_a K_b <= 15360); partition counts beyond one tile (8) and one chunk (256)."""
import numpy as np
import pytest
import torch

import common_amd
from common_amd import query
from common_amd._lib import DISTANCES_LDS_CELLS, DISTANCES_MAX_CLUSTERS, DISTANCES_MAX_ROWS

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
EPS = 2.0 ** -52


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def padded(ctx, a, extra=5):
    """the partitions as a view of a wider tensor: ld = m + extra, junk behind every row"""
    a = np.asarray(a, dtype=np.int32)
    wide = np.full((a.shape[0], a.shape[1] + extra), 123456789, dtype=np.int32)
    wide[:, ::2] = -77
    wide[:, :a.shape[1]] = a
    return dev(ctx, wide)[:, :a.shape[1]]


def with_clusters(rng, m, k):
    """a random partition of m rows with exactly k clusters, labels anywhere in int32"""
    lab = np.concatenate([np.arange(k), rng.integers(0, k, m - k)])
    rng.shuffle(lab)
    names = rng.choice(np.arange(-3 * k, 3 * k), size=k, replace=False)
    return names[lab].astype(np.int32)


def mixed(rng, m, n):
    """n partitions: all-in-one, singletons (or 1000 clusters), the extreme labels, then random ones of few and many"""
    out = np.empty((n, m), dtype=np.int32)
    for i in range(n):
        kind = i % 5
        if kind == 0:
            out[i] = -5
        elif kind == 1:
            out[i] = np.arange(m) if m <= DISTANCES_MAX_CLUSTERS else with_clusters(rng, m, 1000)
        elif kind == 2:
            out[i] = rng.choice(np.array([I32.min, I32.max, -1, 0, 1], dtype=np.int64), m).astype(np.int32)
        elif kind == 3:
            out[i] = with_clusters(rng, m, min(m, 3))
        else:
            out[i] = with_clusters(rng, m, min(m, 40 + i))
    return out


def against_host(ctx, A, B, a_dev=None, b_dev=None):
    """the device's eight outputs against the host path's; the largest error as a share of its gate"""
    A = np.asarray(A)
    m = A.shape[1]
    got = ctx.partition_distances(dev(ctx, A) if a_dev is None else a_dev,
                                  None if B is None else (dev(ctx, B) if b_dev is None else b_dev))
    ctx.synchronize()
    got = [g.cpu().numpy() for g in got]
    want = query._sums_host(A, None if B is None else np.asarray(B))
    share = 0.0
    for idx in (0, 2, 4, 5, 7):                                 # pairs_ab, pairs_a, nclusters_a, pairs_b, nclusters_b
        assert got[idx].dtype == want[idx].dtype and np.array_equal(got[idx], want[idx]), idx
    for idx in (1, 3, 6):                                       # nlogn_ab, nlogn_a, nlogn_b
        gate = EPS * (m + 16) * np.maximum(1.0, want[idx])
        err = np.abs(got[idx] - want[idx])
        assert (err <= gate).all(), (idx, float((err / gate).max()))
        share = max(share, float((err / gate).max()))
    _, vi_got = query._binder_vi(got, m)
    _, vi_want = query._binder_vi(want, m)
    gate = EPS * (m + 16) * (want[3][:, None] + want[6][None, :] + 2.0 * want[1]) / m
    err = np.abs(vi_got - vi_want)
    assert (err <= gate).all()
    vshare = float(np.where(gate > 0, err / np.where(gate > 0, gate, 1.0), 0.0).max())
    print("m = %d, %d x %d: nlogn at %.3f of its gate, vi at %.3f" % (m, got[0].shape[0], got[0].shape[1], share, vshare))
    return got


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 257, 1000, 1024, 1025, 4096, 4097, 16385, DISTANCES_MAX_ROWS])
def test_every_row_count_against_the_host(gpu_ctx, m):
    rng = np.random.default_rng(m)
    A, B = mixed(rng, m, 5), mixed(rng, m, 7)[2:]
    against_host(gpu_ctx, A, B, a_dev=padded(gpu_ctx, A), b_dev=padded(gpu_ctx, B, 3))
    against_host(gpu_ctx, A, None, a_dev=padded(gpu_ctx, A, 1))


def test_both_sides_of_the_table_boundary(gpu_ctx):
    """K_a K_b = 15360 stays in LDS, 15367 does not; 1024 clusters against 15 | 16 and against 1024"""
    assert DISTANCES_LDS_CELLS == 120 * 128
    rng = np.random.default_rng(5)
    m = 1500
    names = []
    for ka, kb in ((120, 128), (1024, 15), (1, 1024), (121, 127), (1024, 16), (1024, 1024)):
        A = np.stack([with_clusters(rng, m, ka), with_clusters(rng, m, ka)])
        B = np.stack([with_clusters(rng, m, kb)])
        got = against_host(gpu_ctx, A, B)
        assert got[4].tolist() == [ka, ka] and got[7].tolist() == [kb]
        names.append(gpu_ctx.last_kernel("zmatrix"))
    assert len(set(names[:3])) == 1 and len(set(names[3:])) == 1 and names[0] != names[3]      # both routes ran
    # one call whose pairs take different routes: 2 x 1024 in LDS, 16 x 1024 and 1024 x 1024 not
    A = np.stack([with_clusters(rng, m, k) for k in (2, 16, 1024, 1)])
    against_host(gpu_ctx, A, None)


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 65), (7, 7), (65, 1), (65, 65), (7, 65)])
def test_partition_counts_beyond_a_tile(gpu_ctx, na, nb):
    rng = np.random.default_rng(na * 100 + nb)
    m = 97
    against_host(gpu_ctx, mixed(rng, m, na), mixed(rng, m, nb + 1)[1:])


def raw(ctx, a, b=None):
    out = ctx.partition_distances(a, b)
    ctx.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(x, y):
    return all(np.array_equal(p.view(np.int64) if p.dtype == np.float64 else p, q.view(np.int64) if q.dtype == np.float64 else q)
               for p, q in zip(x, y))


def test_beyond_a_chunk_and_the_same_bits_under_any_split(gpu_ctx):
    """300 x 290 partitions, more than a chunk of 256 on both sides: the whole call against its pieces (each within a
    chunk), the rows and columns at the chunk's edge against the host, the same call twice, (b, a) transposed, b = None"""
    rng = np.random.default_rng(11)
    m = 130
    A, B = mixed(rng, m, 300), mixed(rng, m, 291)[1:]
    A[7], B[3] = with_clusters(rng, m, 128), with_clusters(rng, m, 121)       # 128 x 121 cells: a pair of the global route
    a, b = dev(gpu_ctx, A), dev(gpu_ctx, B)
    whole = raw(gpu_ctx, a, b)
    assert same_bits(whole, raw(gpu_ctx, a, b))
    for cut_a, cut_b in ((256, 256), (1, 289), (150, 7)):
        parts = [[raw(gpu_ctx, a[i0:i1], b[j0:j1]) for j0, j1 in ((0, cut_b), (cut_b, 290))]
                 for i0, i1 in ((0, cut_a), (cut_a, 300))]
        for idx in (0, 1):
            glued = np.block([[parts[0][0][idx], parts[0][1][idx]], [parts[1][0][idx], parts[1][1][idx]]])
            assert same_bits([glued], [whole[idx]])
        for idx in (2, 3, 4):
            assert same_bits([np.concatenate([parts[0][0][idx], parts[1][0][idx]])], [whole[idx]])
        for idx in (5, 6, 7):
            assert same_bits([np.concatenate([parts[0][0][idx], parts[0][1][idx]])], [whole[idx]])
    edge = against_host(gpu_ctx, A[250:262], B[250:262])
    assert same_bits([edge[0], edge[1]], [whole[0][250:262, 250:262], whole[1][250:262, 250:262]])
    swapped = raw(gpu_ctx, b, a)
    assert same_bits([swapped[0].T, swapped[1].T, swapped[5], swapped[6]], [whole[0], whole[1], whole[2], whole[3]])
    itself = raw(gpu_ctx, a)
    assert same_bits(itself, raw(gpu_ctx, a, a))
    assert same_bits([itself[0], itself[1]], [itself[0].T, itself[1].T])
    assert same_bits(itself[2:5], itself[5:8])


def planted(rng, S, m, k, noise):
    truth = rng.integers(0, k, m)
    out = np.tile(truth, (S, 1))
    flip = rng.random((S, m)) < noise
    out[flip] = rng.integers(0, k + 2, int(flip.sum()))
    return out.astype(np.int32)


def test_summed_binder_is_the_accumulators_binder_num(gpu_ctx):
    rng = np.random.default_rng(37)
    S, m = 37, 300
    A = planted(rng, S, m, 6, 0.3)
    A[0], A[1] = 0, np.arange(m)
    cands = mixed(rng, m, 9)
    got = query.expected_loss(dev(gpu_ctx, A), dev(gpu_ctx, cands))
    zm = common_amd.ZMatrix(gpu_ctx, m, int(A.max()) + 1)
    try:
        zm.add(dev(gpu_ctx, A))
        binder, _, valid = zm.partition_loss(dev(gpu_ctx, cands))
    finally:
        zm.close()
    assert isinstance(got.binder_num, torch.Tensor) and got.binder_num.dtype == torch.int64
    assert valid == got.valid == S and torch.equal(got.binder_num, binder)
    want = query.expected_loss(list(A), cands)
    assert np.array_equal(got.binder_num.cpu().numpy(), want.binder_num)
    gate = EPS * (m + 16) * 4.0 * np.log2(m)                   # (nlogn_a + nlogn_b + 2 nlogn_ab) / m <= 4 log2 m
    err = np.abs(got.vi.cpu().numpy() - want.vi)
    print("expected VI at %.3f of its gate" % float((err / gate).max()))
    assert (err <= gate).all()
    own = query.expected_loss(dev(gpu_ctx, A))                  # the samples are the candidates
    assert np.array_equal(own.binder_num.cpu().numpy(), query.expected_loss(list(A)).binder_num)


def test_query_functions_on_device_tensors(gpu_ctx):
    rng = np.random.default_rng(3)
    m = 211
    A, B = mixed(rng, m, 6), mixed(rng, m, 4)
    want = query.partition_distances(A, B)
    for got in (query.partition_distances(dev(gpu_ctx, A), dev(gpu_ctx, B)), query.partition_distances(A, B, ctx=gpu_ctx),
                query.partition_distances([dev(gpu_ctx, a) for a in A], B.astype(np.int64))):
        assert isinstance(got.vi, torch.Tensor) and got.binder.dtype == torch.int64 and got.vi.dtype == torch.float64
        assert np.array_equal(got.binder.cpu().numpy(), want.binder)
        assert np.array_equal(got.pairs_ab.cpu().numpy(), want.pairs_ab)
        assert np.array_equal(got.nclusters_a.cpu().numpy(), want.nclusters_a)
        assert np.array_equal(got.nclusters_b.cpu().numpy(), want.nclusters_b)
        assert np.abs(got.vi.cpu().numpy() - want.vi).max() <= EPS * (m + 16) * 4.0 * np.log2(m)
    # the adjusted Rand index: five float64 operations on the same integers, values of magnitude at most about 1
    ari = query.adjusted_rand(dev(gpu_ctx, A), dev(gpu_ctx, B))
    assert isinstance(ari, torch.Tensor) and np.abs(ari.cpu().numpy() - query.adjusted_rand(A, B)).max() <= 1e-12
    assert np.array_equal(np.diag(query.adjusted_rand(dev(gpu_ctx, A)).cpu().numpy()), np.ones(6))


def test_credible_ball_and_vi_estimate_on_the_device(gpu_ctx):
    rng = np.random.default_rng(21)
    S, m = 40, 150
    A = planted(rng, S, m, 5, 0.25)
    est = planted(rng, 1, m, 5, 0.0)[0]
    want = query.credible_ball(list(A), est, 0.9, "binder")
    got = query.credible_ball(dev(gpu_ctx, A), est, 0.9, "binder")
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    want = query.credible_ball(list(A), est, 0.9, "vi")
    gate = EPS * (m + 16) * 4.0 * np.log2(m)
    # the ball is decided at the radius and at the largest distances within each bound: every distinct distance of the host's
    # is further from its neighbours than the gate, so the device orders the samples as the host does
    distinct = np.unique(want.distances)
    assert np.diff(distinct).min() > 4 * gate
    got = query.credible_ball(dev(gpu_ctx, A), dev(gpu_ctx, est), 0.9, "vi")
    assert np.abs(got.distances - want.distances).max() <= gate and abs(got.radius - want.radius) <= gate
    for name in ("members", "horizontal", "upper", "lower", "nclusters"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    cands = np.concatenate([A[:10], mixed(rng, m, 5)])
    want = query.vi_estimate(list(A), candidates=cands)
    best = np.sort(want.losses)[:2]
    assert best[1] - best[0] > 4 * gate
    for got in (query.vi_estimate(dev(gpu_ctx, A), candidates=dev(gpu_ctx, cands)), query.vi_estimate(list(A), cands, ctx=gpu_ctx)):
        assert got.index == want.index and np.array_equal(got.labels, want.labels)
        assert np.abs(got.losses - want.losses).max() <= gate
        assert np.array_equal(got.confidence, want.confidence)
    own, own_want = query.vi_estimate(dev(gpu_ctx, A)), query.vi_estimate(list(A))
    best = np.sort(own_want.losses)[:2]
    if best[1] - best[0] > 4 * gate:
        assert own.index == own_want.index and np.array_equal(own.labels, own_want.labels)
    assert np.abs(own.losses - own_want.losses).max() <= gate


def test_error_paths(gpu_ctx):
    rng = np.random.default_rng(1)
    m = DISTANCES_MAX_CLUSTERS + 40
    ok = dev(gpu_ctx, mixed(rng, m, 2))
    many = dev(gpu_ctx, np.stack([with_clusters(rng, m, DISTANCES_MAX_CLUSTERS + 1)]))
    with pytest.raises(ValueError, match="1025 clusters"):
        gpu_ctx.partition_distances(ok, many)
    with pytest.raises(ValueError, match="1025 clusters"):
        query.partition_distances(many.cpu().numpy(), ctx=gpu_ctx)
    big = torch.zeros((1, DISTANCES_MAX_ROWS + 1), dtype=torch.int32, device=gpu_ctx.torch_device)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.partition_distances(big)
    assert e.value.code == -4                                   # MSC_EUNSUPPORTED
    for bad in (ok.to(torch.int64), ok.cpu(), ok.T, ok[:, ::2], ok.to(torch.float32), ok.reshape(2, 2, -1),
                ok[:0], ok[:, :0], None):
        with pytest.raises(ValueError):
            gpu_ctx.partition_distances(bad)
    with pytest.raises(ValueError, match="same rows"):
        gpu_ctx.partition_distances(ok, ok[:, :-1].contiguous())
    with pytest.raises(ValueError, match="keeps counts"):
        zm = common_amd.ZMatrix(gpu_ctx, 8, 4)
        try:
            query.expected_loss(zm)
        finally:
            zm.close()
    gpu_ctx.synchronize()                                       # nothing was launched, nothing was reported
    against_host(gpu_ctx, ok.cpu().numpy(), None)


def test_the_c_entry_point_itself(gpu_ctx):
    """MSC_EINVAL for what the header lists, nothing computed when no pair output is asked for, and a partition with more
    than 1024 clusters found on the device: -1 / NaN in every output it takes part in, MSC_EDEVICE at the next wait"""
    import ctypes as C
    rng = np.random.default_rng(2)
    m = DISTANCES_MAX_CLUSTERS + 30
    A = np.stack([with_clusters(rng, m, 9), with_clusters(rng, m, DISTANCES_MAX_CLUSTERS + 1), with_clusters(rng, m, 1024)])
    B = mixed(rng, m, 11)
    a, b = dev(gpu_ctx, A), dev(gpu_ctx, B)
    lib, ptr = gpu_ctx.lib, lambda t: C.c_void_p(t.data_ptr())
    none = [None] * 8

    def call(h, pa, lda, na, pb, ldb, nb, rows, flags=0, outs=none):
        return lib.msc_partition_distances(h, pa, lda, na, pb, ldb, nb, rows, flags, *outs)
    assert call(None, ptr(a), m, 3, ptr(b), m, 11, m) == -1               # no context
    assert call(gpu_ctx._h, None, m, 3, ptr(b), m, 11, m) == -1           # no a
    assert call(gpu_ctx._h, ptr(a), m, 0, ptr(b), m, 11, m) == -1         # na == 0
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m, 0, m) == -1          # nb == 0
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m, 11, 0) == -1         # m == 0
    assert call(gpu_ctx._h, ptr(a), m - 1, 3, ptr(b), m, 11, m) == -1     # lda < m
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m - 1, 11, m) == -1     # ldb < m
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m, 11, m, flags=1) == -1
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m, 11, DISTANCES_MAX_ROWS + 1) == -1     # (lda < m comes first)
    assert call(gpu_ctx._h, ptr(a), 1 << 20, 3, None, 0, 0, DISTANCES_MAX_ROWS + 1) == -4  # MSC_EUNSUPPORTED, nothing read
    assert call(gpu_ctx._h, ptr(a[:1]), m, 1, ptr(b), m, 11, m) == 0      # nothing asked for
    gpu_ctx.synchronize()
    t = gpu_ctx.torch_device
    pairs_ab = torch.zeros((3, 11), dtype=torch.int64, device=t)
    nlogn_ab = torch.zeros((3, 11), dtype=torch.float64, device=t)
    pa, la, ka = (torch.zeros(3, dtype=d, device=t) for d in (torch.int64, torch.float64, torch.int32))
    assert call(gpu_ctx._h, ptr(a), m, 3, ptr(b), m, 11, m, outs=[ptr(pairs_ab), ptr(nlogn_ab), ptr(pa), ptr(la), ptr(ka),
                                                                   None, None, None]) == 0
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == -6 and "1024 clusters" in str(e.value) and "detail of the first: 1]" in str(e.value)
    gpu_ctx.synchronize()                                                 # (read and cleared)
    want = query._sums_host(A[[0, 2]], B)
    assert np.array_equal(pairs_ab.cpu().numpy()[[0, 2]], want[0]) and (pairs_ab[1] == -1).all()
    assert bool(torch.isnan(nlogn_ab[1]).all()) and not bool(torch.isnan(nlogn_ab[[0, 2]]).any())
    assert pa.tolist() == [int(want[2][0]), -1, int(want[2][1])] and ka.tolist() == [9, -1, 1024]
    assert bool(torch.isnan(la[1])) and not bool(torch.isnan(la[[0, 2]]).any())
    against_host(gpu_ctx, A[[0, 2]], B)                                   # the context is as good as before
