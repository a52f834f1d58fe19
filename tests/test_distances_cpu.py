"""No GPU: the host path of common_amd.query's partition_distances / adjusted_rand / expected_loss / vi_estimate /
credible_ball -- the yardstick of tests/test_gpu_distances.py -- against first principles: brute-force pair counts,
entropies from probabilities, the metric axioms, the identities that tie the exact expected losses to partition_loss's
integers and to its variation-of-information bound, a hand-made credible ball, and the error paths."""
import numpy as np
import pytest

from common_amd import query

I32 = np.iinfo(np.int32)


def random_partitions(rng, n, m):
    out = np.empty((n, m), dtype=np.int64)
    for i in range(n):
        out[i] = rng.integers(-3, i, m) if i % 3 else rng.integers(0, max(2, m // 2), m) * 1000
    return out


def brute_binder(a, b):
    """row pairs that exactly one of the two partitions joins"""
    m = len(a)
    return sum(int((a[r] == a[s]) != (b[r] == b[s])) for r in range(m) for s in range(r + 1, m))


def entropy_vi(a, b):
    """H(a) + H(b) - 2 I(a; b) in bits, from the probabilities"""
    m = len(a)
    la, lb = np.unique(a), np.unique(b)
    p = np.array([[np.sum((a == x) & (b == y)) for y in lb] for x in la], dtype=np.float64) / m
    pa, pb = p.sum(axis=1), p.sum(axis=0)
    H = lambda q: -np.sum(q[q > 0] * np.log2(q[q > 0]))
    nz = p > 0
    mutual = np.sum(p[nz] * np.log2(p[nz] / np.outer(pa, pb)[nz]))
    return H(pa) + H(pb) - 2.0 * mutual


@pytest.mark.parametrize("m", [1, 2, 7, 40])
def test_binder_and_vi_against_first_principles(m):
    rng = np.random.default_rng(m)
    A, B = random_partitions(rng, 5, m), random_partitions(rng, 4, m)
    A[0], B[0] = 7, np.arange(m)                                # all in one, all singletons
    d = query.partition_distances(A, B)
    assert d.binder.dtype == np.int64 and d.vi.dtype == np.float64 and d.binder.shape == d.vi.shape == (5, 4)
    for i in range(5):
        for j in range(4):
            assert d.binder[i, j] == brute_binder(A[i], B[j])
            assert abs(d.vi[i, j] - entropy_vi(A[i], B[j])) <= 1e-12 * max(1.0, np.log2(m))
    assert d.nclusters_a.tolist() == [np.unique(a).size for a in A]
    assert d.nclusters_b.tolist() == [np.unique(b).size for b in B]
    assert d.nclusters_a[0] == 1 and d.nclusters_b[0] == m
    same = sum(r for r in range(m))                             # C(m, 2): every pair is joined by all-in-one
    assert d.pairs_ab[0, 0] == 0 and d.binder[0, 0] == same


def test_metric_axioms():
    rng = np.random.default_rng(3)
    m = 60
    P = random_partitions(rng, 12, m)
    d = query.partition_distances(P)
    assert np.array_equal(d.vi.diagonal(), np.zeros(12)) and np.array_equal(d.binder.diagonal(), np.zeros(12, dtype=np.int64))
    assert np.array_equal(d.vi, d.vi.T) and np.array_equal(d.binder, d.binder.T)
    both = query.partition_distances(P, P)
    assert np.array_equal(both.vi, d.vi) and np.array_equal(both.binder, d.binder)
    assert (d.vi[~np.eye(12, dtype=bool)] > 0).all()            # (the random partitions are distinct)
    relabelled = 5 - 3 * P                                      # the same partitions under other names
    assert np.array_equal(query.partition_distances(P, relabelled).vi.diagonal(), np.zeros(12))
    for i in range(12):
        for j in range(12):
            for k in range(12):
                assert d.vi[i, k] <= d.vi[i, j] + d.vi[j, k] + 1e-12
                assert d.binder[i, k] <= d.binder[i, j] + d.binder[j, k]
    # one vector against one vector
    one = query.partition_distances(P[0], P[1])
    assert one.vi.shape == (1, 1) and one.vi[0, 0] == d.vi[0, 1]


def test_extreme_and_negative_labels():
    rng = np.random.default_rng(8)
    m = 50
    small = rng.integers(0, 4, m)
    names = np.array([I32.min, -1, 0, I32.max], dtype=np.int64)
    wide = np.array([-2 ** 62, -5, 2 ** 40, 2 ** 62], dtype=np.int64)
    other = rng.integers(0, 3, m)
    want = query.partition_distances(small, other)
    for lab in (names[small], names[small].astype(np.int32), wide[small]):
        got = query.partition_distances(lab, other)
        assert np.array_equal(got.binder, want.binder) and np.array_equal(got.vi, want.vi)


def test_adjusted_rand():
    rng = np.random.default_rng(4)
    m = 400
    P = random_partitions(rng, 6, m)
    ari = query.adjusted_rand(P, 11 * P + 2)
    assert ari.dtype == np.float64 and np.array_equal(ari.diagonal(), np.ones(6))
    assert np.array_equal(query.adjusted_rand(P), query.adjusted_rand(P, P))
    # the textbook form on one pair
    a, b = P[1], P[2]
    d = query.partition_distances(a, b)
    pa = sum(int(np.sum(a == x)) * (int(np.sum(a == x)) - 1) // 2 for x in np.unique(a))
    pb = sum(int(np.sum(b == x)) * (int(np.sum(b == x)) - 1) // 2 for x in np.unique(b))
    E = pa * pb / (m * (m - 1) / 2)
    assert abs(query.adjusted_rand(a, b)[0, 0] - (int(d.pairs_ab[0, 0]) - E) / ((pa + pb) / 2 - E)) <= 1e-14
    # independent partitions: the index has mean 0 and a standard deviation of order 1 / m for a few balanced clusters
    # (Hubert and Arabie's permutation model); 200 draws, every one within 0.05 and their mean within 0.01
    X, Y = rng.integers(0, 4, (200, m)), rng.integers(0, 5, (1, m))
    ind = query.adjusted_rand(X, Y)[:, 0]
    assert np.abs(ind).max() < 0.05 and abs(ind.mean()) < 0.01
    # a zero denominator: both all-in-one, both singletons, a single row
    assert query.adjusted_rand(np.zeros(9, dtype=int), np.ones(9, dtype=int))[0, 0] == 1.0
    assert query.adjusted_rand(np.arange(9), np.arange(9)[::-1].copy())[0, 0] == 1.0
    assert query.adjusted_rand(np.array([3]), np.array([4]))[0, 0] == 1.0
    assert query.adjusted_rand(np.zeros(9, dtype=int), np.arange(9))[0, 0] == 0.0


def samples_and_candidates(rng, S=37, m=300):
    truth = rng.integers(0, 6, m)
    A = np.tile(truth, (S, 1))
    flip = rng.random((S, m)) < 0.3
    A[flip] = rng.integers(0, 8, int(flip.sum()))
    A[0], A[1], A[2] = 0, np.arange(m), rng.choice(np.array([I32.min, I32.max, -1]), m)
    cands = np.concatenate([A[:6], random_partitions(rng, 5, m), np.arange(m)[None]])
    return A, cands


def test_expected_loss_ties_to_partition_loss():
    rng = np.random.default_rng(37)
    A, cands = samples_and_candidates(rng)
    S, m = A.shape
    got = query.expected_loss(list(A), cands)
    binder, vi_lb, valid = query.partition_loss(list(A), cands)
    assert got.valid == valid == S and got.binder_num.dtype == np.int64
    assert np.array_equal(got.binder_num, binder)               # exactly: the same integer from the samples and from the counts
    # Jensen: E[VI] >= the bound, once its candidate-independent term (1 / (m S)) sum_s nlogn_s is put back
    term = sum(float(np.sum(n * np.log2(n))) for n in (np.unique(a, return_counts=True)[1].astype(float) for a in A)) / (m * S)
    assert (got.vi >= vi_lb + term - 1e-9).all()
    assert (got.vi[:-1] > vi_lb[:-1] + term + 1e-6).any()       # and it is no identity
    assert abs(got.vi[-1] - (vi_lb[-1] + term)) <= 1e-9         # all singletons: equality
    # the definition, pair by pair
    d = query.partition_distances(cands, A)
    assert np.array_equal(got.binder_num, d.binder.sum(axis=1))
    for c in range(cands.shape[0]):
        acc = 0.0
        for s in range(S):
            acc += d.vi[c, s]
        assert got.vi[c] == acc / S
    own = query.expected_loss(list(A))
    assert np.array_equal(own.binder_num, query.partition_loss(list(A), A)[0])
    assert np.array_equal(own.vi[:6], got.vi[:6])


def test_vi_estimate():
    rng = np.random.default_rng(5)
    A, cands = samples_and_candidates(rng, S=20, m=80)
    est = query.vi_estimate(list(A), cands)
    losses = query.expected_loss(list(A), cands).vi
    assert isinstance(est, query.PointEstimate) and np.array_equal(est.losses, losses)
    assert est.index == int(np.argmin(losses)) and np.array_equal(est.labels, query._renumber(cands[est.index]))
    binder_est = query.point_estimate(list(A), "binder", candidates=cands[est.index:est.index + 1])
    assert np.array_equal(est.confidence, binder_est.confidence)          # computed as point_estimate computes it
    twice = np.concatenate([cands, cands])
    assert query.vi_estimate(list(A), twice).index == est.index           # the lowest index among equals
    own = query.vi_estimate(list(A))
    assert own.index == int(np.argmin(query.expected_loss(list(A)).vi)) and own.losses.shape == (20,)


def test_credible_ball_by_hand():
    # ten samples of four rows around the estimate {0, 1}{2, 3}; Binder distances by hand:
    est = np.array([0, 0, 1, 1])
    S = np.array([[0, 0, 1, 1],      # 0            2 clusters
                  [5, 5, 9, 9],      # 0            2
                  [0, 0, 1, 2],      # 1            3
                  [0, 1, 2, 2],      # 1            3
                  [0, 0, 0, 1],      # 3            2   ({0,1,2}: joins 02, 12; separates 23)
                  [0, 1, 2, 3],      # 2            4
                  [0, 0, 0, 0],      # 4            1
                  [0, 1, 0, 1],      # 4            2
                  [0, 1, 1, 1],      # 3            2
                  [0, 1, 2, 3]])     # 2            4
    want = np.array([0, 0, 1, 1, 3, 2, 4, 4, 3, 2])
    ball = query.credible_ball(list(S), est, level=0.75, metric="binder")
    assert np.array_equal(ball.distances, want) and ball.distances.dtype == np.int64
    assert ball.nclusters.tolist() == [2, 2, 3, 3, 2, 4, 1, 2, 2, 4]
    # ceil(7.5) = 8: the 8th smallest of 0 0 1 1 2 2 3 3 4 4 is 3, and BOTH samples at 3 are in (a tie at the radius)
    assert ball.radius == 3 and ball.members.tolist() == [True] * 6 + [False, False, True, True]
    assert ball.horizontal.tolist() == [4, 8]
    assert ball.upper.tolist() == [4, 8]                        # fewest clusters among the members: 2; the farthest of those
    assert ball.lower.tolist() == [5, 9]                        # most clusters: 4
    every = query.credible_ball(list(S), est, level=1.0, metric="binder")
    assert every.radius == 4 and every.members.all() and every.horizontal.tolist() == [6, 7]
    assert every.upper.tolist() == [6] and every.lower.tolist() == [5, 9]
    least = query.credible_ball(list(S), est, level=0.05, metric="binder")
    assert least.radius == 0 and least.members.tolist() == [True, True] + [False] * 8
    assert least.horizontal.tolist() == least.upper.tolist() == least.lower.tolist() == [0, 1]
    vi = query.credible_ball(list(S), est, level=0.75)          # "vi" is the default; these distances are multiples of 1/2
    assert np.array_equal(vi.distances, query.partition_distances(est, S).vi[0])
    assert vi.distances[0] == 0.0 and vi.distances[6] == 1.0 and vi.distances[5] == 1.0 and vi.distances[7] == 2.0
    assert vi.radius == np.sort(vi.distances)[7] and np.array_equal(vi.members, vi.distances <= vi.radius)


def test_error_paths():
    A = np.arange(12).reshape(3, 4) % 3
    with pytest.raises(ValueError, match="integer"):
        query.partition_distances(A.astype(float))
    with pytest.raises(ValueError, match="empty"):
        query.partition_distances(np.zeros((0, 4), dtype=int))
    with pytest.raises(ValueError, match="empty"):
        query.partition_distances(np.zeros((2, 0), dtype=int))
    with pytest.raises(ValueError, match="rows"):
        query.partition_distances(A, A[:, :3])
    with pytest.raises(ValueError, match="metric"):
        query.credible_ball(list(A), A[0], metric="rand")
    for level in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            query.credible_ball(list(A), A[0], level=level)
    with pytest.raises(ValueError, match="one vector"):
        query.credible_ball(list(A), A[:2])
    with pytest.raises(ValueError, match="size"):
        query.credible_ball(list(A), A[0, :3])
    with pytest.raises(ValueError, match="size"):
        query.expected_loss(list(A), A[:, :3])
    with pytest.raises(ValueError, match="empty"):
        query.expected_loss([])
    with pytest.raises(ValueError, match="same size"):
        query.expected_loss([[0, 1], [0, 1, 2]])
    with pytest.raises(ValueError, match="integer"):
        query.expected_loss(list(A.astype(float)))
    # point_estimate is as it was: the exact VI is another entry point
    with pytest.raises(ValueError, match="loss"):
        query.point_estimate(list(A), loss="evi")
