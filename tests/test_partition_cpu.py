"""Point-estimate clustering from posterior samples, host side: common_amd.query.partition_sums / partition_loss /
point_estimate on numpy input against a hand-worked case, a plain triple loop, the brute-force pair sum of Binder's loss
and all 203 set partitions of six rows (the Binder minimiser, the VI lower bound against the true expected VI); the
renumbering, the tie rule, the confidence and every ValueError; and the two msc_zmatrix_partition_* entries in the
header, the binding and the built library.  No device needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import common_amd
from common_amd import _lib as L
from common_amd import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("msc_zmatrix_partition_sums", "msc_zmatrix_partition_loss")


def pair_counts(A):
    A = np.asarray(A)
    return (A[:, :, None] == A[:, None, :]).sum(0).astype(np.int64)


def loop_sums(A, cands):
    """w and size by the definition, one (candidate, a, b) at a time"""
    C = pair_counts(A)
    n = C.shape[0]
    w = np.zeros((len(cands), n), dtype=np.int64)
    size = np.zeros((len(cands), n), dtype=np.int64)
    for k, c in enumerate(cands):
        for a in range(n):
            for b in range(n):
                if c[a] == c[b]:
                    w[k, a] += C[a, b]
                    size[k, a] += 1
    return w, size


def brute_binder(A, c):
    """V * sum_{a<b} |delta_c(a, b) - Z_ab| in integers"""
    C, V = pair_counts(A), len(A)
    n = C.shape[0]
    return sum(abs(V * int(c[a] == c[b]) - int(C[a, b])) for a in range(n) for b in range(a + 1, n))


def set_partitions(n):
    """every partition of n rows as a restricted growth string"""
    out = []

    def grow(prefix, top):
        if len(prefix) == n:
            out.append(list(prefix))
            return
        for v in range(top + 2):
            grow(prefix + [v], max(top, v))
    grow([0], 0)
    return np.array(out, dtype=np.int64)


def vi(c, s):
    """the variation of information of two partitions, in bits"""
    c, s = np.asarray(c), np.asarray(s)
    n = c.size
    out = 0.0
    for a in range(n):
        nc, ns = (c == c[a]).sum(), (s == s[a]).sum()
        both = ((c == c[a]) & (s == s[a])).sum()
        out += np.log2(nc) + np.log2(ns) - 2. * np.log2(both)
    return out / n


def test_hand_worked_three_rows():
    A = [[0, 0, 1], [0, 0, 0], [5, 7, 7], [2, 2, 3]]
    # C = [[4 3 1] [3 4 2] [1 2 4]], V = 4, T = 6
    cands = [[0, 0, 0], [9, 9, -1], [1, 2, 3], [4, 6, 6]]
    w, size = query.partition_sums(A, cands)
    assert w.dtype == np.int64 and size.dtype == np.int32
    assert w.tolist() == [[8, 9, 7], [7, 7, 4], [4, 4, 4], [4, 6, 6]]
    assert size.tolist() == [[3, 3, 3], [2, 2, 1], [1, 1, 1], [1, 2, 2]]
    binder, vi_lb, valid = query.partition_loss(A, cands)
    # T + V P - 2 Q: all-in-one 6 + 12 - 12; {01}{2} 6 + 4 - 6; singletons 6; {0}{12} 6 + 4 - 4
    assert binder.dtype == np.int64 and binder.tolist() == [6, 4, 6, 6] and valid == 4
    assert vi_lb.dtype == np.float64
    want = (3 * np.log2(3.) - 2 * (np.log2(8.) + np.log2(9.) + np.log2(7.))) / 3 + 4.
    assert abs(vi_lb[0] - want) < 1e-12 and vi_lb[2] == 0.0
    # one candidate as a plain vector
    assert query.partition_loss(A, cands[1])[0].tolist() == [4]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sums_against_the_triple_loop(seed):
    rng = np.random.default_rng(seed)
    n, S = 23 + seed, 9
    A = rng.integers(0, 5, (S, n))
    cands = np.concatenate([rng.integers(-3, 4, (4, n)),                       # negative labels
                            rng.integers(100, 103, (2, n)),                    # labels no sample holds
                            np.array([[np.iinfo(np.int32).min, -1, np.iinfo(np.int32).max][i % 3] for i in range(n)])[None],
                            A[:2]])
    w, size = query.partition_sums(list(A), cands)
    lw, ls = loop_sums(A, cands)
    assert np.array_equal(w, lw) and np.array_equal(size, ls)
    assert (w >= S).all()
    binder, _, valid = query.partition_loss(A, cands)
    assert valid == S
    assert binder.tolist() == [brute_binder(A, c) for c in cands]
    assert (binder >= 0).all()


def test_all_partitions_of_six_rows():
    rng = np.random.default_rng(11)
    n, S = 6, 7
    A = rng.integers(0, 3, (S, n))
    parts = set_partitions(n)
    assert parts.shape == (203, n)
    binder, vi_lb, valid = query.partition_loss(A, parts)
    brute = np.array([brute_binder(A, c) for c in parts])
    assert np.array_equal(binder, brute)
    est = query.point_estimate(A, "binder", candidates=parts)
    assert est.index == int(np.argmin(brute)) and brute[est.index] == brute.min()
    assert np.array_equal(est.losses, brute)
    # the dropped term, and the bound: vi_lb + it <= the expected VI of every candidate
    dropped = np.mean([[np.log2((s == s[a]).sum()) for a in range(n)] for s in A])
    true_vi = np.array([np.mean([vi(c, s) for s in A]) for c in parts])
    assert (vi_lb + dropped <= true_vi + 1e-12).all()
    est_vi = query.point_estimate(A, "vi", candidates=parts)
    assert est_vi.index == int(np.argmin(vi_lb)) and np.array_equal(est_vi.losses, vi_lb)
    singles = int(np.flatnonzero((parts == np.arange(n)).all(axis=1))[0])
    assert vi_lb[singles] == 0.0


def test_point_estimate_renumbering_ties_and_confidence():
    A = np.array([[7, 7, 3, 3, 9], [7, 7, 3, 3, 3], [1, 1, 2, 2, 5], [4, 4, 4, 6, 6]])
    est = query.point_estimate(A)                     # candidates: the samples; 0 and 2 are the same partition
    assert isinstance(est, query.PointEstimate)
    assert est.losses.dtype == np.int64 and est.losses[0] == est.losses[2]
    assert est.index == 0                             # the lowest index among equal losses
    assert est.labels.tolist() == [0, 0, 1, 1, 2]     # numbered in the order of first row
    assert est.confidence.dtype == np.float64 and est.confidence.shape == (5,)
    assert ((est.confidence > 0) & (est.confidence <= 1)).all()
    w, size = query.partition_sums(A, A[:1])
    assert np.array_equal(est.confidence, w[0] / (4. * size[0]))
    assert est.confidence[4] == 1.0                   # a singleton is always with itself
    tied = query.point_estimate(A, "vi", candidates=[A[3], A[1], A[3]])
    assert tied.losses[0] == tied.losses[2]
    assert tied.index == int(np.argmin(tied.losses)) and tied.index != 2
    # labels that only a candidate holds, given in any order
    est2 = query.point_estimate(A, candidates=[[5, 5, -2, -2, -2]])
    assert est2.index == 0 and est2.labels.tolist() == [0, 0, 1, 1, 1]


def test_value_errors():
    A = [[0, 1, 1], [0, 0, 1]]
    with pytest.raises(ValueError, match="loss"):
        query.point_estimate(A, loss="ari")
    with pytest.raises(ValueError, match="empty assignments"):
        query.point_estimate([])
    with pytest.raises(ValueError, match="same size"):
        query.partition_loss([[0, 1], [0, 1, 2]], [[0, 1]])
    with pytest.raises(ValueError, match="empty candidates"):
        query.partition_loss(A, np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="size of the assignment"):
        query.partition_sums(A, [[0, 1]])
    with pytest.raises(ValueError, match="integer labels"):
        query.partition_loss(A, [[0., 1., 1.]])


def test_symbols_are_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L._SIGS and name in common_amd.EXPORTS
        assert re.search(r" T %s$" % name, out, re.M)
    assert L.ABI_VERSION == 1 and "#define MSC_ABI_VERSION 1" in text
    for name in ("partition_sums", "partition_loss", "point_estimate", "PointEstimate"):
        assert hasattr(common_amd.query, name)
    for name in ("partition_sums", "partition_loss"):
        assert callable(getattr(common_amd.ZMatrix, name))
    assert common_amd.point_estimate is query.point_estimate
