"""common_amd.query on numpy input (groups, zmatrix, zmatrix_reorder, the heuristic block ordering) against hand-worked
cases and an independent pair loop, every ValueError of the reference module, and the msc_zmatrix_* entries in the
header and the binding.  No device needed."""
import os
import re

import numpy as np
import pytest

import common_amd
from common_amd import _lib as L
from common_amd import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("msc_zmatrix_create", "msc_zmatrix_add", "msc_zmatrix_nsamples", "msc_zmatrix_counts",
               "msc_zmatrix_result", "msc_zmatrix_reset", "msc_zmatrix_destroy")


def pair_loop_counts(assignments):
    """C[i, j] = samples in which rows i and j carry the same label, one pair at a time"""
    n = len(assignments[0])
    c = np.zeros((n, n), dtype=np.int64)
    for a in assignments:
        for i in range(n):
            for j in range(n):
                c[i, j] += a[i] == a[j]
    return c


def test_groups_hand_worked():
    assert query.groups([2, 0, 2, 5, 0, 2]) == [[0, 2, 5], [1, 4], [3]]
    assert query.groups([2, 0, 2, 5, 0, 2], sort=True) == [[0, 2, 5], [1, 4], [3]]
    assert query.groups([7, 1, 1, 3, 3, 3]) == [[0], [1, 2], [3, 4, 5]]
    assert query.groups([7, 1, 1, 3, 3, 3], sort=True) == [[3, 4, 5], [1, 2], [0]]
    # ties keep the order of first appearance
    assert query.groups(np.array([4, 9, 9, 4, 1]), sort=True) == [[0, 3], [1, 2], [4]]
    assert query.groups([]) == []
    assert all(isinstance(i, int) for g in query.groups(np.array([3, 3, 1], dtype=np.int32)) for i in g)


def test_groups_matches_a_dict_walk():
    rng = np.random.default_rng(5)
    for _ in range(30):
        a = rng.integers(-4, 6, rng.integers(1, 50))
        want = {}
        for i, g in enumerate(a.tolist()):
            want.setdefault(g, []).append(i)
        assert query.groups(a) == list(want.values())
        assert query.groups(a, sort=True) == sorted(want.values(), key=len, reverse=True)


def test_zmatrix_hand_worked():
    z = query.zmatrix([[0, 0, 1], [0, 1, 1]])
    want = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.5], [0.0, 0.5, 1.0]], dtype=np.float32)
    assert z.dtype == np.float32 and np.array_equal(z, want)
    z3 = query.zmatrix([[5, 5], [5, 6], [0, 1]])
    assert np.array_equal(z3, np.array([[1, 1 / 3], [1 / 3, 1]], dtype=np.float32))


@pytest.mark.parametrize("seed", range(6))
def test_zmatrix_against_pair_loop(seed):
    rng = np.random.default_rng(seed)
    n, S = int(rng.integers(1, 30)), int(rng.integers(1, 12))
    A = [rng.integers(-2, int(rng.integers(1, 8)), n) for _ in range(S)]
    got = query.zmatrix(A)
    want = pair_loop_counts(A).astype(np.float32) / np.float32(S)
    assert got.dtype == np.float32 and got.shape == (n, n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(query.zmatrix(np.array(A)), got)     # an [S, n] array is a list of vectors too
    assert np.all(np.diag(got) == 1.0) and np.array_equal(got, got.T)


def test_zmatrix_equals_float32_sum_of_ones():
    # the reference adds ones in float32 and divides by float(S): bit-equal to float32(count) / float32(S) below 2^24
    rng = np.random.default_rng(11)
    A = [rng.integers(0, 3, 9) for _ in range(7)]
    acc = np.zeros((9, 9), dtype=np.float32)
    for a in A:
        acc += (a[:, None] == a[None, :]).astype(np.float32)
    acc /= float(len(A))
    assert np.array_equal(query.zmatrix(A).view(np.uint32), acc.view(np.uint32))


def test_zmatrix_value_errors():
    with pytest.raises(ValueError, match="empty"):
        query.zmatrix([])
    with pytest.raises(ValueError, match="same size"):
        query.zmatrix([[0, 1], [0, 1, 2]])


def test_zmatrix_reorder():
    z = np.arange(16, dtype=np.float32).reshape(4, 4)
    order = np.array([2, 0, 3, 1])
    got = query.zmatrix_reorder(z, order)
    for a in range(4):
        for b in range(4):
            assert got[a, b] == z[order[a], order[b]]
    assert np.array_equal(query.zmatrix_reorder(z, [0, 1, 2, 3]), z)
    with pytest.raises(ValueError, match="not a zmatrix"):
        query.zmatrix_reorder(np.zeros((3, 4)), [0, 1, 2])
    with pytest.raises(ValueError, match="not a zmatrix"):
        query.zmatrix_reorder(np.zeros(4), [0, 1, 2, 3])
    for bad in ([0, 1, 1, 2], [0, 1, 2], [[0, 1], [2, 3]], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="not a valid permutation"):
            query.zmatrix_reorder(z, bad)


def test_heuristic_block_ordering_groups_blocks():
    # two blocks interleaved: the ordering puts each block's rows next to each other
    a = np.array([0, 1, 0, 1, 0, 1, 2, 2])
    z = query.zmatrix([a, a, a])
    order = query.zmatrix_heuristic_block_ordering(z)
    assert sorted(order.tolist()) == list(range(8))
    labels = a[order]
    assert sum(labels[i] != labels[i + 1] for i in range(7)) == 2
    block = query.zmatrix_reorder(z, order)
    assert np.array_equal(block, np.kron(np.eye(3), np.ones((1, 1)))[labels][:, labels].astype(np.float32))
    with pytest.raises(ValueError, match="not a zmat"):
        query.zmatrix_heuristic_block_ordering(np.zeros((2, 3)))


def test_heuristic_block_ordering_is_single_linkage_of_the_condensed_distances():
    import scipy.cluster.hierarchy as hier
    rng = np.random.default_rng(3)
    z = query.zmatrix([rng.integers(0, 3, 12) for _ in range(5)])
    iu = np.triu_indices(12, k=1)
    want = hier.leaves_list(hier.linkage(1.0 - z[iu], method="single"))
    assert np.array_equal(query.zmatrix_heuristic_block_ordering(z), want)


def test_new_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in common_amd.EXPORTS
        assert name in L._SIGS
    assert "typedef struct msc_zmatrix msc_zmatrix;" in text
    assert L.ABI_VERSION == 1


def test_package_exports():
    assert common_amd.ZMatrix is common_amd.runtime.ZMatrix
    assert common_amd.query is query
    for name in ("groups", "zmatrix", "zmatrix_reorder", "zmatrix_heuristic_block_ordering"):
        assert callable(getattr(query, name))
