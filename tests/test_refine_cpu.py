"""Greedy refinement of point-estimate partitions, host side: common_amd.query.refine_partition on numpy input (the
yardstick of msc_zmatrix_partition_refine) over all 203 partitions of six rows -- the running binder_num against
partition_loss, strict decrease exactly when a row moved, local optimality by brute force, a second refinement that moves
nothing, the numbering -- the tie rule, the id capacity and zero sweeps, a visiting order that changes the trajectory,
point_estimate's refine argument, and the entry point in the header, the binding and the built library.  No device needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import common_amd
from common_amd import _lib as L
from common_amd import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def numbered_by_first_row(labels):
    seen = []
    for v in labels:
        if v not in seen:
            seen.append(v)
    return seen == list(range(len(seen)))


def single_moves(labels):
    """every partition one row move away: the row into each other cluster, and alone"""
    labels = np.asarray(labels)
    out = []
    for a in range(labels.size):
        for k in list(np.unique(labels)) + [labels.max() + 1]:
            if k != labels[a]:
                c = labels.copy()
                c[a] = k
                out.append(c)
    return np.array(out)


def is_local_optimum(A, labels):
    here = int(query.partition_loss(A, labels)[0][0])
    return int(query.partition_loss(A, single_moves(labels))[0].min()) >= here


SIX = np.array([[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 2], [0, 1, 0, 1, 2, 2], [0, 0, 0, 0, 1, 1],
                [2, 2, 2, 0, 0, 1], [0, 0, 1, 2, 2, 2], [1, 0, 0, 2, 2, 2], [0, 0, 0, 1, 0, 1]])   # fixed noisy samples


def test_all_partitions_of_six_rows_as_starts():
    parts = set_partitions(6)
    assert parts.shape == (203, 6)
    start_loss = query.partition_loss(SIX, parts)[0]
    r = query.refine_partition(SIX, parts)
    assert isinstance(r, query.RefinedPartitions) and r.valid == len(SIX)
    assert r.labels.shape == (203, 6) and r.labels.dtype == np.int32
    assert r.binder_num.dtype == np.int64 and r.moves.dtype == np.int64
    assert np.array_equal(r.binder_num, query.partition_loss(SIX, r.labels)[0])
    assert (r.binder_num <= start_loss).all()
    assert np.array_equal(start_loss - r.binder_num > 0, r.moves > 0)
    assert (r.moves > 0).any() and (r.moves == 0).any() and (r.sweeps >= 1).all() and (r.sweeps < 20).all()
    for k in range(203):
        assert is_local_optimum(SIX, r.labels[k]), parts[k]
        assert numbered_by_first_row(r.labels[k].tolist())
    again = query.refine_partition(SIX, r.labels)
    assert (again.moves == 0).all() and (again.sweeps == 1).all()
    assert np.array_equal(again.labels, r.labels) and np.array_equal(again.binder_num, r.binder_num)


def test_ties_keep_a_row_where_it_is():
    A = [[0, 0], [0, 1]]                               # together once, apart once: both partitions cost the same
    r = query.refine_partition(A, [[0, 0], [0, 1]])
    assert r.labels.tolist() == [[0, 0], [0, 1]]
    assert r.moves.tolist() == [0, 0] and r.sweeps.tolist() == [1, 1]
    assert r.binder_num[0] == r.binder_num[1] == 1


def test_capacity_and_zero_sweeps():
    A = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 2]])
    one = query.refine_partition(A, [[5, 5, 5, 5]], max_clusters=1)       # no free id: nobody can leave
    assert one.labels.tolist() == [[0, 0, 0, 0]] and one.moves.tolist() == [0] and one.sweeps.tolist() == [1]
    free = query.refine_partition(A, [[5, 5, 5, 5]])
    assert free.labels.tolist() == [[0, 0, 1, 1]] and free.moves[0] > 0
    with pytest.raises(ValueError, match="max_clusters"):
        query.refine_partition(A, [[0, 1, 2, 2]], max_clusters=2)
    with pytest.raises(ValueError, match="max_clusters"):
        query.refine_partition(A, [[0, 0, 0, 0]], max_clusters=5)
    with pytest.raises(ValueError, match="max_clusters"):
        query.refine_partition(A, [[0, 0, 0, 0]], max_clusters=0)
    start = [[7, -3, 7, 9]]
    zero = query.refine_partition(A, start, max_sweeps=0)
    assert zero.labels.tolist() == [[0, 1, 0, 2]] and zero.sweeps.tolist() == [0] and zero.moves.tolist() == [0]
    assert zero.binder_num[0] == query.partition_loss(A, start)[0][0]


def test_visiting_order_changes_the_trajectory():
    # two local optima within reach of one start: which one is reached depends on who is asked first (found by search
    # over random samples of five rows; the two ends cost 16 and 18)
    A = np.array([[1, 1, 0, 1, 1], [1, 2, 1, 1, 2], [2, 2, 2, 2, 2], [1, 2, 2, 2, 1]])
    start = [[1, 0, 0, 1, 2]]
    up = query.refine_partition(A, start)
    down = query.refine_partition(A, start, order=[4, 3, 2, 1, 0])
    assert up.labels.tolist() == [[0, 0, 0, 0, 0]] and down.labels.tolist() == [[0, 1, 1, 1, 0]]
    assert up.binder_num.tolist() == [16] and down.binder_num.tolist() == [18]
    assert not (np.array_equal(up.labels, down.labels) and np.array_equal(up.moves, down.moves))
    for r in (up, down):
        assert is_local_optimum(A, r.labels[0])
        assert r.binder_num[0] == query.partition_loss(A, r.labels)[0][0]
    with pytest.raises(ValueError, match="permutation"):
        query.refine_partition(A, start, order=[0, 1, 2, 2, 3])


def test_symbol_is_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    name = "msc_zmatrix_partition_refine"
    assert name in declared and name in L._SIGS and name in common_amd.EXPORTS
    assert re.search(r" T %s$" % name, out, re.M)
    assert len(L._SIGS[name][1]) == 11
    assert L.ABI_VERSION == 1 and "#define MSC_ABI_VERSION 1" in text
    assert callable(common_amd.ZMatrix.partition_refine)
    assert common_amd.refine_partition is query.refine_partition
    # the caps the header states are the binding's
    assert "m <= %d and max_clusters <= %d" % (L.ZMATRIX_REFINE_MAX_ROWS, L.ZMATRIX_REFINE_MAX_CLUSTERS) in text
    assert L.ZMATRIX_REFINE_MAX_ROWS >= 32768 and L.ZMATRIX_REFINE_MAX_CLUSTERS >= 1024


def test_point_estimate_arguments():
    rng = np.random.default_rng(5)
    truth = rng.integers(0, 3, 40)
    A = np.tile(truth, (12, 1))
    flip = rng.random(A.shape) < 0.3
    A[flip] = rng.integers(0, 5, int(flip.sum()))
    plain = query.point_estimate(A)
    same = query.point_estimate(A, refine=0)
    assert type(same) is type(plain) and same.index == plain.index
    assert np.array_equal(same.labels, plain.labels) and np.array_equal(same.losses, plain.losses)
    assert np.array_equal(same.confidence, plain.confidence)
    # what it returned before the argument existed: Dahl's estimator, the first sample of the lowest loss
    losses = query.partition_loss(A, A)[0]
    assert plain.index == int(np.argmin(losses)) and np.array_equal(plain.losses, losses)
    fine = query.point_estimate(A, refine=5)
    got = int(query.partition_loss(A, fine.labels)[0][0])
    assert got <= losses.min() and got < losses.min()            # (noisy samples: the optimum is none of them)
    assert np.array_equal(fine.losses, losses)
    assert fine.index in np.argsort(losses, kind="stable")[:8].tolist()
    w, size = query.partition_sums(A, fine.labels)
    assert np.array_equal(fine.confidence, w[0] / (12. * size[0]))
    one = query.point_estimate(A, refine=5, starts=1)
    assert one.index == plain.index
    with pytest.raises(ValueError, match="variation-of-information"):
        query.point_estimate(A, loss="vi", refine=1)
    assert query.point_estimate(A, loss="vi", refine=0).index == query.point_estimate(A, loss="vi").index
