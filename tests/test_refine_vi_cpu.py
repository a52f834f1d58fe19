"""Greedy refinement under the exact expected variation of information, host side: msc_vi_table (the fixed-point table of
n log2 n that the host path and the kernels share; it needs no device), common_amd.query.refine_partition_vi on numpy
input (the yardstick of msc_partition_refine_vi) over all 203 partitions of six rows -- the integer decrease against the
float64 expected VI, local optimality by brute force -- the id capacity, a visiting order, zero sweeps, wide and negative
labels, vi_estimate's refine argument, and the entry points in the header, the binding and the built library.  No device
needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import common_amd
from common_amd import _lib as L
from common_amd import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = float(1 << 24)


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


def gate(moves, m):
    """what the integer decrease and the float64 expected VI may differ by, in bits: a G is within 1 of its real value, a D
    is made of 3 S of them and a move of two D, over S m 2^24; then the float64 path's own rounding"""
    return moves * 6.0 / (m * SCALE) + 2.0 ** -50 * (m + 16) * math.log2(m + 1)


def single_moves(labels, max_clusters):
    """every partition one row move away: the row into each other cluster, and alone while an id is free"""
    labels = np.asarray(labels)
    out = []
    for a in range(labels.size):
        new = [labels.max() + 1] if np.unique(labels).size < max_clusters else []
        for k in list(np.unique(labels)) + new:
            if k != labels[a]:
                c = labels.copy()
                c[a] = k
                out.append(c)
    return np.array(out).reshape(-1, labels.size)


def test_table():
    m = 32768
    F = query.vi_table(m)
    assert F.dtype == np.int64 and F.shape == (m + 1,)
    n = np.arange(1, m + 1, dtype=np.float64)
    want = np.concatenate(([0.0], np.rint(n * np.log2(n) * SCALE)))
    assert np.abs(F - want.astype(np.int64)).max() <= 1
    assert F[0] == 0 and F[1] == 0 and F[2] == 2 << 24
    G = np.diff(F)
    assert (np.diff(G) >= 0).all() and G[0] == 0
    assert G.max() < 17 << 24
    assert np.array_equal(query.vi_table(5), F[:6]) and query.vi_table(0).tolist() == [0]


SIX = np.array([[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 2], [0, 1, 0, 1, 2, 2], [2, 2, 2, 0, 0, 1]])


def test_all_partitions_of_six_rows_as_starts():
    parts = set_partitions(6)
    S, m = SIX.shape
    assert parts.shape == (203, 6)
    r = query.refine_partition_vi(SIX, parts)
    assert isinstance(r, query.RefinedVI) and r.valid == S
    assert r.labels.shape == (203, 6) and r.labels.dtype == np.int32
    assert r.decrease.dtype == np.int64 and r.moves.dtype == np.int64 and r.vi.dtype == np.float64
    assert np.array_equal(r.vi_start, query.expected_loss(SIX, parts).vi)
    assert np.array_equal(r.vi, query.expected_loss(SIX, r.labels).vi)
    assert (r.decrease >= 0).all() and np.array_equal(r.decrease > 0, r.moves > 0)
    assert (r.moves > 0).any() and (r.moves == 0).any() and (r.sweeps >= 1).all() and (r.sweeps < 20).all()
    for k in range(203):
        off = abs((r.vi_start[k] - r.vi[k]) - r.decrease[k] / (S * m * SCALE))
        assert off <= gate(int(r.moves[k]), m), (parts[k], off)
        assert r.labels[k].tolist() == query._renumber(r.labels[k]).tolist()
    # a result with sweeps < max_sweeps is a local optimum: brute force over all rows x (clusters + 1), once per result
    ends = {}
    for k in range(203):
        ends.setdefault(tuple(r.labels[k].tolist()), []).append(k)
    for labels, ks in ends.items():
        near = single_moves(labels, m)
        best = query.expected_loss(SIX, near).vi.min()
        for k in ks:
            assert r.vi[k] - best <= gate(int(r.moves[k]), m), (labels, parts[k], r.vi[k] - best)
    again = query.refine_partition_vi(SIX, r.labels)
    assert (again.moves == 0).all() and (again.sweeps == 1).all() and (again.decrease == 0).all()
    assert np.array_equal(again.labels, r.labels)


def planted(rng, m, S, k, noise, wide=False):
    truth = rng.integers(0, k, m)
    A = np.tile(truth, (S, 1))
    flip = rng.random(A.shape) < noise
    A[flip] = rng.integers(0, k + 2, int(flip.sum()))
    if wide:
        A = A * 1000003 - 2 ** 31
    return A


def test_capacity_order_and_zero_sweeps():
    rng = np.random.default_rng(11)
    A = planted(rng, 30, 9, 3, 0.25)
    m, S = 30, 9
    one = query.refine_partition_vi(A, [[5] * m], max_clusters=1)          # no free id: nobody can leave
    assert one.labels.tolist() == [[0] * m] and one.moves.tolist() == [0] and one.sweeps.tolist() == [1]
    stripes = (np.arange(m) % 2)[None]
    # rows that are alone in every sample leave for ids of their own while there are any: D_k = S G(n'_k) > 0 everywhere
    A[:, -3:] = 100 + np.arange(3)
    two = query.refine_partition_vi(A, stripes, max_clusters=3)            # binds: one free id for three loners
    loose = query.refine_partition_vi(A, stripes)
    assert two.labels.max() == 2 and loose.labels.max() >= 4 and loose.vi[0] < two.vi[0] <= two.vi_start[0]
    assert len(set(loose.labels[0, -3:].tolist())) == 3 and len(set(two.labels[0, -3:].tolist())) == 1
    for bad in (0, m + 1):
        with pytest.raises(ValueError, match="max_clusters"):
            query.refine_partition_vi(A, stripes, max_clusters=bad)
    with pytest.raises(ValueError, match="max_clusters"):
        query.refine_partition_vi(A, [np.arange(m) % 3], max_clusters=2)
    order = rng.permutation(m)
    up, down = query.refine_partition_vi(A, stripes, max_sweeps=1), query.refine_partition_vi(A, stripes, max_sweeps=1,
                                                                                              order=order)
    assert up.sweeps.tolist() == [1] and down.sweeps.tolist() == [1]
    assert not (np.array_equal(up.labels, down.labels) and np.array_equal(up.decrease, down.decrease))
    for r in (up, down, two, loose):
        assert abs((r.vi_start[0] - r.vi[0]) - r.decrease[0] / (S * m * SCALE)) <= gate(int(r.moves[0]), m)
    with pytest.raises(ValueError, match="permutation"):
        query.refine_partition_vi(A, stripes, order=[0] * m)
    start = [[7, -3, 7, 9] + [9] * (m - 4)]
    zero = query.refine_partition_vi(A, start, max_sweeps=0)
    assert zero.labels[0, :5].tolist() == [0, 1, 0, 2, 2] and zero.sweeps.tolist() == [0] and zero.moves.tolist() == [0]
    assert zero.decrease.tolist() == [0] and zero.vi[0] == zero.vi_start[0] == query.expected_loss(A, start).vi[0]


def test_wide_and_negative_labels_and_default_starts():
    rng = np.random.default_rng(12)
    A = planted(rng, 40, 12, 4, 0.2)
    W = A * 1000003 - 2 ** 31                                              # the same partitions, labels over all of int32
    assert W.min() >= -2 ** 31 and W.max() < 2 ** 31 and W.min() < -2 ** 30
    a, w = query.refine_partition_vi(A), query.refine_partition_vi(W.astype(np.int32))
    for x, y in zip(a[:6], w[:6]):
        assert np.array_equal(x, y)
    assert a.labels.shape == (8, 40)
    # the default starts: the nstarts samples of lowest exact expected VI, ties to the lowest index
    top = np.argsort(query.expected_loss(A).vi, kind="stable")
    assert np.array_equal(a.vi_start, query.expected_loss(A).vi[top[:8]])
    three = query.refine_partition_vi(A, nstarts=3)
    assert np.array_equal(three.labels, a.labels[:3]) and np.array_equal(three.decrease, a.decrease[:3])
    given = query.refine_partition_vi(A, starts=A[top[:3]])
    assert np.array_equal(given.labels, three.labels)
    assert (a.vi <= a.vi_start).all() and a.vi.min() < query.expected_loss(A).vi.min()


def test_vi_estimate_refine_argument():
    rng = np.random.default_rng(5)
    A = planted(rng, 40, 12, 3, 0.3)
    plain = query.vi_estimate(A)
    same = query.vi_estimate(A, refine=0)
    assert type(same) is type(plain) and same.index == plain.index
    assert np.array_equal(same.labels, plain.labels) and np.array_equal(same.losses, plain.losses)
    assert np.array_equal(same.confidence, plain.confidence)
    # what it returned before the argument existed: the first sample of the lowest exact expected VI
    losses = query.expected_loss(A).vi
    assert plain.index == int(np.argmin(losses)) and np.array_equal(plain.losses, losses)
    assert np.array_equal(plain.labels, query._renumber(A[plain.index]))
    fine = query.vi_estimate(A, refine=5)
    got = query.expected_loss(A, fine.labels).vi[0]
    assert got <= losses.min() and got < losses.min()                      # (noisy samples: the optimum is none of them)
    assert np.array_equal(fine.losses, losses)
    assert fine.index in np.argsort(losses, kind="stable")[:8].tolist()
    w, size = query.partition_sums(A, fine.labels)
    assert np.array_equal(fine.confidence, w[0] / (12. * size[0]))
    r = query.refine_partition_vi(A, max_sweeps=5)
    assert np.array_equal(fine.labels, r.labels[int(np.argmin(r.vi))])
    one = query.vi_estimate(A, refine=5, starts=1)
    assert one.index == plain.index
    cands = np.stack([A[3], A[0], np.zeros(40, dtype=A.dtype)])
    c = query.vi_estimate(A, candidates=cands, refine=5)
    assert query.expected_loss(A, c.labels).vi[0] <= query.expected_loss(A, cands).vi.min()
    with pytest.raises(ValueError, match="refine"):
        query.vi_estimate(A, refine=-1)


def test_a_zmatrix_keeps_no_samples():
    class Stub(common_amd.ZMatrix):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(ValueError, match="keeps counts, not samples"):
        query.refine_partition_vi(Stub(), [[0, 0]])


def test_symbols_are_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    for name, nargs in (("msc_vi_table", 2), ("msc_partition_refine_vi", 17)):
        assert name in declared and name in L._SIGS and name in common_amd.EXPORTS
        assert re.search(r" T %s$" % name, out, re.M)
        assert len(L._SIGS[name][1]) == nargs
    assert L.ABI_VERSION == 1 and "#define MSC_ABI_VERSION 1" in text
    assert callable(common_amd.Context.partition_refine_vi)
    assert "m <= %d, nsamples <= %d, max_clusters <= %d" % (L.REFINE_VI_MAX_ROWS, L.REFINE_VI_MAX_SAMPLES,
                                                            L.REFINE_VI_MAX_CLUSTERS) in text
    assert L.VI_TABLE_SCALE == 1 << 24 and "rint(n log2(n) 2^24)" in text
