"""Single linkage of a z-matrix, host side: common_amd/csrc/linkage_host.hpp built with the host compiler -- Prim's chain
in every (threads, columns a thread) shape the kernel is instantiated at, then the stable sort, the union-find
relabelling and the leaf walk -- against scipy's linkage and leaves_list, exactly; common_amd.query's new functions on
numpy input; the entry point in the header, the binding and the built library.  No device needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.cluster.hierarchy as hier

import common_amd
from common_amd import _lib as L
from common_amd import query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [2, 3, 17, 64, 65, 257, 600]
# what kernels_linkage.hip launches (linkage::shape_for): one column a thread in 1 .. 16 waves, then 1024 threads
SHAPES = [(64 * w, 1) for w in range(1, 17)] + [(1024, c) for c in (2, 4, 8, 16, 32, 64)]


def _build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "linkage_host.cpp"), "-o", out] + extra)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(_build(tmp_path_factory.mktemp("linkage"), "linkage_host.so", ["-shared", "-fPIC"]))
    lib.linkage_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.linkage_shape.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return lib


def walk(lk):
    """leaves_list restated (pre-order from the last node, column 0 first): scipy's own refuses a linkage with a negative
    distance, which a matrix with entries above 1 has"""
    n = lk.shape[0] + 1
    out, stack = [], [2 * n - 2]
    while stack:
        v = stack.pop()
        if v < n:
            out.append(v)
        else:
            stack += [int(lk[v - n, 1]), int(lk[v - n, 0])]
    return np.array(out)


def scipy_of(z):
    n = z.shape[0]
    lk = hier.linkage(1. - np.array(z[np.triu_indices(n, k=1)]))
    if (lk[:, 2] < 0).any():
        return lk, walk(lk)
    order = hier.leaves_list(lk)
    assert np.array_equal(order, walk(lk))
    return lk, order


def host_of(lib, z, threads, cols, ld=None):
    n = z.shape[0]
    ld = n if ld is None else ld
    buf = np.full((n, ld), np.nan, dtype=np.float32)      # (the padding is never read)
    buf[:, :n] = z
    lk = np.empty((n - 1, 4), dtype=np.float64)
    order = np.empty(n, dtype=np.uint32)
    assert lib.linkage_host(buf.ctypes.data, ld, n, threads, cols, lk.ctypes.data, order.ctypes.data) == 0
    return lk, order


def check_every_shape(lib, z):
    z = np.ascontiguousarray(z, dtype=np.float32)
    n = z.shape[0]
    assert np.array_equal(z, z.T)
    want_lk, want_order = scipy_of(z)
    for threads, cols in [(0, 0)] + [s for s in SHAPES if s[0] * s[1] >= n]:
        lk, order = host_of(lib, z, threads, cols, ld=n + (threads // 64) % 3)
        assert np.array_equal(lk, want_lk), (n, threads, cols)
        assert np.array_equal(order, want_order), (n, threads, cols)


def zmatrix_of(rng, n, S, K):
    return query.zmatrix([rng.integers(0, K, n) for _ in range(S)])


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("n", NS)
def test_z_matrices_in_every_shape(host, n, S):
    rng = np.random.default_rng(100 * n + S)
    check_every_shape(host, zmatrix_of(rng, n, S, 4))


@pytest.mark.parametrize("n", NS)
def test_one_label_and_n_labels(host, n):
    check_every_shape(host, query.zmatrix([np.zeros(n, dtype=np.int64)]))       # every distance 0
    check_every_shape(host, query.zmatrix([np.arange(n)]))                      # every distance 1


@pytest.mark.parametrize("n", NS)
def test_real_valued_without_ties_and_values_above_one(host, n):
    rng = np.random.default_rng(n)
    v = rng.permutation(n * n).astype(np.float32).reshape(n, n) / np.float32(n * n)     # distinct, exact in float32
    z = np.triu(v, 1) + np.triu(v, 1).T + np.eye(n, dtype=np.float32)
    assert np.unique(z[np.triu_indices(n, 1)]).size == n * (n - 1) // 2
    check_every_shape(host, z)
    big = zmatrix_of(rng, n, 3, 3) * np.float32(4.0) - np.float32(0.5)          # up to 3.5: negative distances, with ties
    assert big.max() > 1.0
    check_every_shape(host, big)


def test_the_launchers_shapes_are_the_ones_tested(host):
    seen = set()
    for n in list(range(2, 1100)) + [2048, 2049, 4096, 4097, 8193, 16385, 32768, 32769, 65536]:
        t, c = C.c_uint32(), C.c_uint32()
        host.linkage_shape(n, C.byref(t), C.byref(c))
        assert t.value * c.value >= n and (t.value - 64) * c.value < n or c.value > 1
        seen.add((t.value, c.value))
    assert seen == set(SHAPES)
    for n in (0, 1, 65537):
        host.linkage_shape(n, C.byref(t), C.byref(c))
        assert t.value == 0
    assert L.LINKAGE_MAX_N == 65536


def test_stand_alone_program(tmp_path):
    exe = _build(tmp_path, "linkage_host", ["-DLINKAGE_HOST_MAIN"])
    out = subprocess.check_output([exe]).decode()
    assert "linkage_host ok" in out


def test_query_linkage_on_numpy_input_is_scipys():
    rng = np.random.default_rng(9)
    for n, S in [(2, 1), (12, 5), (40, 3)]:
        z = zmatrix_of(rng, n, S, 3)
        want, order = scipy_of(z)
        got = query.zmatrix_linkage(z)
        assert got.dtype == np.float64 and got.shape == (n - 1, 4) and np.array_equal(got, want)
        assert np.array_equal(query.zmatrix_heuristic_block_ordering(z), order)


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


def test_clusters_equal_fcluster_as_a_partition():
    rng = np.random.default_rng(4)
    S = 4
    z = zmatrix_of(rng, 60, S, 3)
    lk = hier.linkage(1. - z[np.triu_indices(60, 1)])
    # on the matrix's values (multiples of 1 / 4), between them, and outside [0, 1]
    for thr in [0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.3, 0.6, 0.9, -0.5, 1.5]:
        got = query.zmatrix_clusters(z, thr)
        assert got.shape == (60,) and np.issubdtype(got.dtype, np.integer)
        assert same_partition(got, hier.fcluster(lk, 1. - thr, criterion="distance")), thr
        # labels in the order of their first row
        firsts = [int(np.flatnonzero(got == k)[0]) for k in range(got.max() + 1)]
        assert got[0] == 0 and firsts == sorted(firsts)
        # the definition: chains of pairs with 1 - Z <= 1 - threshold
        adj = (1. - z.astype(np.float64)) <= 1. - thr
        reach = adj | np.eye(60, dtype=bool)
        for _ in range(7):
            reach = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        assert np.array_equal(got[:, None] == got[None, :], reach), thr
    assert query.zmatrix_clusters(z, 1.5).max() == 59 and query.zmatrix_clusters(z, -0.5).max() == 0


def test_value_errors():
    for fn in (query.zmatrix_linkage, query.zmatrix_heuristic_block_ordering):
        with pytest.raises(ValueError, match="not a zmat"):
            fn(np.zeros((2, 3), dtype=np.float32))
        with pytest.raises(ValueError):
            fn(np.ones((1, 1), dtype=np.float32))          # n < 2: scipy refuses an empty distance vector
    with pytest.raises(ValueError, match="not a zmat"):
        query.zmatrix_clusters(np.zeros(4, dtype=np.float32), 0.5)
    z = np.ones((3, 3), dtype=np.float32)
    z[0, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        query.zmatrix_linkage(z)


def test_symbol_is_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "microscopes_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(msc_\w+)\(", text, re.M))
    assert "msc_linkage_single" in declared
    assert "msc_linkage_single" in L._SIGS and "msc_linkage_single" in common_amd.EXPORTS
    assert L.ABI_VERSION == 1 and "#define MSC_ABI_VERSION 1" in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", common_amd.LIB_PATH]).decode()
    assert re.search(r" T msc_linkage_single$", out, re.M)
    for name in ("zmatrix_linkage", "zmatrix_clusters", "zmatrix_heuristic_block_ordering"):
        assert callable(getattr(common_amd.query, name))
    for name in ("linkage", "block_ordering"):
        assert callable(getattr(common_amd.ZMatrix, name))
    assert callable(common_amd.Context.linkage_single)
