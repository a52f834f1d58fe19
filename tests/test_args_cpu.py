"""common_amd/_args.py, the one place the binding checks a caller's tensor or row range before the library sees it, driven
directly with CPU tensors (a tensor on the meta device stands in for "some other device"); and a scan of runtime.py and
chains.py for a caller's tensor that reaches ctypes any other way.  No library, no device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from common_amd import _args as A

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 3, 4


def refused(fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)


def test_flat():
    t = torch.zeros(6, dtype=torch.int32)
    for ok in (t, torch.zeros(9, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32)):
        p = A.flat(ok, torch.int32, 6, CPU, "z")
        assert isinstance(p, C.c_void_p) and p.value == ok.data_ptr()
    A.flat(torch.zeros(0, dtype=torch.int32), torch.int32, 0, CPU, "z")          # nothing needed, nothing there
    for bad in (np.zeros(6, np.int32), t.to(torch.int64), t.to(torch.float32), torch.zeros(12, dtype=torch.int32)[::2],
                torch.zeros(5, dtype=torch.int32), torch.zeros(6, dtype=torch.int32, device="meta"), None, [0] * 6):
        refused(A.flat, bad, torch.int32, 6, CPU, "z")
        if bad is not None:
            refused(A.flat, bad, torch.int32, 6, CPU, "z", True)
    assert A.flat(None, torch.int32, 6, CPU, "z", True) is None
    assert A.flat(t, torch.int32, 6, CPU, "z", True).value == t.data_ptr()


def test_flat_dtype_classes():
    u32 = getattr(torch, "uint32", torch.int32)
    for dtype in ((torch.int32, u32), 4):                                       # `order`; `top_slot`
        for ok in (torch.int32, u32):
            assert A.flat(torch.zeros(4, dtype=ok), dtype, 4, CPU, "t").value
        for bad in (torch.int64, torch.float32):
            refused(A.flat, torch.zeros(4, dtype=bad), dtype, 4, CPU, "t")
    assert A.flat(torch.zeros(5, dtype=torch.int64), 8, 5, CPU, "counters").value   # `counters`
    for bad in (torch.int32, torch.float64):
        refused(A.flat, torch.zeros(5, dtype=bad), 8, 5, CPU, "counters")
    for ok in (torch.uint8, torch.bool):                                        # a mask
        assert A.flat(torch.zeros(4, dtype=ok), (torch.uint8, torch.bool), 4, CPU, "mask").value
    refused(A.flat, torch.zeros(4, dtype=torch.int8), (torch.uint8, torch.bool), 4, CPU, "mask")


def test_matrix():
    full = torch.zeros((N, K), dtype=torch.float32)
    padded = torch.zeros((N, K + 3), dtype=torch.float32)[:, :K]
    line = torch.zeros(N * K, dtype=torch.float32)
    assert not padded.is_contiguous()
    for ok, ld in ((full, K), (padded, K + 3), (line, K), (torch.zeros((N + 2, K + 1), dtype=torch.float32), K + 1)):
        p, got = A.matrix(ok, torch.float32, N, K, CPU, "out")
        assert p.value == ok.data_ptr() and got == ld and type(got) is int
        assert ok.dim() == 1 or got == ok.stride(0)                             # the tensor's own row stride
    for bad in (torch.zeros((N, K - 1), dtype=torch.float32), torch.zeros(N, dtype=torch.float32),
                torch.zeros(N * K - 1, dtype=torch.float32), torch.zeros((N - 1, K), dtype=torch.float32),
                torch.zeros((K, N), dtype=torch.float32).T, torch.zeros((N, K), dtype=torch.float32, device="meta"),
                torch.zeros(2 * N * K, dtype=torch.float32)[::2], full.double(), full.numpy(), None,
                torch.zeros((1, N, K), dtype=torch.float32), torch.zeros((N, 1), dtype=torch.float32).expand(N, K)):
        refused(A.matrix, bad, torch.float32, N, K, CPU, "out")
    A.matrix(torch.zeros((0, K), dtype=torch.float32), torch.float32, 0, K, CPU, "out")   # no rows asked for


def test_vectors():
    m = 5
    one = torch.zeros(m, dtype=torch.int32)
    many = torch.zeros((3, m), dtype=torch.int32)
    padded = torch.zeros((3, m + 2), dtype=torch.int32)[:, :m]
    single = torch.zeros((1, m), dtype=torch.int32)
    for given in (None, m):                                                     # Context's partitions; ZMatrix's vectors
        for t, count, ld in ((one, 1, m), (many, 3, m), (padded, 3, m + 2), (single, 1, m)):
            got, c, l = A.vectors(t, CPU, "z", given)
            assert got is t and (c, l) == (count, ld)
        for bad in (many.to(torch.int64), many.to(torch.float32), many.numpy(), None, many.to("meta"), many.T,
                    torch.zeros((3, 2 * m), dtype=torch.int32)[:, ::2], torch.zeros(2 * m, dtype=torch.int32)[::2],
                    many.reshape(1, 3, m), many.expand(2, 3, m), torch.zeros((3, 1), dtype=torch.int32).expand(3, m),
                    torch.zeros(m * 4, dtype=torch.int32).as_strided((3, m), (m - 1, 1))):
            refused(A.vectors, bad, CPU, "z", given)
    # a fixed m: exactly m labels a vector, and no vectors at all is a valid (empty) set
    for bad in (torch.zeros(m + 1, dtype=torch.int32), torch.zeros((2, m - 1), dtype=torch.int32)):
        refused(A.vectors, bad, CPU, "z", m)
    none = many[:0]
    assert A.vectors(none, CPU, "z", m)[1:] == (0, m)
    # m left to the tensor: neither count nor m may be 0
    for bad in (none, many[:, :0], torch.zeros(0, dtype=torch.int32)):
        refused(A.vectors, bad, CPU, "a")
    assert A.vectors(torch.zeros((2, 7), dtype=torch.int32), CPU, "a")[1:] == (2, 7)


def test_rows():
    assert A.rows(10, 0, None) == (0, 10)
    assert A.rows(10, 4, None) == (4, 6)
    assert A.rows(10, 10, None) == (10, 0)
    for bad in ((10, 11, None), (10, -1, 2), (10, 0, -1), (10, -1, None)):
        refused(A.rows, *bad)
    assert A.rows(10, 5, 10) == (5, 10)                  # past the end: the library's to refuse
    got = A.rows(np.uint64(10), np.int64(2), np.int32(3))
    assert got == (2, 3) and all(type(v) is int for v in got)
    assert all(type(v) is int for v in A.rows(10, 4, None))


def test_no_caller_tensor_reaches_ctypes_unchecked():
    """in runtime.py and chains.py .data_ptr() is applied only to tensors the binding made itself: every parameter of a
    public method goes through common_amd/_args.py"""
    own = {"runtime.py": ["sp = (C.c_void_p * len(grids))(*[t.data_ptr() for t in scores])"],     # hp_gibbs's own scores
           "chains.py": ["zp = self.z.data_ptr() + 4 * row0"]}                                    # the ensemble's own z
    for name, allowed in own.items():
        src = open(os.path.join(ROOT, "common_amd", name)).read()
        uses = [ln.strip() for ln in src.splitlines() if ".data_ptr()" in ln]
        assert [u.split("  ")[0] for u in uses] == allowed, uses
        # the spellings of the former call sites, and the checks that went with them
        for pat in (r"\b(z|out|order|trace|top_slot|counters|slots|scores|off|log|proposed|m|c|t)\.data_ptr\(\)",
                    r"\.is_contiguous\(\)", r"c_void_p\(\w+\.data_ptr\(\)\)"):
            hits = [ln.strip() for ln in src.splitlines() if re.search(pat, ln) and ln.strip().split("  ")[0] not in allowed]
            assert not hits, (name, pat, hits)
