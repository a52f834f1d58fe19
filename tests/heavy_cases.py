"""The heavy rungs: one group's sufficient statistics at the sizes a CRP produces (one group holding most of 1e7 - 1e8
rows next to singletons and empty slots), and the row values scored against them.  Shared by the fixture's generator
(tests/golden/make_heavy_golden.py, mpmath at 60 digits) and by the tests that read the fixture
(tests/test_heavy_cpu.py, tests/test_gpu_heavy.py): everything here is exact float32 / uint32, numpy only.

A rung is (count, variant): COUNTS x (balanced, lopsided), rung index 2 * (index of the count) + variant.  niw stops at
1e7 (its float32 sum_xxT no longer resolves the scatter beyond)."""
import json
import os

import numpy as np

from oracle import oracle as orc
from tests.gpu_helpers import distinct_hp

COUNTS = [0, 1, 2, 37, 10 ** 3, 10 ** 5, 10 ** 7, 10 ** 8]
# name -> (family, dim)
FAMILIES = {"bb": (orc.BB, 0), "bbnc": (orc.BBNC, 0), "gp": (orc.GP, 0), "bnb": (orc.BNB, 0), "dd": (orc.DD, 7),
            "dm": (orc.DM, 4), "nich": (orc.NICH, 0), "niw3": (orc.NIW, 3), "niw20": (orc.NIW, 20)}
MIXED = ["bb", "gp", "bnb", "dd", "dm", "nich"]
COUNT_VALUES = [0, 1, 2, 5, 31, 32, 40, 1000, 1023, 1024, 3000, 65535]
DM_VALUES = [(0, 0, 0, 0), (0, 1, 0, 0), (9, 6, 3, 2), (1000, 20, 2, 1), (512, 256, 255, 1), (65000, 4000, 900, 100)]
NICH_VALUES = [-1000.5, -3.0, 0.0, 0.75, 2.25, 1e3, 3e7]
NIW_SDS = [0.0, 0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 10.0]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heavy.json")


def counts_of(name):
    return COUNTS[:-1] if name.startswith("niw") else COUNTS


def rung_counts(name):
    """the group size of every rung of the family"""
    return np.repeat(np.asarray(counts_of(name), dtype=np.int64), 2)


def hp_of(name):
    fam, dim = FAMILIES[name]
    return distinct_hp(fam, dim)


def hp_block(name):
    """the float32 block the device is given"""
    fam, dim = FAMILIES[name]
    return orc.pack_hp(fam, hp_of(name), dim)


def _niw_moments(dim):
    """(m, Sigma) of the niw rungs in double: m = the prior's mu + 3, Sigma = its dense psi"""
    hp = distinct_hp(orc.NIW, dim)
    return np.asarray(hp["mu"], dtype=np.float64) + 3.0, np.asarray(hp["psi"], dtype=np.float64)


def rungs(name):
    """-> float-state record array [number of rungs] (oracle.ss_dtype(.., "f32"): the field names of common_amd.ss_dtype)"""
    fam, dim = FAMILIES[name]
    cs = counts_of(name)
    ss = np.zeros(2 * len(cs), dtype=orc.ss_dtype(fam, dim, "f32"))
    for ci, n in enumerate(cs):
        for lop in (0, 1):
            g = ss[2 * ci + lop]
            if fam in (orc.BB, orc.BBNC):
                g["heads"] = min(n, 1) if lop else n // 2
                g["tails"] = n - int(g["heads"])
                if fam == orc.BBNC:
                    g["p"] = 2.0 ** -20 if lop else 0.5
            elif fam == orc.GP:
                g["count"], g["sum"], g["log_prod"] = n, (40 if lop else 3) * n, np.float32(1.5 * n)
            elif fam == orc.BNB:
                g["count"], g["sum"] = n, (n // 8 if lop else 6 * n)
            elif fam == orc.DD:
                c = np.zeros(dim, dtype=np.int64)
                if not lop:
                    c[:] = n // dim
                    c[:n % dim] += 1
                elif n < 7:
                    c[2] = n
                else:                                   # all but six rows in category 2, category 5 empty
                    c[:] = [2, 1, n - 6, 1, 1, 0, 1]
                assert c.sum() == n
                g["count_sum"], g["counts"] = n, c
            elif fam == orc.DM:
                c1 = (3 * n) // 5
                g["counts"] = [20 * n - c1, c1, 0, 0] if lop else [5 * n] * 4
                g["ratio"] = np.float32(-0.25 * n)
            elif fam == orc.NICH:
                g["count"] = n
                g["mean"] = np.float32(-1000.5 if lop else 0.75)
                g["count_times_variance"] = np.float32((1e-4 if lop else 2.25) * n)
            elif fam == orc.NIW:
                # (one variant only: the issue fixes the moments; the lopsided rung halves the scatter about the same mean)
                m, S = _niw_moments(dim)
                if lop:
                    S = 0.5 * S
                g["count"] = n
                g["sum_x"] = (n * m).astype(np.float32)
                g["sum_xxT"] = (n * (S + np.outer(m, m))).astype(np.float32)
    return ss


def values(name):
    """-> the row values of the family, as the column's numpy array [number of values(, dim)]"""
    fam, dim = FAMILIES[name]
    if fam in (orc.BB, orc.BBNC):
        return np.array([False, True])
    if fam in (orc.GP, orc.BNB):
        return np.array(COUNT_VALUES, dtype=np.uint32)
    if fam == orc.DD:
        return np.arange(dim, dtype=np.int32)
    if fam == orc.DM:
        return np.array(DM_VALUES, dtype=np.int32)
    if fam == orc.NICH:
        return np.array(NICH_VALUES, dtype=np.float32)
    m, S = _niw_moments(dim)
    L = np.linalg.cholesky(S)
    out = []
    for j, t in enumerate(NIW_SDS):                     # m itself, then t standard deviations out along a direction of its own
        u = np.cos(1.0 + 0.7 * j + 1.3 * np.arange(dim))
        out.append(m + t * (L @ (u / np.linalg.norm(u))))
    return np.array(out).astype(np.float32)


def np_dtype(name):
    fam, dim = FAMILIES[name]
    return {orc.BB: np.bool_, orc.BBNC: np.bool_, orc.GP: np.uint32, orc.BNB: np.uint32, orc.DD: np.int32,
            orc.DM: np.dtype((np.int32, (dim,))), orc.NICH: np.float32, orc.NIW: np.dtype((np.float32, (dim,)))}[fam]


def load_fixture():
    """-> {name: dict(score_value [R, V], loo [R, V] (NaN where the removal is infeasible), loo_ok [R, V] bool,
    score_data [R])} in float64"""
    with open(FIXTURE) as fh:
        raw = json.load(fh)
    out = {}
    for name, d in raw["families"].items():
        ok = np.array(d["loo_ok"], dtype=bool)
        loo = np.array([[np.nan if x is None else x for x in row] for row in d["loo"]], dtype=np.float64)
        assert np.array_equal(ok, ~np.isnan(loo))
        out[name] = dict(score_value=np.array(d["score_value"], dtype=np.float64), loo=loo, loo_ok=ok,
                         score_data=np.array(d["score_data"], dtype=np.float64))
    return out
