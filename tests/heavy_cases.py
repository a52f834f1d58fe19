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
from tests.gpu_helpers import crp_prior_matrix, distinct_hp

COUNTS = [0, 1, 2, 37, 10 ** 3, 10 ** 5, 10 ** 7, 10 ** 8]
# name -> (family, dim)
FAMILIES = {"bb": (orc.BB, 0), "bbnc": (orc.BBNC, 0), "gp": (orc.GP, 0), "bnb": (orc.BNB, 0), "dd": (orc.DD, 7),
            "dm": (orc.DM, 4), "nich": (orc.NICH, 0), "niw3": (orc.NIW, 3), "niw20": (orc.NIW, 20)}
MIXED = ["bb", "gp", "bnb", "dd", "dm", "nich"]
# the families the sequential sweep and the chain ensembles take (route_sequential refuses dm, niw and bbnc): 16 rungs each
SEQUENTIAL = ["bb", "gp", "bnb", "dd", "nich"]
ALPHA32 = np.float32(1.3)                  # the CRP concentration of every heavy state, as the device holds it
# the heavy tests' two layouts of the families with 16 rungs (all but niw): one group per rung, and K = 300 with group k on
# rung k mod 16 -- the group counts score_assignment is kept for in the fixture, key -> (rungs, K)
LAYOUT_KEYS = {"K16": (16, 16), "K300": (16, 300)}
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


def layout_counts(R, K):
    """the group counts of a layout: group k holds the count of rung k mod R"""
    return np.repeat(np.asarray(COUNTS[:R // 2], dtype=np.int64), 2)[np.arange(K) % R]


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


def load_score_assignment():
    """-> {layout key of LAYOUT_KEYS: score_assignment of the layout's group counts at ALPHA32} in float64"""
    with open(FIXTURE) as fh:
        d = json.load(fh)["score_assignment"]
    assert d["alpha"] == float(ALPHA32)
    return {key: float(d[key]) for key in LAYOUT_KEYS}


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


_FX = {}


def fixture():
    if not _FX:
        _FX.update(load_fixture())
    return _FX


def layout(names, K=None):
    """-> (K, rung [K], counts [K]): one group per rung (K None) or group k on rung k mod (number of rungs)"""
    R = len(rungs(names[0]))
    assert all(len(rungs(n)) == R for n in names)
    K = R if K is None else K
    rung = np.arange(K) % R
    return K, rung, rung_counts(names[0])[rung]


class Expect(object):
    """the fixture's expectations for a state of the named families on a heavy layout and n rows, row i holding value
    i mod (number of values) of every family: host side, numpy only.  vmax: the gp / bnb columns take only the
    values up to it (COUNT_VALUES ascends: the first ones)"""

    def __init__(self, names, K=None, n=512, vmax=None):
        fx = fixture()
        self.names, self.n = names, n
        self.K, self.rung, self.counts = layout(names, K)
        R = len(rungs(names[0]))
        nv = {nm: len(values(nm)) for nm in names}
        if vmax is not None:
            nv.update({nm: int((values(nm) <= vmax).sum()) for nm in names if nm in ("gp", "bnb")})
        self.vidx = [np.arange(n) % nv[nm] for nm in names]
        # [n, K] in double: the plain scores, the leave-one-out ones, and where the removal is feasible for every feature
        self.plain = sum(fx[nm]["score_value"][self.rung][:, v].T for nm, v in zip(names, self.vidx))
        self.ok = np.logical_and.reduce([fx[nm]["loo_ok"][self.rung][:, v].T for nm, v in zip(names, self.vidx)])
        self.loo = sum(np.where(self.ok, fx[nm]["loo"][self.rung][:, v].T, 0.0) for nm, v in zip(names, self.vidx))
        self.data = np.array([fx[nm]["score_data"][self.rung] for nm in names])
        # every row in a group it can leave (the groups taken in turn, so every rung loses rows); none: unassigned
        self.z = np.full(n, -1, dtype=np.int32)
        for i in range(n):
            feas = np.nonzero(self.ok[i])[0]
            if len(feas):
                self.z[i] = feas[(i * 7 + i // 16) % len(feas)]
        self.rungs_left = np.unique(self.rung[self.z[self.z >= 0]])
        self.R = R

    def records(self):
        """the rows as a record array, field f<i> holding feature i's column"""
        rec = np.zeros(self.n, dtype=[("f%d" % i, np_dtype(nm)) for i, nm in enumerate(self.names)])
        for i, nm in enumerate(self.names):
            rec["f%d" % i] = values(nm)[self.vidx[i]]
        return rec

    def expected(self, loo=False):
        want = self.plain.copy()
        if loo:
            own = self.z >= 0
            want[own, self.z[own]] = self.loo[own, self.z[own]]
        return want

    def totals(self, loo=False, alpha=1.3):
        """-> (t [n, K], logp [n]): scores + CRP prior, and the row's predictive log-density, in double"""
        from scipy.special import logsumexp
        z = self.z if loo else None
        t = self.expected(loo) + crp_prior_matrix(self.counts, alpha, z)
        n_r = float(self.counts.sum()) - (0.0 if z is None else (z >= 0).astype(np.float64))
        return t, logsumexp(t, axis=1) - np.log(n_r + alpha)
