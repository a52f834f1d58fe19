"""Host side of tests/test_gpu_heavy_chains.py: which row every chain visits on the heavy layouts, the fixture's
expectation of the visit (tests/golden/heavy.json through tests/heavy_cases.py), its dart, the exact tables it leaves, and
the tile plan the ensemble's predictive takes.  numpy, fractions and the host compiler only: tests/test_heavy_chains_cpu.py
runs all of it without a device.

The state: the five families the sequential sweep takes (hc.SEQUENTIAL), one feature each, on the heavy rungs.  NROWS
fixture rows, row i holding value i mod (number of values) of every family (96 = 8 x 12: every pair of a count value and a
categorical / real value occurs), and two rows of this file's own whose nich value sits next to the lopsided rungs' mean
(NEAR_MEAN): row NROWS sits in a lopsided 1e8 group and leaves it, row NROWS + 1 is unassigned and its dart lands it
there.  The fixture holds no score for those two values: their visits are held by the tables they leave, not by scores.

The assignment is hc.Expect's, with one change: on the one-group-a-rung layout its rule leaves two rungs that a row could
leave without one (a row's feasible groups are few there), so a row is moved onto each such rung (Visits._cover)."""
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

from oracle import oracle as orc
from tests import heavy_cases as hc
from tests.gpu_helpers import crp_prior_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")
NAMES = hc.SEQUENTIAL
NROWS, NCHAINS = 96, 128
SEED, SWEEP = 7100, 3
ALPHA = float(hc.ALPHA32)
LAYOUTS = [None, 300]
NEAR_MEAN = np.array([-1000.375, -1000.5625], dtype=np.float32)      # both exact in float32; the lopsided mean is -1000.5
NEAR_ROW = dict(bb=False, gp=40, bnb=0, dd=2)                         # the two rows' other values: what a lopsided rung holds
BETAS = np.array([1.0, 0.5, 0.25, 0.0], dtype=np.float32)
ND = 8                                                                # chains of a tempered call: BETAS twice
EDGE = 1e-5                                                           # _check_agreement's distance of a dart from a CDF step
RUNGS = {nm: hc.rungs(nm) for nm in NAMES}
LOPSIDED_1E8 = 15                                                     # the rung (1e8 rows, lopsided)


# ---- the tile plan of the ensemble's predictive -----------------------------------------------------------------------

_PLAN_EXE = []


def cm_plan(names, K, vmax=None):
    """what route_calls.hpp plan_chains_marginal (host-only code, built here with the host compiler as
    tests/test_route_calls_cpu.py builds its program) plans for a state of the named families whose gp / bnb columns
    hold values up to vmax -> dict(TG, TS, lds_floats, wide, large, staged=[feature -> bool])"""
    if not _PLAN_EXE:
        exe = os.path.join(tempfile.mkdtemp(prefix="cm_plan_"), "chains_marginal_plan_host")
        subprocess.check_call([os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                               os.path.join(ROOT, "tests", "cxx", "chains_marginal_plan_host.cpp"), "-o", exe])
        _PLAN_EXE.append(exe)
    args = [str(int(K))]
    for nm in names:
        fam, dim = hc.FAMILIES[nm]
        vcap = 0
        if nm in ("gp", "bnb"):                       # (abi.cpp: vcap = min(the bound column's maximum + 1, the table's cap))
            top = int(hc.values(nm).max() if vmax is None else hc.values(nm)[hc.values(nm) <= vmax].max())
            vcap = min(top + 1, 1024)
        args += [str(int(fam)), str(int(dim)), str(vcap)]
    lines = subprocess.check_output([_PLAN_EXE[0]] + args, universal_newlines=True).split("\n")
    tg, ts, lds, wide, large = (int(x) for x in lines[0].split())
    staged = [int(ln.split()[1]) >= 0 for ln in lines[1:1 + len(names)]]
    return dict(TG=tg, TS=ts, lds_floats=lds, wide=bool(wide), large=bool(large), staged=staged)


# ---- draws --------------------------------------------------------------------------------------------------------------

def cdf_of(t):
    return np.cumsum(orc.scores_to_probs(t))


def want_draw(t, u):
    """the group a dart u draws from the totals t: test_gpu_heavy._sweep_check's rule"""
    return min(int(np.searchsorted(cdf_of(t), u, side="right")), len(t) - 1)


def near_edge(t, u):
    """does the dart lie within EDGE of a step of the fixture's CDF?"""
    return bool(np.min(np.abs(cdf_of(t) - u)) < EDGE)


def step_proven(t, u, got, want):
    """tests/test_gpu_sweep.py _check_agreement's test of one disagreement: the dart within EDGE of the CDF step between
    the two draws, or less than EDGE of mass between them"""
    p = orc.scores_to_probs(t)
    cdf = np.cumsum(p)
    lo, hi = sorted((int(got), int(want)))
    return bool(abs(cdf[lo] - u) < EDGE or p[lo + 1:hi + 1].sum() < EDGE)


def lse(t):
    m = np.max(t)
    return float(m + np.log(np.sum(np.exp(t - m))))


# ---- the visits -----------------------------------------------------------------------------------------------------------

class Visits(hc.Expect):
    """chain c of NCHAINS visits row row_of[c] = c mod (NROWS + 2) under the key seeds[c] = SEED + c (but the chain of the
    unassigned near-mean row, whose key is searched so that the dart lands in self.lop with a quarter of that group's
    mass to spare on either side)"""

    def __init__(self, K=None):
        hc.Expect.__init__(self, NAMES, K, NROWS)
        n = self.n
        self._cover()
        lops = np.nonzero(self.rung == LOPSIDED_1E8)[0]
        self.lop = int(lops[len(lops) // 2])
        self.nrows = n + 2
        self.zfull = np.concatenate([self.z, [self.lop, -1]]).astype(np.int32)
        self.rec = self.records()
        self.row_of = np.arange(NCHAINS) % self.nrows
        assert set(self.row_of) == set(range(self.nrows))
        self.total = int(self.counts.sum())
        # the fixture rows' expectation after the leave: the features' sum, the log pseudocounts, their total
        self.feat = self.expected(loo=True)
        self.crp = crp_prior_matrix(self.counts, ALPHA, self.z)
        self.t = self.feat + self.crp
        self.n_r = self.total - (self.z >= 0).astype(np.int64)
        self.inc = np.array([lse(self.t[r]) - math.log(float(self.n_r[r]) + ALPHA) for r in range(n)])
        self.seeds = [SEED + c for c in range(NCHAINS)]
        self.t_join = self._near_mean_totals(1)
        self._place_join()
        self.u = np.array([orc.uniform01(self.seeds[c], SWEEP, int(self.row_of[c])) for c in range(NCHAINS)])
        # the tempered calls: call j visits row j in ND chains, chain i at BETAS[i % 4] under the key seeds[j] + 1000 (i // 4)
        self.beta_d = BETAS[np.arange(ND) % len(BETAS)]
        self.keys_d = [[self.seeds[j] + 1000 * (i // len(BETAS)) for i in range(ND)] for j in range(n)]
        self.u_d = np.array([[orc.uniform01(self.keys_d[j][i], SWEEP, j) for i in range(ND)] for j in range(n)])

    def _cover(self):
        """every rung that some row can leave loses a row: a row whose own rung keeps another row moves there"""
        z = self.z
        for r in np.unique(self.rung[np.nonzero(self.ok.any(axis=0))[0]]):
            if r in self.rung[z[z >= 0]]:
                continue
            held = np.bincount(self.rung[z[z >= 0]], minlength=self.R)
            for i, k in zip(*np.nonzero(self.ok & (self.rung == r)[None, :])):
                if z[i] < 0 or held[self.rung[z[i]]] > 1:
                    z[i] = k
                    break
        self.rungs_left = np.unique(self.rung[z[z >= 0]])
        assert np.array_equal(self.rungs_left, np.unique(self.rung[np.nonzero(self.ok.any(axis=0))[0]]))

    def records(self):
        rec = np.zeros(self.nrows, dtype=[("f%d" % i, hc.np_dtype(nm)) for i, nm in enumerate(self.names)])
        for i, nm in enumerate(self.names):
            rec["f%d" % i][:self.n] = hc.values(nm)[self.vidx[i]]
            rec["f%d" % i][self.n:] = NEAR_MEAN if nm == "nich" else NEAR_ROW[nm]
        return rec

    def row_values(self, r):
        """the row's value of every family, as Python numbers (nich: the float32's exact value)"""
        return {nm: (float(self.rec["f%d" % i][r]) if nm == "nich" else int(self.rec["f%d" % i][r]))
                for i, nm in enumerate(self.names)}

    def _near_mean_totals(self, which):
        """totals of near-mean row `which` against the pristine state: the four lookup features from the fixture, nich from
        the oracle's double twin -- no arbiter at these sizes, and none is needed: the totals only place a dart well
        inside a group's share of the CDF, no score is held against them"""
        fx = hc.fixture()
        t = crp_prior_matrix(self.counts, ALPHA)[0].copy()
        for nm in ("bb", "gp", "bnb", "dd"):
            j = int(np.nonzero(hc.values(nm) == NEAR_ROW[nm])[0][0])
            t += fx[nm]["score_value"][self.rung, j]
        F = orc.Family(orc.NICH, hc.hp_of("nich"), 0, "f64")
        t += F.score_matrix(orc.widen_ss(orc.NICH, RUNGS["nich"], 0), NEAR_MEAN[which:which + 1])[0][self.rung]
        return t

    def _place_join(self):
        c = self.n + 1
        assert self.row_of[c] == c
        p = orc.scores_to_probs(self.t_join)
        cdf = np.cumsum(p)
        lo, hi = cdf[self.lop] - p[self.lop], cdf[self.lop]
        assert p[self.lop] > 1e-3
        for key in range(SEED + c, SEED + c + 100000 * NCHAINS, NCHAINS):
            u = orc.uniform01(key, SWEEP, c)
            if lo + 0.25 * p[self.lop] < u < hi - 0.25 * p[self.lop]:
                self.seeds[c] = key
                return
        raise AssertionError("no key lands the near-mean row in group %d" % self.lop)

    # the tempered visit of row j at temperature beta (float32): log pseudocount + float64(beta) * (the features' sum)
    def t_tempered(self, j, beta):
        return self.crp[j].copy() if float(beta) == 0.0 else self.crp[j] + float(np.float32(beta)) * self.feat[j]

    def near_share(self):
        """-> (share of the untempered visits of fixture rows, share of the tempered visits) whose dart lies within EDGE
        of a step of the fixture's CDF"""
        plain = [near_edge(self.t[self.row_of[c]], self.u[c]) for c in range(NCHAINS) if self.row_of[c] < self.n]
        temp = [near_edge(self.t_tempered(j, self.beta_d[i]), self.u_d[j, i]) for j in range(self.n) for i in range(ND)]
        return float(np.mean(plain)), float(np.mean(temp))


# ---- the tables a visit leaves, exactly -----------------------------------------------------------------------------------

class ExactGroup(object):
    """one group's statistics of the five features as integers and rationals, from the float32 / uint32 fields of a rung"""

    def __init__(self, r):
        g = {nm: RUNGS[nm][r] for nm in NAMES}
        self.bb = [int(g["bb"]["heads"]), int(g["bb"]["tails"])]
        self.gp = [int(g["gp"]["count"]), int(g["gp"]["sum"])]
        self.log_prod = float(g["gp"]["log_prod"])
        self.bnb = [int(g["bnb"]["count"]), int(g["bnb"]["sum"])]
        self.dd = [int(x) for x in g["dd"]["counts"]]
        self.n = int(g["nich"]["count"])
        mean, ctv = Fraction(float(g["nich"]["mean"])), Fraction(float(g["nich"]["count_times_variance"]))
        self.sx, self.sxx = self.n * mean, ctv + self.n * mean * mean
        self.sxx_top, self.stores = self.sxx, 1          # the largest sum of squares held, and how often it was stored

    def move(self, row, sign):
        """the row (Visits.row_values) joins (sign 1) or leaves (sign -1)"""
        self.bb[0 if row["bb"] else 1] += sign
        self.gp[0] += sign
        self.gp[1] += sign * row["gp"]
        self.log_prod += sign * math.lgamma(row["gp"] + 1.0)
        self.bnb[0] += sign
        self.bnb[1] += sign * row["bnb"]
        self.dd[row["dd"]] += sign
        x = Fraction(row["nich"])
        self.n += sign
        self.sx += sign * x
        self.sxx += sign * x * x
        self.sxx_top, self.stores = max(self.sxx_top, self.sxx), self.stores + 1
        assert min(self.bb + self.gp + self.bnb + self.dd + [self.n]) >= 0

    def nich(self):
        """-> (mean, count_times_variance) as the commit defines them: no rows no mean, at most one row no scatter"""
        mean = self.sx / self.n if self.n > 0 else Fraction(0)
        ctv = self.sxx - self.sx * self.sx / self.n if self.n > 1 else Fraction(0)
        return mean, ctv

    def ctv_representation_bound(self):
        """what the state's additive table can hold of count_times_variance, relative: the table keeps sum x^2 in
        double, stored once when the fields are lifted into it and once a move, each store rounding it by up to half
        an ulp, 2^-53 of the sum; the field itself is a float32, half an ulp again, 2^-24.  From the exact sums alone."""
        ctv = self.nich()[1]
        return self.stores * 2.0 ** -53 * float(self.sxx_top) / float(ctv) + 2.0 ** -24 if ctv > 0 else 0.0
