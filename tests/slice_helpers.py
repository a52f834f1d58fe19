"""Host twin of slice sampling (msc_hp_slice / msc_theta_slice, include/microscopes_hip.h): the algorithm the header
states, restated in numpy / Python double arithmetic operation by operation, with orc.philox for the random words and the
oracle's double score_data / score_assignment for the targets.  The GPU tests replay every device update with it from
the device's pre-step values; test_slice_cpu.py checks the twin itself is stationary on closed-form targets."""
import math

import numpy as np

from oracle import oracle as orc

KEY_XOR = 0x2545F4914F6CDD1D
M = 64                       # stepping-out limit
SHRINK = 256                 # rejected proposals before the update stalls
OK, NON_FINITE, STALLED = 0, 1, 2
PRIOR_FLAT, PRIOR_EXPONENTIAL, PRIOR_NORMAL, PRIOR_NONINF_BETA = range(4)
U32 = 0xFFFFFFFF


def f32(x):
    return float(np.float32(x))


class Uniforms(object):
    """u_b of one update: Philox4x32-10 block b of counter (c0, c1, sweep & 0xffffffff, b), key seed ^ KEY_XOR"""

    def __init__(self, seed, c0, c1, sweep):
        key = (int(seed) ^ KEY_XOR) & 0xFFFFFFFFFFFFFFFF
        self.key = [key & U32, key >> 32]
        self.ctr = [int(c0) & U32, int(c1) & U32, int(sweep) & U32]

    def u(self, b):
        w = orc.philox(self.key, self.ctr + [b])
        return ((int(w[0]) >> 5) * 67108864.0 + (int(w[1]) >> 6) + 0.5) * (1.0 / 9007199254740992.0)


def hp_uniforms(seed, target, entry, sweep):
    return Uniforms(seed, target, entry, sweep)


def theta_uniforms(seed, slot, feature, sweep):
    return Uniforms(seed, slot, 0x80000000 | feature, sweep)


def slice_update(g, in_support, x0, w, uni):
    """One update (Neal 2003, Fig. 3 + Fig. 5) of the float x0 with width w -> (x, evals, status, comparisons): the
    installed float, the evaluations of g taken (inside the support only, g(x0) included), OK / NON_FINITE / STALLED,
    and every (y, g(z)) comparison made, in order."""
    x0 = f32(x0)
    w = f32(w)
    n = [0]
    cmps = []

    def at(z):
        f = f32(z)
        if not in_support(f):
            return -math.inf
        n[0] += 1
        return g(f)

    g0 = at(x0)
    if not math.isfinite(g0):
        return x0, n[0], NON_FINITE, cmps
    y = g0 + math.log(uni.u(0))
    L = x0 - w * uni.u(1)
    R = L + w
    J = int(math.floor(M * uni.u(2)))
    Kr = M - 1 - J

    def above(z):
        gz = at(z)
        cmps.append((y, gz))
        return y < gz

    while J > 0 and above(L):
        L -= w
        J -= 1
    while Kr > 0 and above(R):
        R += w
        Kr -= 1
    for j in range(SHRINK):
        x1 = f32(L + uni.u(3 + j) * (R - L))
        if above(x1):
            return x1, n[0], OK, cmps
        if x1 < x0:
            L = x1
        else:
            R = x1
    return x0, n[0], STALLED, cmps


def deciding_margin(cmps):
    """the smallest relative gap |y - g(z)| / max(1, |y|) over the comparisons of an update: where the device and the twin
    install different values, some comparison went the other way, and it must be this close"""
    m = math.inf
    for y, gz in cmps:
        if math.isfinite(gz):
            m = min(m, abs(y - gz) / max(1.0, abs(y)))
    return m


def log_prior(kind, x, a, b, partner):
    """MSC_PRIOR_* in double, as the device evaluates it (a, b, partner: the float32 values)"""
    if kind == PRIOR_EXPONENTIAL:
        return -math.inf if x < 0.0 else math.log(a) - a * x
    if kind == PRIOR_NORMAL:
        d = x - a
        return -0.5 * math.log(2.0 * math.pi * b) - 0.5 * (d * d) / b
    if kind == PRIOR_NONINF_BETA:
        return -2.5 * math.log(x + partner)
    return 0.0


def positive_support(family, coord):
    return not (family == orc.NICH and coord == 0)


def support(positive):
    if positive:
        return lambda x: 0.0 < x < math.inf
    return lambda x: math.isfinite(x)


def feature_target(family, dim, hp, coord, ss64, counted, prior, a, b, partner):
    """g(x) of one coordinate of a feature: the oracle's double score_data over the counted slots with hp[coord] = x,
    plus the prior"""
    sel = ss64[counted]
    base = np.array(hp, dtype=np.float32)
    a, b = f32(a), f32(b)

    def g(x):
        h = base.copy()
        h[coord] = x
        lik = float(orc.Family(family, h, dim, "f64").score_data_all(sel).sum()) if sel.shape[0] else 0.0
        return lik + log_prior(prior, x, a, b, f32(partner))
    return g


def alpha_target(counts, prior, a, b):
    z = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    a, b = f32(a), f32(b)
    return lambda x: orc.score_assignment(z, x) + log_prior(prior, x, a, b, 0.0)


def theta_target(hp, heads, tails):
    """bbnc_score_data(hp, heads, tails, p) from the oracle's double twin"""
    F = orc.Family(orc.BBNC, np.asarray(hp, dtype=np.float32), 0, "f64")
    ss = np.zeros(1, dtype=orc.ss_dtype(orc.BBNC, 0, "f64"))
    ss["heads"], ss["tails"] = heads, tails

    def g(p):
        ss["p"] = p
        return F.score_data(ss, 0)
    return g


def theta_support(p):
    return 0.0 < p < 1.0
