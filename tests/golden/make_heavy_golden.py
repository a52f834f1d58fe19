#!/usr/bin/env python
"""Generate tests/golden/heavy.json: score_value, leave-one-out score_value and score_data of every family on the heavy
rungs of tests/heavy_cases.py, and the CRP term score_assignment of the heavy layouts' group counts, evaluated with
mpmath at 60 digits.

The double twin (oracle/) cannot arbitrate at these sizes: it takes the same differences of lgamma in double as the
device's prepare steps, and those cancel at the size of lgamma's value (1e9 ln 1e9), not of the result.  Here every
formula -- the definitions in family_math.hpp's comments and oracle/msc_oracle_impl.inc, remove_value included -- is
evaluated from the EXACT values of the float32 / uint32 statistics and float32 hyperparameters the device is given, so
the rounding of inputs is not an error source, and rounded to double once at the end.

Run:  python tests/golden/make_heavy_golden.py     (rewrites tests/golden/heavy.json; needs mpmath)
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf, loggamma, log, matrix, cholesky, pi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import oracle as orc                # noqa: E402
from tests import heavy_cases as hc             # noqa: E402

mp.dps = 60
lg = loggamma
M = lambda x: mpf(float(x))                     # a float32 / double / integer below 2^53, exactly


class Infeasible(Exception):
    pass


# ---- per family: score_value(hp, group, value), remove(group, value) -> group, score_data(hp, group) -----------------
# a group is a dict of mpf / lists of mpf named as the suff-stat record's fields

def group_of(name, rec):
    fam, dim = hc.FAMILIES[name]
    g = {}
    for f in rec.dtype.names:
        a = np.asarray(rec[f])
        g[f] = M(a) if a.ndim == 0 else ([M(x) for x in a] if a.ndim == 1 else matrix([[M(x) for x in r] for r in a]))
    return g


def need(cond):
    if not cond:
        raise Infeasible()


def bb_sv(hp, g, v):
    a, b = hp
    return log(((a + g["heads"]) if v else (b + g["tails"])) / (a + b + g["heads"] + g["tails"]))


def bb_rm(g, v):
    f = "heads" if v else "tails"
    need(g[f] >= 1)
    return dict(g, **{f: g[f] - 1})


def bb_sd(hp, g):
    a, b = hp
    h, t = g["heads"], g["tails"]
    return lg(a + b) - lg(a + b + h + t) + lg(a + h) - lg(a) + lg(b + t) - lg(b)


def mlog(x):
    return mpf("-inf") if x == 0 else log(x)


def bbnc_sv(hp, g, v):
    return mlog(g["p"]) if v else mlog(1 - g["p"])


def bbnc_sd(hp, g):
    a, b = hp
    p = g["p"]
    lbeta = lg(a) + lg(b) - lg(a + b)
    return (a - 1) * log(p) + (b - 1) * log(1 - p) - lbeta + g["heads"] * log(p) + g["tails"] * log(1 - p)


def gp_sv(hp, g, v):
    a, b = hp[0] + g["sum"], hp[1] + g["count"]
    return lg(a + v) - lg(a) - lg(v + 1) + a * log(b) - (a + v) * log(1 + b)


def cnt_rm(g, v):
    need(g["count"] >= 1 and g["sum"] >= v)
    return dict(g, count=g["count"] - 1, sum=g["sum"] - v)


def gp_sd(hp, g):
    al, ib = hp
    a, b = al + g["sum"], ib + g["count"]
    return lg(a) - lg(al) + al * log(ib) - a * log(b) - g["log_prod"]


def bnb_sv(hp, g, v):
    al, be, r = hp
    a, b = al + r * g["count"], be + g["sum"]
    return lg(r + v) - lg(v + 1) - lg(r) + lg(a + b) - lg(a) - lg(b) + lg(a + r) + lg(b + v) - lg(a + r + b + v)


def bnb_sd(hp, g):
    al, be, r = hp
    a, b = al + r * g["count"], be + g["sum"]
    return lg(al + be) - lg(al) - lg(be) + lg(a) + lg(b) - lg(a + b)


def dd_sv(hp, g, v):
    v = int(v)
    return log((hp[v] + g["counts"][v]) / (sum(hp) + g["count_sum"]))


def dd_rm(g, v):
    v = int(v)
    need(g["counts"][v] >= 1)
    c = list(g["counts"])
    c[v] -= 1
    return dict(count_sum=g["count_sum"] - 1, counts=c)


def dd_sd(hp, g):
    return sum(lg(a + c) - lg(a) for a, c in zip(hp, g["counts"])) + lg(sum(hp)) - lg(sum(hp) + g["count_sum"])


def dm_sv(hp, g, x):
    A, N, X = sum(hp), sum(g["counts"]), sum(x)
    s = sum(lg(a + n + xi) - lg(a + n) - lg(xi + 1) for a, n, xi in zip(hp, g["counts"], x))
    return s + lg(X + 1) + lg(A + N) - lg(A + N + X)


def dm_rm(g, x):
    need(all(n >= xi for n, xi in zip(g["counts"], x)))
    return dict(g, counts=[n - xi for n, xi in zip(g["counts"], x)])


def dm_sd(hp, g):
    A, N = sum(hp), sum(g["counts"])
    return g["ratio"] + sum(lg(c + a) - lg(a) for a, c in zip(hp, g["counts"])) + lg(A) - lg(A + N)


def nich_post(hp, g):
    mu, kappa, sigmasq, nu = hp
    n, mean, ctv = g["count"], g["mean"], g["count_times_variance"]
    d = mu - mean
    kn, nun = kappa + n, nu + n
    return (kappa * mu + mean * n) / kn, kn, (nu * sigmasq + ctv + (n * kappa * d * d) / kn) / nun, nun


def nich_sv(hp, g, x):
    mun, kn, sn, nun = nich_post(hp, g)
    lam = kn / ((kn + 1) * sn)
    d = x - mun
    return lg(nun / 2 + mpf(1) / 2) - lg(nun / 2) + log(lam / (pi * nun)) / 2 - (nun / 2 + mpf(1) / 2) * log(1 + lam * d * d / nun)


def nich_rm(g, x):
    n, mean, ctv = g["count"], g["mean"], g["count_times_variance"]
    need(n >= 1)
    total, delta = mean * n, x - mean
    n1 = n - 1
    mean1 = mpf(0) if n1 == 0 else (total - x) / n1
    if n1 <= 1:
        ctv1 = mpf(0)               # (remove_value's own rule: a group of at most one row has no scatter)
    else:
        ctv1 = ctv - delta * (x - mean1)
        need(ctv1 > 0)
    return dict(count=n1, mean=mean1, count_times_variance=ctv1)


def nich_sd(hp, g):
    mu, kappa, sigmasq, nu = hp
    mun, kn, sn, nun = nich_post(hp, g)
    return lg(nun / 2) - lg(nu / 2) + log(kappa / kn) / 2 + nu / 2 * log(nu * sigmasq) - nun / 2 * log(nun * sn) - \
        g["count"] / 2 * log(pi)


def niw_hp(hp, d):
    kappa, nu = hp[0], hp[1]
    mu = matrix(hp[2:2 + d])
    psi = matrix(d, d)
    for i in range(d):
        for j in range(d):
            psi[i, j] = hp[2 + d + i * d + j]
    return kappa, nu, mu, psi


def niw_post(hp, g):
    d = len(g["sum_x"])
    kappa, nu, mu, psi = niw_hp(hp, d)
    n, sx = g["count"], matrix(g["sum_x"])
    kn, nun = kappa + n, nu + n
    mun = (kappa * mu + sx) / kn
    psin = psi + g["sum_xxT"] + kappa * (mu * mu.T) - kn * (mun * mun.T)
    return d, kn, nun, mun, psin


def chol_logdet(a):
    try:
        L = cholesky(a)             # raises on a matrix that is not positive definite
    except ValueError:
        raise Infeasible()
    return L, 2 * sum(log(L[i, i]) for i in range(a.rows))


def niw_sv(hp, g, x):
    if "_sv" not in g:                  # (the values of a rung share its factorisation)
        d, kn, nun, mun, psin = niw_post(hp, g)
        dof = nun - d + 1
        g["_sv"] = (d, dof, mun) + chol_logdet(psin * ((kn + 1) / (kn * dof)))
    d, dof, mun, L, logdet = g["_sv"]
    y = mp.lu_solve(L, matrix(x) - mun)
    q = sum(t * t for t in y)
    return lg((dof + d) / 2) - lg(dof / 2) - mpf(d) / 2 * log(dof * pi) - logdet / 2 - (dof + d) / 2 * log(1 + q / dof)


def niw_rm(g, x):
    need(g["count"] >= 1)
    xv = matrix(x)
    return dict(count=g["count"] - 1, sum_x=[a - b for a, b in zip(g["sum_x"], x)], sum_xxT=g["sum_xxT"] - xv * xv.T)


def lmultigamma(d, a):
    return mpf(d * (d - 1)) / 4 * log(pi) + sum(lg(a + mpf(1 - j) / 2) for j in range(1, d + 1))


def niw_sd(hp, g):
    d, kn, nun, mun, psin = niw_post(hp, g)
    kappa, nu, mu, psi = niw_hp(hp, d)
    ld0, ldn = chol_logdet(psi)[1], chol_logdet(psin)[1]
    return lmultigamma(d, nun / 2) - lmultigamma(d, nu / 2) + nu / 2 * ld0 - nun / 2 * ldn + mpf(d) / 2 * log(kappa / kn) - \
        g["count"] * d / 2 * log(pi)


FORMULAS = {orc.BB: (bb_sv, bb_rm, bb_sd), orc.BBNC: (bbnc_sv, bb_rm, bbnc_sd), orc.GP: (gp_sv, cnt_rm, gp_sd),
            orc.BNB: (bnb_sv, cnt_rm, bnb_sd), orc.DD: (dd_sv, dd_rm, dd_sd), orc.DM: (dm_sv, dm_rm, dm_sd),
            orc.NICH: (nich_sv, nich_rm, nich_sd), orc.NIW: (niw_sv, niw_rm, niw_sd)}


def family_table(name):
    """-> dict(score_value [R][V], loo [R][V] (None where infeasible), loo_ok [R][V], score_data [R]) of Python floats"""
    fam, dim = hc.FAMILIES[name]
    sv, rm, sd = FORMULAS[fam]
    hp = [M(x) for x in hc.hp_block(name)]
    vals = [[M(x) for x in v] if np.ndim(v) else M(v) for v in hc.values(name)]
    out = dict(score_value=[], loo=[], loo_ok=[], score_data=[])
    for rec in hc.rungs(name):
        g = group_of(name, rec)
        if fam == orc.NIW:
            chol_logdet(niw_post(hp, g)[4])     # the posterior scale matrix of the rung itself: positive definite
        out["score_data"].append(float(sd(hp, g)))
        out["score_value"].append([float(sv(hp, g, v)) for v in vals])
        row = []
        for v in vals:
            try:
                row.append(float(sv(hp, rm(g, v), v)))
            except Infeasible:
                row.append(None)
        out["loo"].append(row)
        out["loo_ok"].append([int(x is not None) for x in row])
    return out


def score_assignment(counts, alpha):
    """the CRP term of a partition with these group sizes: occ ln(alpha) + sum lgamma(n_k) + lgamma(alpha) - lgamma(N + alpha)
    over the occupied groups (group_manager.hpp score_assignment)"""
    a = M(alpha)
    occ = [int(c) for c in counts if c > 0]
    return len(occ) * log(a) + sum(lg(mpf(c)) for c in occ) + lg(a) - lg(mpf(sum(occ)) + a)


def assignment_table():
    """-> {layout key: score_assignment} at alpha = float32(1.3), for the count vectors of hc.layout_counts"""
    return dict(alpha=float(hc.ALPHA32),
                **{key: float(score_assignment(hc.layout_counts(R, K), hc.ALPHA32)) for key, (R, K) in hc.LAYOUT_KEYS.items()})


def generate():
    return dict(dps=mp.dps, counts=hc.COUNTS, families={name: family_table(name) for name in hc.FAMILIES},
                score_assignment=assignment_table())


def _enc(o):
    if isinstance(o, dict):
        return "{" + ", ".join('"%s": %s' % (k, _enc(o[k])) for k in sorted(o)) + "}"
    if isinstance(o, (list, tuple)):
        return "[" + ", ".join(_enc(x) for x in o) + "]"
    if o is None:
        return "null"
    if isinstance(o, float):
        return "%.17g" % o if np.isfinite(o) else ("-Infinity" if o < 0 else "Infinity")
    return "%d" % o


def main():
    doc = generate()
    with open(hc.FIXTURE, "w") as fh:
        fh.write('{"counts": %s, "dps": %d, "families": {\n' % (_enc(doc["counts"]), doc["dps"]))
        fh.write(",\n".join('"%s": %s' % (n, _enc(doc["families"][n])) for n in sorted(doc["families"])))
        fh.write("\n}, \"score_assignment\": %s}\n" % _enc(doc["score_assignment"]))
    print("wrote %s: %d bytes" % (hc.FIXTURE, os.path.getsize(hc.FIXTURE)))


if __name__ == "__main__":
    main()
