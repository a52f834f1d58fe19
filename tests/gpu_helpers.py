"""Shared builders for the -m gpu parity tests: seeded synthetic features, the
float state the device is given, and the same state widened for the double twin."""
import numpy as np

from oracle import oracle as orc

TOL = 1e-6  # north_star: float log-scores within 1e-6 relative of the double evaluation


_AUDIT = {}


def audit(name, err, gate):
    """every gate that is not the plain TOL goes through here: the largest error seen per gate is kept and, with
    MSC_TOL_AUDIT=<file> in the environment, written out when the session ends (profiles/r03_tolerance_audit.json is
    such a run) -- a gate is a budget with a reason, and this is the evidence it is held against"""
    err = float(err)
    rec = _AUDIT.setdefault(name, {"max_err": 0.0, "gate": float(gate), "checks": 0})
    rec["max_err"] = max(rec["max_err"], err)
    rec["gate"] = max(rec["gate"], float(gate))
    rec["checks"] += 1
    assert err <= gate, (name, err, gate)


def _dump_audit():
    import json
    import os
    path = os.environ.get("MSC_TOL_AUDIT")
    if path and _AUDIT:
        with open(path, "w") as fh:
            json.dump(_AUDIT, fh, indent=1, sort_keys=True)


import atexit  # noqa: E402
atexit.register(_dump_audit)


def rel_err(got, want):
    """|got - want| / max(1, |want|): relative for |score| >= 1, absolute below."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def make_feature(family, N, K, rng, dim=0, hp=None):
    """-> dict(family, dim, hp, values, np_dtype) with group structure in the data."""
    z_true = rng.integers(0, K, N)
    if family in (orc.BB, orc.BBNC):
        p = rng.random(K)
        vals = (rng.random(N) < p[z_true]).astype(np.bool_)
        hp = hp or dict(alpha=1.0, beta=1.0)
        dt = np.bool_
    elif family == orc.GP:
        lam = rng.gamma(2.0, 2.0, K)
        vals = rng.poisson(lam[z_true]).astype(np.uint32)
        hp = hp or dict(alpha=1.0, inv_beta=1.0)
        dt = np.uint32
    elif family == orc.BNB:
        pr = rng.uniform(0.15, 0.8, K)
        r = int((hp or {}).get("r", 3))
        vals = rng.negative_binomial(r, pr[z_true]).astype(np.uint32)
        hp = hp or dict(alpha=1.5, beta=2.0, r=3)
        dt = np.uint32
    elif family == orc.DM:
        th = rng.dirichlet(np.ones(dim) * 0.7, K)
        tot = rng.integers(0, 40, N)
        vals = np.array([rng.multinomial(t, th[g]) for t, g in zip(tot, z_true)], dtype=np.int32).reshape(N, dim)
        hp = hp or dict(alphas=list(rng.uniform(0.3, 2.0, dim).astype(np.float32)))
        dt = np.dtype((np.int32, (dim,)))
    elif family == orc.DD:
        th = rng.dirichlet(np.ones(dim), K)
        cdf = th.cumsum(1)
        vals = (rng.random(N)[:, None] > cdf[z_true]).sum(1).clip(0, dim - 1).astype(np.int32)
        hp = hp or dict(alphas=[1.0] * dim)
        dt = np.int32
    elif family == orc.NICH:
        centres = rng.normal(0, 10, K)
        vals = (centres[z_true] + rng.normal(0, 1, N)).astype(np.float32)
        hp = hp or dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0)
        dt = np.float32
    elif family == orc.NIW:
        centres = rng.normal(0, 3, (K, dim))
        A = rng.normal(0, 1, (K, dim, dim)) / np.sqrt(dim)
        vals = (centres[z_true] + np.einsum("nij,nj->ni", A[z_true], rng.normal(0, 1, (N, dim)))).astype(np.float32)
        hp = hp or dict(mu=np.zeros(dim), kappa=1.0, psi=np.eye(dim), nu=float(dim))
        dt = np.dtype((np.float32, (dim,)))
    else:
        raise ValueError(family)
    return dict(family=family, dim=dim, hp=hp, values=vals, np_dtype=dt)


# the state of several features that the hyperparameter tests run, feature j on distinct_hp(.., i=j)
MIXED = [(orc.BB, 0), (orc.BB, 0), (orc.GP, 0), (orc.GP, 0), (orc.DD, 7), (orc.DD, 33), (orc.NICH, 0), (orc.NICH, 0),
         (orc.NICH, 0), (orc.BNB, 0), (orc.DM, 4), (orc.BBNC, 0), (orc.NIW, 3)]


def distinct_hp(family, dim=0, i=0):
    """A hyperparameter block in which no two fields can stand in for each other: every value a dyadic rational (the
    float block the device is given and the double twin see the same number), the fields of a block different from each
    other and from 1, mu away from 0, psi dense.  make_feature's defaults (all ones, mu = 0, psi = I) cannot tell alpha
    from beta, inv_beta from beta, one alphas index from another, kappa from nu, or a dropped kappa mu mu^T / nu sigmasq
    / ln det psi term from a kept one.  i: the variant for the i-th feature of a state (every positive scalar + i / 8,
    mu - i / 2, alphas rotated by i places, r = 4 + i % 3), so that reading another feature's block shows as well.
    (alphas cycle with period 7 and niw's mu[j] = ((5 j) % 7 - 3) / 2 passes through 0 at j = 2 mod 7: vectors longer
    than that repeat values, neighbours still differ.  "Different from each other and from 1" holds at i = 0 and for
    feature j of MIXED at i = j -- the variants the tests use, asserted in test_hypers_cpu.py -- not for every i: nich
    at i = 5 has kappa = 1.)"""
    s = 0.125 * i
    if family in (orc.BB, orc.BBNC):
        return dict(alpha=0.75 + s, beta=2.5 + s)
    if family == orc.GP:
        return dict(alpha=2.5 + s, inv_beta=0.375 + s)
    if family == orc.BNB:
        return dict(alpha=2.5 + s, beta=0.75 + s, r=4 + i % 3)
    if family in (orc.DD, orc.DM):
        base = [0.25 + 0.5 * ((3 * j) % 7) for j in range(dim)]
        return dict(alphas=[float(a) + s for a in np.roll(base, i)])
    if family == orc.NICH:
        return dict(mu=-1.25 - 0.5 * i, kappa=0.375 + s, sigmasq=2.5 + s, nu=3.5 + s)
    if family == orc.NIW:
        B = np.random.default_rng(1000 + dim).standard_normal((dim, dim))
        psi = (B @ B.T / dim + 1.5 * np.eye(dim)).astype(np.float32).astype(np.float64)
        psi = np.tril(psi) + np.tril(psi, -1).T          # (the device reads the lower triangle: exactly symmetric)
        mu = np.array([((5 * j) % 7 - 3) / 2.0 for j in range(dim)]) - 0.5 * i
        return dict(mu=mu, kappa=0.75 + s, psi=psi, nu=dim + 2.5 + s)
    raise ValueError(family)


def random_hp(family, dim, hrng):
    """A block drawn from hrng (the fuzzers' hyperparameter stream -- a generator of its own, so the shapes, data and masks
    a seed draws stay what they were): positive scalars log-uniform in [0.25, 4], mu uniform in [-3, 3], niw a dense
    symmetric psi with a random diagonal load and nu = dim + U(0.5, 4); bnb's r stays 3 (make_feature draws the data
    with it).  Every value is rounded to float: the device's block and the twin's hold the same numbers."""
    def pos(size=None):
        return np.asarray(np.exp(hrng.uniform(np.log(0.25), np.log(4.0), size))).astype(np.float32).astype(np.float64)

    def loc(size=None):
        return np.asarray(hrng.uniform(-3.0, 3.0, size)).astype(np.float32).astype(np.float64)
    if family in (orc.BB, orc.BBNC):
        return dict(alpha=float(pos()), beta=float(pos()))
    if family == orc.GP:
        return dict(alpha=float(pos()), inv_beta=float(pos()))
    if family == orc.BNB:
        return dict(alpha=float(pos()), beta=float(pos()), r=3)
    if family in (orc.DD, orc.DM):
        return dict(alphas=[float(a) for a in pos(dim)])
    if family == orc.NICH:
        return dict(mu=float(loc()), kappa=float(pos()), sigmasq=float(pos()), nu=float(pos()))
    if family == orc.NIW:
        B = hrng.standard_normal((dim, dim))
        psi = (B @ B.T / dim + np.diag(hrng.uniform(0.5, 2.5, dim))).astype(np.float32).astype(np.float64)
        psi = np.tril(psi) + np.tril(psi, -1).T
        return dict(mu=loc(dim), kappa=float(pos()), psi=psi, nu=float(np.float32(dim + hrng.uniform(0.5, 4.0))))
    raise ValueError(family)


def edge_assignment(N, K, rng):
    """-> z with the edge state every hyperparameter test wants: the last group empty, the one before it a singleton
    (row 3: leaving it empties the group, its leave-one-out score is the prior's alone), row 5 unassigned"""
    z = rng.integers(0, K - 2, N).astype(np.int32)
    z[3] = K - 2
    z[5] = -1
    return z


def recarray_of(features):
    dt = np.dtype([("f%d" % i, f["np_dtype"]) for i, f in enumerate(features)])
    arr = np.zeros(len(features[0]["values"]), dtype=dt)
    for i, f in enumerate(features):
        arr["f%d" % i] = f["values"]
    return arr


def state_from_assignment(features, K, z):
    """Suff-stats of every feature given z: accumulate in double, round the float
    fields to float (what the device stores), widen again for the twin.
    -> list of (Family64, ss64_of_float_state, ss32)."""
    out = []
    for f in features:
        F = orc.Family(f["family"], f["hp"], f["dim"], "f64")
        init = None
        if f["family"] == orc.BBNC:     # the group's explicit p is state, drawn once per group
            init = np.zeros(K, dtype=orc.ss_dtype(orc.BBNC, 0, "f64"))
            init["p"] = np.random.default_rng(K).uniform(0.05, 0.95, K).astype(np.float32)
        ss64 = F.accumulate(K, f["values"], z, ss_init=init)
        ss32 = orc.narrow_ss(f["family"], ss64, f["dim"])
        out.append((F, orc.widen_ss(f["family"], ss32, f["dim"]), ss32))
    return out


def load_state(st, feats_state):
    """push hp + float suff-stats of every feature into a common_amd.State"""
    import common_amd
    for i, (F, _, ss32) in enumerate(feats_state):
        st.set_hp(i, F.hp)
        rec = np.zeros(ss32.shape[0], dtype=common_amd.ss_dtype(F.family, F.dim))
        for name in rec.dtype.names:
            rec[name] = ss32[name]
        st.set_ss(i, rec)


def oracle_scores(features, feats_state, z=None, rows=None):
    """double-twin [n, K] matrix summed over features (optionally leave-one-out)."""
    total = None
    for f, (F, ss64, _) in zip(features, feats_state):
        v = f["values"] if rows is None else f["values"][rows]
        zz = None if z is None else (z if rows is None else z[rows])
        m = F.score_matrix(ss64, v, zz)
        total = m if total is None else total + m
    return total


def crp_prior_matrix(counts, alpha, z=None):
    """[n, K] log pseudocounts (group_manager.hpp:274-283); with z: row n removed first."""
    counts = np.asarray(counts, dtype=np.int64)
    K = counts.shape[0]
    ne = int((counts == 0).sum())
    if z is None:
        base = np.where(counts > 0, np.log(np.maximum(counts, 1)), np.log(alpha / max(ne, 1)))
        return base[None, :]
    out = np.empty((len(z), K))
    for n, g in enumerate(z):
        c = counts.copy()
        if g >= 0:
            c[g] -= 1
        ne_n = int((c == 0).sum())
        out[n] = np.where(c > 0, np.log(np.maximum(c, 1)), np.log(alpha / max(ne_n, 1)))
    return out
