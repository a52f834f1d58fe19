"""Shared by tests/test_blocked_niw_cpu.py and tests/test_gpu_blocked_niw.py: the host build of
common_amd/csrc/blocked_niw.hpp, a numpy restatement of the niw posterior, and the statistics that hold a batch of drawn
(mean, whiten, c) to the posterior -- one set of checks for the host's draws and the device's."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_GATE = 1e-3
SEED = 20261021


def build_host(tmpdir):
    out = os.path.join(str(tmpdir), "blocked_niw_host.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "common_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "blocked_niw_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.niw_max_dim.restype = C.c_uint32
    lib.niw_post_host.argtypes = [C.c_uint32, vp, C.c_double, vp, vp, vp]
    lib.niw_draw_host.argtypes = [C.c_uint32, vp, C.c_double, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                  C.c_uint32, vp, vp, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hp_block(hp, d):
    """{kappa, nu, mu[d], psi[d * d]} as the float block the device holds"""
    return np.ascontiguousarray(np.concatenate([[hp["kappa"], hp["nu"]], np.asarray(hp["mu"]).ravel(),
                                                np.asarray(hp["psi"]).ravel()]), dtype=np.float32)


def members(d, n, centre=2.0):
    """n rows of dimension d with a dense covariance, and their float sums as a slot's record holds them"""
    rng = np.random.default_rng(7 + 31 * d + n)
    B = rng.standard_normal((d, d)) / math.sqrt(d) + np.eye(d)
    x = (centre + rng.standard_normal((n, d)) @ B.T).astype(np.float32)
    x64 = x.astype(np.float64)
    return x, x64.sum(0).astype(np.float32), (x64.T @ x64).astype(np.float32)


def posterior(hpb, d, n, sx, sxx):
    """kappa_n, nu_n, mu_n, Psi_n in double from the float block and the float sums"""
    hpb = hpb.astype(np.float64)
    kappa, nu, mu, psi = hpb[0], hpb[1], hpb[2:2 + d], hpb[2 + d:].reshape(d, d)
    psi = np.tril(psi) + np.tril(psi, -1).T              # (the lower triangle is what is read)
    sx, sxx = sx.astype(np.float64), sxx.astype(np.float64)
    sxx = np.tril(sxx) + np.tril(sxx, -1).T
    kn, nun = kappa + n, nu + n
    mun = (kappa * mu + sx) / kn
    return kn, nun, mun, psi + sxx + kappa * np.outer(mu, mu) - kn * np.outer(mun, mun)


def host_post(lib, hpb, d, n, sx, sxx):
    out = np.zeros(2 + d + d * d)
    lib.niw_post_host(d, _p(hpb), float(n), _p(sx), _p(sxx), _p(out))
    return out[0], out[1], out[2:2 + d].copy(), out[2 + d:].reshape(d, d).copy()


def host_draws(lib, hpb, d, n, sx, sxx, nslots, seed=SEED, sweep=0, slot0=0, tag=0):
    nt = d * (d + 1) // 2
    mean, whiten, vmu = np.zeros((nslots, d)), np.zeros((nslots, nt)), np.zeros((nslots, d))
    c = np.zeros(nslots, dtype=np.float32)
    lib.niw_draw_host(d, _p(hpb), float(n), _p(sx), _p(sxx), slot0, nslots, seed, sweep, tag, _p(mean), _p(whiten), _p(vmu),
                      _p(c))
    return mean, whiten, vmu, c


def unpack(whiten, d):
    """[n, d (d + 1) / 2] packed rows -> [n, d, d] lower-triangular V"""
    V = np.zeros((whiten.shape[0], d, d))
    i, j = np.tril_indices(d)                            # row-major over the lower triangle: tri(i, j) = i (i + 1) / 2 + j
    V[:, i, j] = whiten
    return V


def ks(x, dist):
    p = stats.kstest(x, dist.cdf).pvalue
    assert p >= P_GATE, p
    return p


def ks2(x, y):
    p = stats.ks_2samp(x, y).pvalue
    assert p >= P_GATE, p
    return p


def fixed_vector(d):
    """a vector along no axis, every entry different"""
    return np.array([(-1.0) ** j * (1.0 + 0.25 * j) for j in range(d)])


def reference_sigmas(nun, Psin, n, seed=SEED):
    return np.asarray(stats.invwishart(df=nun, scale=Psin).rvs(n, random_state=np.random.default_rng(seed))).reshape(n, *Psin.shape)


def sigma_stats(Sigma):
    return np.linalg.slogdet(Sigma)[1], Sigma[:, 1, 0]


def check_draws(mean, whiten, c, d, kn, nun, mun, Psin):
    """the drawn (mean, whiten, c) of identical slots against NIW(mu_n, kappa_n, Psi_n, nu_n)"""
    n = mean.shape[0]
    assert np.isfinite(mean).all() and np.isfinite(whiten).all() and np.isfinite(c).all()
    V = unpack(whiten, d)
    a = fixed_vector(d)
    Pinv = np.linalg.inv(Psin)
    # Sigma^-1 = V^T V ~ W(Psi_n^-1, nu_n): a^T Sigma^-1 a / a^T Psi_n^-1 a ~ chi2(nu_n)
    ks(((V @ a) ** 2).sum(1) / (a @ Pinv @ a), stats.chi2(nun))
    # Sigma ~ IW(Psi_n, nu_n): Psi_n[i, i] / Sigma[i, i] ~ chi2(nu_n - d + 1) at both ends of the diagonal (a Bartlett
    # factor with the degrees of freedom in the usual order fails at one of them)
    Vinv = np.linalg.inv(V)
    Sigma = Vinv @ np.transpose(Vinv, (0, 2, 1))
    for i in (0, d - 1):
        ks(Psin[i, i] / Sigma[:, i, i], stats.chi2(nun - d + 1))
    ref = reference_sigmas(nun, Psin, n)
    got_ld, got_off = sigma_stats(Sigma)
    ref_ld, ref_off = sigma_stats(ref)
    ks2(got_ld, ref_ld)
    ks2(got_off, ref_off)
    # mu | Sigma ~ N(mu_n, Sigma / kappa_n): sqrt(kappa_n) V (mu - mu_n) ~ N(0, I)
    zs = math.sqrt(kn) * np.einsum("nij,nj->ni", V, mean - mun[None, :])
    ks(zs.ravel(), stats.norm())
    want_c = -0.5 * d * math.log(2.0 * math.pi) + np.log(np.diagonal(V, axis1=1, axis2=2)).sum(1)
    assert np.allclose(c, want_c, rtol=1e-5, atol=1e-5)
