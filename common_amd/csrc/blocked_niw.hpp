// blocked_niw.hpp -- the blocked (uncollapsed) Gibbs sampler's parameter draw of a Normal-Inverse-Wishart feature
// (msc_blocked_draw, kernels_blocked_niw.hip k_blocked_draw_niw), in the manner of blocked_post.hpp: plain functions over
// the variate generators of pred_samplers.hpp, so that the host compiler builds the same code
// (tests/test_blocked_niw_cpu.py checks posterior and draws against scipy without a GPU).  One body: every function
// that more than one thread can share takes (t, nt, sync) -- the caller's index among nt workers and their barrier -- and
// the host calls it with (0, 1, a no-op); the kernel with its 64 threads and __syncthreads.
//
// Posterior of a slot, in double, from the reference's fields as k_niw_prepare reads them: hp {kappa, nu, mu[d],
// psi[d * d]}, raw {count, sum_x[d], sum_xxT[d * d]}:
//   kappa_n = kappa + n, nu_n = nu + n, mu_n = (kappa mu + sum_x) / kappa_n,
//   Psi_n = psi + sum_xxT + kappa mu mu^T - kappa_n mu_n mu_n^T = L L^T.
//
// The draw leaves a TRIANGULAR whitening matrix V with Sigma = (V^T V)^-1 ~ IW(Psi_n, nu_n): the operand stream of the
// matrix kernels holds only the blocks on or below the diagonal.  T lower triangular, T_ii^2 ~ chi2(nu_n - d + 1 + i)
// (0-based: the degrees of freedom INCREASE down the diagonal), T_ij ~ N(0, 1) for j < i; V = T L^-1.  Why: with
// Psi_n^-1 = L^-T L^-1, Sigma^-1 = V^T V = L^-T (T^T T) L^-1 ~ W(Psi_n^-1, nu_n) needs T^T T ~ W(I, nu_n).  Bartlett's
// factor B (lower, B_ii^2 ~ chi2(nu_n - i)) gives B B^T ~ W(I, nu_n); reversing the order of the coordinates turns B B^T
// into T^T T with T = J B^T J lower triangular and T_ii = B_{d-1-i, d-1-i}: chi2(nu_n - d + 1 + i).  The usual order on
// the diagonal of a lower factor gives the law of B^T B, which is not Wishart.
// The mean: mu = mu_n + V^-1 z / sqrt(kappa_n), z ~ N(0, I) (cov (V^T V)^-1 / kappa_n = Sigma / kappa_n), so
// V mu = V mu_n + z / sqrt(kappa_n) needs no solve.
//
// Streams: key = seed ^ kKey; matrix row i of slot k draws from pred::Stream(key, (i + 1) << 32 | k, sweep, tag): first
// z_i, then T_i0 .. T_i,i-1, then the chi2 of T_ii.  Every other stream of the sampler has a high counter word of 0.
// Nothing but (seed, sweep, slot, row, tag) enters a counter.
//
// What a slot's draw leaves: V as a packed lower triangle (tri(i, j) = i (i + 1) / 2 + j), mu, V mu, and the one float
// slice c = -(d / 2) ln 2 pi + sum_i ln V_ii, so that the log-likelihood of x is c - |V x - V mu|^2 / 2.
#pragma once

#include "blocked_post.hpp"

namespace msc {
namespace blocked {

constexpr uint32_t kNiwMaxDim = 32;                // what the blocked sweep takes (route_calls.hpp route_blocked)

MSC_PRED_HD size_t tri(uint32_t i, uint32_t j) { return (size_t)i * (i + 1u) / 2u + j; }
MSC_PRED_HD size_t ntri(uint32_t d) { return (size_t)d * (d + 1u) / 2u; }

// a stored double: finite, whatever the draw or a degenerate Psi_n made of it
MSC_PRED_HD double fin64(double v) { return (v > -1e300 && v < 1e300) ? v : 0.0; }

struct NoSync {
  MSC_PRED_HD void operator()() const {}
};

// kappa_n, nu_n, mu_n[d] and the packed lower triangle of Psi_n into A
template <class Sync>
MSC_PRED_HD void niw_post(uint32_t d, const float *hp, double n, const float *sx, const float *sxx, double *kappa_n,
                          double *nu_n, double *mun, double *A, uint32_t t, uint32_t nt, Sync sync) {
  const double kappa = hp[0], nu = hp[1];
  const float *mu = hp + 2, *psi = hp + 2 + d;
  const double kn = kappa + n;
  *kappa_n = kn;
  *nu_n = nu + n;
  for (uint32_t i = t; i < d; i += nt) mun[i] = (kappa * (double)mu[i] + (double)sx[i]) / kn;
  sync();
  for (uint32_t idx = t; idx < d * d; idx += nt) {
    const uint32_t i = idx / d, j = idx - i * d;
    if (j > i) continue;
    A[tri(i, j)] = (double)psi[idx] + (double)sxx[idx] + kappa * (double)mu[i] * (double)mu[j] - kn * mun[i] * mun[j];
  }
  sync();
}

// A (packed Psi_n) -> L in place, L^-1 into Li; the pivots are kept positive, so both stay finite
template <class Sync>
MSC_PRED_HD void niw_factor(uint32_t d, double *A, double *Li, uint32_t t, uint32_t nt, Sync sync) {
  for (uint32_t j = 0; j < d; j++) {               // right-looking Cholesky, lower triangle
    const double ajj = A[tri(j, j)];
    const double ljj = sqrt(ajj > 1e-300 ? ajj : 1e-300);
    sync();
    for (uint32_t i = j + 1 + t; i < d; i += nt) A[tri(i, j)] /= ljj;
    if (t == 0) A[tri(j, j)] = ljj;
    sync();
    const uint32_t m = d - j - 1;
    for (uint32_t idx = t; idx < m * m; idx += nt) {
      const uint32_t i = j + 1 + idx / m, c = j + 1 + idx % m;
      if (c <= i) A[tri(i, c)] -= A[tri(i, j)] * A[tri(c, j)];
    }
    sync();
  }
  for (uint32_t c = t; c < d; c += nt) {           // L^-1 by columns: worker c solves L y = e_c
    Li[tri(c, c)] = 1.0 / A[tri(c, c)];
    for (uint32_t i = c + 1; i < d; i++) {
      double s = 0;
      for (uint32_t m = c; m < i; m++) s += A[tri(i, m)] * Li[tri(m, c)];
      Li[tri(i, c)] = -s / A[tri(i, i)];
    }
  }
  sync();
}

// row i of T into row[0 .. i] and z_i, from the row's own stream
MSC_PRED_HD void niw_draw_row(uint64_t key, uint32_t k, uint64_t sweep, uint32_t tag, uint32_t i, uint32_t d, double nu_n,
                              double *row, double *z) {
  pred::Stream s(key, (uint64_t)(i + 1u) << 32 | k, sweep, tag);
  *z = s.normal();
  for (uint32_t j = 0; j < i; j++) row[j] = s.normal();
  row[i] = sqrt(pred::chi2(s, nu_n - (double)d + 1.0 + (double)i));
}

// row i of V = T L^-1 over row i of T, in place: V_ic = sum_{j = c .. i} T_ij Li_jc, c ascending (T_ic is last read
// for V_ic itself)
MSC_PRED_HD void niw_whiten_row(uint32_t i, double *row, const double *Li) {
  for (uint32_t c = 0; c <= i; c++) {
    double s = 0;
    for (uint32_t j = c; j <= i; j++) s += row[j] * Li[tri(j, c)];
    row[c] = s;
  }
}

// The whole draw of slot k.  Scratch: A, Li = packed triangles, mun, z, vmu, mean = [d]; all of it shared by the nt
// workers.  On return A holds V, mean mu, vmu V mu (every value finite); *c_out (worker 0's alone is set) the slice.
template <class Sync>
MSC_PRED_HD void draw_niw(uint32_t d, const float *hp, double n, const float *sx, const float *sxx, uint64_t key, uint32_t k,
                          uint64_t sweep, uint32_t tag, double *A, double *Li, double *mun, double *z, double *vmu,
                          double *mean, float *c_out, uint32_t t, uint32_t nt, Sync sync) {
  double kn, nun;
  niw_post(d, hp, n, sx, sxx, &kn, &nun, mun, A, t, nt, sync);
  niw_factor(d, A, Li, t, nt, sync);
  for (uint32_t i = t; i < d; i += nt) {           // (L is no longer read: T, then V, takes its place)
    double *row = A + tri(i, 0);
    niw_draw_row(key, k, sweep, tag, i, d, nun, row, &z[i]);
    niw_whiten_row(i, row, Li);
    for (uint32_t j = 0; j <= i; j++) row[j] = fin64(row[j]);
    if (!(row[i] > 1e-300)) row[i] = 1e-300;       // (the diagonal stays positive: its log is the slice)
    z[i] = fin64(z[i] / sqrt(kn));
    double b = 0;
    for (uint32_t j = 0; j <= i; j++) b += row[j] * mun[j];
    vmu[i] = fin64(b + z[i]);
  }
  sync();
  if (t == 0) {
    // mu - mu_n = V^-1 z / sqrt(kappa_n) by forward substitution, and the slice
    double ld = 0;
    for (uint32_t i = 0; i < d; i++) {
      const double *row = A + tri(i, 0);
      double s = z[i];
      for (uint32_t j = 0; j < i; j++) s -= row[j] * mean[j];
      mean[i] = s / row[i];
      ld += log(row[i]);
    }
    for (uint32_t i = 0; i < d; i++) mean[i] = fin64(mun[i] + mean[i]);
    *c_out = fin(-0.5 * (double)d * 1.8378770664093453 + ld);
  }
  sync();
}

}  // namespace blocked
}  // namespace msc
