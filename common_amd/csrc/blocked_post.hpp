// blocked_post.hpp -- the blocked (uncollapsed) Gibbs sampler's parameter draws (msc_blocked_draw, kernels_blocked.hip):
// the map from (hyper-parameters, a slot's suff-stats) to the conjugate posterior's parameters, and the draw of the slices
// the assign kernels read, as plain functions over the variate generators of pred_samplers.hpp -- the host compiler builds
// the same code (tests/test_blocked_cpu.py checks posterior and draws against scipy without a GPU).
//
// Streams: key = seed ^ kKey; one stream per (slot, feature): pred::Stream(seed ^ kKey, slot, sweep, feature), the stick
// weight of a slot takes feature tag kStickTag.  Nothing else enters a counter, so two states with equal tables draw
// bit-identical parameters.
//
// Slices (float32, stored [slice][kpad]; every stored value finite, fin()):
//   bb    {log(1 - p), log p}                     p ~ Beta(alpha + heads, beta + tails)
//   gp    {-lambda, log lambda}                   lambda ~ Gamma(alpha + sum, rate inv_beta + count)
//   bnb   {r log p, log(1 - p)}                   p ~ Beta(alpha + r count, beta + sum)
//   dd    {log theta_i, i < dim}                  theta ~ Dirichlet(alpha_i + c_i)
//   nich  {-log(2 pi sigma^2) / 2, mu, -1 / (2 sigma^2)}   sigma^2 = nu' sigma'^2 / chi2(nu'), mu ~ N(mu', sigma^2 / kappa')
#pragma once

#include "pred_samplers.hpp"

namespace msc {
namespace blocked {

constexpr uint64_t kKey = 0x9FB21C651E98DF25ull;   // the parameter draws' key is seed ^ this
constexpr uint32_t kStickTag = 0x7fffu;
constexpr float kLogFloor = -1e28f;                // what the log of 0 is stored as (x 2^32 counts stays finite in float)

// a stored table value: finite, whatever the draw underflowed or overflowed to
MSC_PRED_HD float fin(double v) {
  if (!(v > (double)kLogFloor)) return kLogFloor;  // (-inf, NaN)
  if (v > 1e28) return 1e28f;
  return (float)v;
}

// the largest L1 distance between the marginal density under K slots and under the Dirichlet process (Ishwaran & James,
// JASA 2001, theorem 2): 4 N exp(-(K - 1) / alpha)
MSC_PRED_HD double truncation_bound(double nrows, uint32_t K, double alpha) {
  return 4.0 * nrows * exp(-((double)K - 1.0) / alpha);
}

// X ~ Beta(a, b) as the logs of X and 1 - X: neither rounds to log(0) while the gammas are positive
MSC_PRED_HD void log_beta_pair(pred::Stream &s, double a, double b, double *log_x, double *log_1mx) {
  const double x = pred::gamma1(s, a), y = pred::gamma1(s, b);
  const double lt = log(x + y);
  *log_x = log(x) - lt;
  *log_1mx = log(y) - lt;
}

// ---- stick weights: V_k ~ Beta(1 + n_k, alpha + sum_{l > k} n_l), V_{K-1} = 1 ----
MSC_PRED_HD void stick_post(double n_k, double n_after, double alpha, double *a, double *b) {
  *a = 1.0 + n_k;
  *b = alpha + n_after;
}
MSC_PRED_HD void draw_stick(pred::Stream &s, double a, double b, bool last, double *log_v, double *log_1mv) {
  if (last) { *log_v = 0.0; *log_1mv = (double)kLogFloor; return; }
  log_beta_pair(s, a, b, log_v, log_1mv);
  if (!(*log_v > (double)kLogFloor)) *log_v = (double)kLogFloor;
  if (!(*log_1mv > (double)kLogFloor)) *log_1mv = (double)kLogFloor;
}

// ---- bb ----
MSC_PRED_HD void bb_post(const float *hp, double heads, double tails, double *a, double *b) {
  *a = (double)hp[0] + heads;
  *b = (double)hp[1] + tails;
}
MSC_PRED_HD void draw_bb(pred::Stream &s, double a, double b, float *out, size_t stride) {
  double lp, lq;
  log_beta_pair(s, a, b, &lp, &lq);
  out[0] = fin(lq);
  out[stride] = fin(lp);
}

// ---- gp ----
MSC_PRED_HD void gp_post(const float *hp, double count, double sum, double *shape, double *rate) {
  *shape = (double)hp[0] + sum;
  *rate = (double)hp[1] + count;
}
MSC_PRED_HD void draw_gp(pred::Stream &s, double shape, double rate, float *out, size_t stride) {
  const double lam = pred::gamma1(s, shape) / rate;
  out[0] = fin(-lam);
  out[stride] = fin(log(lam));
}

// ---- bnb: v ~ NB(r, p), p ~ Beta(alpha, beta); pmf C(v + r - 1, v) p^r (1 - p)^v ----
MSC_PRED_HD void bnb_post(const float *hp, double count, double sum, double *a, double *b) {
  *a = (double)hp[0] + (double)hp[2] * count;
  *b = (double)hp[1] + sum;
}
MSC_PRED_HD void draw_bnb(pred::Stream &s, double a, double b, double r, float *out, size_t stride) {
  double lp, lq;
  log_beta_pair(s, a, b, &lp, &lq);
  out[0] = fin(r * lp);
  out[stride] = fin(lq);
}

// ---- nich: hp {mu, kappa, sigmasq, nu}, suff-stats {count, mean, count_times_variance} ----
MSC_PRED_HD void nich_post(const float *hp, double n, double mean, double ctv, double *mu_n, double *kappa_n,
                           double *sigmasq_n, double *nu_n) {
  const double mu = hp[0], kappa = hp[1], sigmasq = hp[2], nu = hp[3];
  const double kn = kappa + n, nun = nu + n, dm = mu - mean;
  *mu_n = (kappa * mu + n * mean) / kn;
  *kappa_n = kn;
  *nu_n = nun;
  *sigmasq_n = (nu * sigmasq + ctv + n * kappa * dm * dm / kn) / nun;
}
// -> sigma^2, mu (out: the three slices)
MSC_PRED_HD void draw_nich(pred::Stream &s, double mu_n, double kappa_n, double sigmasq_n, double nu_n, float *out,
                           size_t stride, double *sigmasq_out = nullptr, double *mu_out = nullptr) {
  const double sig2 = nu_n * sigmasq_n / pred::chi2(s, nu_n);
  const double mu = mu_n + sqrt(sig2 / kappa_n) * s.normal();
  out[0] = fin(-0.5 * log(6.283185307179586 * sig2));
  out[stride] = fin(mu);
  out[2 * stride] = fin(-0.5 / sig2);
  if (sigmasq_out) *sigmasq_out = sig2;
  if (mu_out) *mu_out = mu;
}

// ---- dd: dim gammas from one stream in value order, normalised in double (the stream is replayed for the logs) ----
MSC_PRED_HD void draw_dd(uint64_t key, uint64_t slot, uint64_t sweep, uint32_t tag, uint32_t dim, const float *hp,
                         const uint32_t *counts, size_t counts_stride, float *out, size_t stride) {
  double tot = 0.0;
  {
    pred::Stream s(key, slot, sweep, tag);
    for (uint32_t i = 0; i < dim; i++) tot += pred::gamma1(s, (double)hp[i] + (double)counts[i * counts_stride]);
  }
  const double lt = log(tot);
  pred::Stream s(key, slot, sweep, tag);
  for (uint32_t i = 0; i < dim; i++)
    out[i * stride] = fin(log(pred::gamma1(s, (double)hp[i] + (double)counts[i * counts_stride])) - lt);
}

}  // namespace blocked
}  // namespace msc
