// chains_merge.hpp -- the reductions of msc_chains_score_marginal (kernels_chains_marginal.hip) as plain functions, so
// that the host compiler builds the same arithmetic (tests/test_chains_marginal_cpu.py holds it to scipy without a GPU).
// Nothing here touches a state.
//
// Two reductions, one inside the other:
//   over the groups of ONE chain   a lane walks the K totals t[k] of its row in ascending batches of G (row_push): the
//                                  running maximum m in float, s = sum exp(t - m) in double (a run is K entries long; a
//                                  batch rescales s at most once).  row_logp finishes L = m + log s - log(n + alpha) in
//                                  double, the logarithm as lse_merge.hpp's lse_finish takes it.
//   over the chains of one row     the terms u_c = lw_c + L_c, all in double, in ASCENDING chain order (w_push): (M, S)
//                                  with S = sum exp(u - M).  A term of -inf (a chain of weight -inf, or a row no group of
//                                  the chain can hold) adds nothing.  When the chains are cut into slices, every slice
//                                  forms its own (M, S) over its chains and the slices are merged in ascending slice order
//                                  (w_merge, a then b); w_finish rounds M + log S to float once.
// The empty part is (-inf, 0) and finishes as -inf.  A single finite term u finishes as (float)u exactly -- S is exactly
// 1, and merging with empty parts multiplies it by exp(0) -- which is what makes a one-hot weight vector reproduce its
// chain's row bit for bit.  A NaN term (the weights held nothing finite) makes S, and so the result, NaN.
#pragma once

#include <cmath>

#include "lse_merge.hpp"

namespace msc {
namespace cmerge {

MSC_LSE_HD bool neg_inf(double v) { return v < 0.0 && v - v != 0.0; }

// ---- one chain: the K totals of a row ----
struct RowPart {
  float m;    // the largest total seen
  double s;   // sum exp(t - m) over the totals seen
};
MSC_LSE_HD RowPart row_empty() { return RowPart{-INFINITY, 0.0}; }

template <int G>
MSC_LSE_HD void row_push(RowPart &p, const float (&t)[G]) {
  float bm = t[0];
#pragma unroll
  for (int j = 1; j < G; j++) bm = t[j] > bm ? t[j] : bm;
  if (bm > p.m) {
    p.s *= (double)lse::lse_term(p.m, bm);                 // (from the empty part: 0 * exp2(-inf))
    p.m = bm;
  }
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < G; j++) e += lse::lse_term(t[j], p.m);   // (a batch of -inf alone against m = -inf: exp2(-inf) = 0 each)
  p.s += (double)e;
}

// L = m + log s - log_norm in double; -inf for a row no group can hold
MSC_LSE_HD double row_logp(const RowPart &p, double log_norm) {
  if (lse::is_neg_inf(p.m) || !(p.s > 0.0)) return -(double)INFINITY;
  return ((double)p.m + (double)lse::log2_fast((float)p.s) * lse::kLn2) - log_norm;
}

// ---- one row: the chains' weighted terms ----
struct WPart {
  double M, S;
};
MSC_LSE_HD WPart w_empty() { return WPart{-(double)INFINITY, 0.0}; }

MSC_LSE_HD void w_push(WPart &p, double u) {
  if (neg_inf(u)) return;
  if (u > p.M) {
    p.S = p.S * exp(p.M - u) + 1.0;                        // (from the empty part: 0 * exp(-inf) + 1)
    p.M = u;
  } else {
    p.S += exp(u - p.M);                                   // (NaN lands here and stays)
  }
}

// a then b
MSC_LSE_HD WPart w_merge(const WPart &a, const WPart &b) {
  WPart r;
  r.M = a.M >= b.M ? a.M : b.M;
  if (neg_inf(r.M)) {
    r.S = a.S + b.S;                                       // (0, or the NaN one of them carries)
    return r;
  }
  r.S = a.S * exp(a.M - r.M) + b.S * exp(b.M - r.M);
  return r;
}

MSC_LSE_HD float w_finish(const WPart &p) {
  if (p.S == 0.0) return -INFINITY;
  return (float)(p.M + log(p.S));
}

// ---- the weights: lw_c = logw_c - logsumexp(logw), or NaN for all when logw holds nothing finite to normalise by (no
// entry above -inf, a NaN, or +inf).  `big` = max logw, `sum` = sum exp(logw - big).
// The order in which big and sum are formed, as k_chains_marginal_prep and the host test both take it from here: kWRuns
// runs, run t over the entries t, t + kWRuns, ... in ascending order (w_run_max, then w_run_sum against the maximum of
// all), the kWRuns results in red[] folded by w_tree_step for o = kWRuns / 2, ..., 1 -- every t < o, then a barrier (the
// host: a loop over t) -- which leaves the result in red[0].
constexpr unsigned kWRuns = 256;
MSC_LSE_HD double w_run_max(const double *logw, unsigned n, unsigned t, bool &bad) {
  double big = -(double)INFINITY;
  for (unsigned i = t; i < n; i += kWRuns) {
    const double v = logw[i];
    bad |= v != v || (v > 0.0 && v - v != 0.0);            // NaN, +inf
    big = v > big ? v : big;
  }
  return big;
}
MSC_LSE_HD double w_run_sum(const double *logw, unsigned n, unsigned t, double big) {
  double sum = 0.0;
  if (!neg_inf(big))
    for (unsigned i = t; i < n; i += kWRuns) sum += exp(logw[i] - big);
  return sum;
}
template <bool MAX>
MSC_LSE_HD void w_tree_step(double *red, unsigned t, unsigned o) {
  if (t >= o) return;
  if (MAX) red[t] = red[t + o] > red[t] ? red[t + o] : red[t];
  else red[t] += red[t + o];
}
MSC_LSE_HD double w_normalised(double logw, double big, double sum, bool bad) {
  if (bad || neg_inf(big)) return NAN;
  return logw - (big + log(sum));
}

}  // namespace cmerge
}  // namespace msc
