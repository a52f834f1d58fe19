// lse_merge.hpp -- the reduction of msc_score_marginal (kernels_marginal.hip): log-sum-exp of a row's K totals with the
// arg-max on the way, as plain functions so that the host compiler builds the same arithmetic
// (tests/test_marginal_cpu.py checks it against scipy without a GPU).  Nothing here touches a state.
//
// A part is (m, s, k): m the largest value seen, s = sum exp(v - m) over the values seen, k the lowest index at which m
// was seen.  The empty part is (-inf, 0, 0).  Two ways to build a row's part, both used by the kernels:
//   online   a lane pushes its run of values one after the other (lse_push), the 64 lanes' parts are merged pairwise
//            (lse_merge): k_row_lse, whose lanes stride over a row of any length in memory;
//   two-pass the row's maximum first (every value is in registers), then every lane adds up exp(v - m) of its values
//            (lse_term) and the 64 sums are added pairwise: the fused kernels.
// Either way every exponent is <= 0 and the entries at the maximum contribute exactly 1, so s >= 1 for a row with a
// finite entry and nothing overflows; a row of -inf alone finishes as -inf with index 0, not NaN.
// Error: exp2 and log2 are within 1 ulp (v_exp_f32 / v_log_f32 on the device), a sum of n terms in (0, 1] formed as
// per-lane runs of r and a tree of depth 6 carries at most (r + 6) half-ulps of relative error, i.e. that much ABSOLUTE
// error in the logarithm: 1.3e-6 in the worst case for the longest fused run (16), typically the square root of it.
// k_row_lse's runs (K / 64 values, 128 at K = 8192) keep s in double for that reason; the fused kernels' stay in float.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MSC_LSE_HD __host__ __device__ inline
#else
#define MSC_LSE_HD inline
#endif

namespace msc {
namespace lse {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr double kLn2 = 0.69314718055994530942;

MSC_LSE_HD float exp2_fast(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x);
#else
  return std::exp2(x);
#endif
}
MSC_LSE_HD float log2_fast(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_logf(x);
#else
  return std::log2(x);
#endif
}
MSC_LSE_HD bool is_neg_inf(float v) { return v < 0.f && v - v != 0.f; }

// exp(v - m) for v <= m; m = -inf (a row of -inf alone) reads as 0 so that the difference is never inf - inf
MSC_LSE_HD float lse_term(float v, float m) { return exp2_fast((v - (is_neg_inf(m) ? 0.f : m)) * kLog2e); }

template <typename S>
struct Part {
  float m;
  S s;
  int32_t k;
};
template <typename S>
MSC_LSE_HD Part<S> lse_empty() { return Part<S>{-INFINITY, (S)0, 0}; }

// one more value, at index k (indices are pushed in ascending order: an equal value keeps the earlier index)
template <typename S>
MSC_LSE_HD void lse_push(Part<S> &p, float v, int32_t k) {
  if (v > p.m) {
    p.s = p.s * (S)lse_term(p.m, v) + (S)1;                // (from the empty part: 0 * exp2(-inf) + 1)
    p.m = v;
    p.k = k;
  } else if (!is_neg_inf(v)) {
    p.s += (S)lse_term(v, p.m);
  }
}
// a then b; on equal maxima the lower index wins whichever side holds it
template <typename S>
MSC_LSE_HD Part<S> lse_merge(const Part<S> &a, const Part<S> &b) {
  Part<S> r;
  r.m = a.m >= b.m ? a.m : b.m;
  r.k = a.m > b.m ? a.k : b.m > a.m ? b.k : (a.k <= b.k ? a.k : b.k);
  r.s = a.s * (S)lse_term(a.m, r.m) + b.s * (S)lse_term(b.m, r.m);
  return r;
}

// what a row's part becomes.  lse = m + log s, in double from the two float parts (one rounding, at the end); logp = lse -
// log_norm; logresp = m - lse = -log s, the log responsibility of the arg-max group (<= 0).
struct Result {
  float logp, logresp;
};
template <typename S>
MSC_LSE_HD Result lse_finish(float m, S s, double log_norm) {
  Result r;
  if (is_neg_inf(m) || !(s > (S)0)) {
    r.logp = -INFINITY;
    r.logresp = 0.f;
    return r;
  }
  const double ls = (double)log2_fast((float)s) * kLn2;
  r.logp = (float)(((double)m + ls) - log_norm);
  r.logresp = (float)(-ls);
  return r;
}

// ---- the fused kernels' chunking: a lane holds G consecutive entries of the row in registers ----
// a lane's part of one row: the maximum of its entries, sum exp(entry - that maximum), the lowest index of the maximum
// (kb = the index of t[0]; MAP = false leaves k at kb)
struct LanePart {
  float m, s;
  int32_t k;
};
template <int G, bool MAP>
MSC_LSE_HD LanePart lane_part(const float (&t)[G], int32_t kb) {
  LanePart p;
  p.m = t[0];
#pragma unroll
  for (int j = 1; j < G; j++) p.m = t[j] > p.m ? t[j] : p.m;
  const float mm = is_neg_inf(p.m) ? 0.f : p.m;            // (a lane beyond K holds -inf alone: its sum is 0, not NaN)
  p.s = 0.f;
#pragma unroll
  for (int j = 0; j < G; j++) p.s += exp2_fast((t[j] - mm) * kLog2e);
  p.k = kb;
  if (MAP) {
#pragma unroll
    for (int j = G - 1; j >= 0; j--) p.k = t[j] == p.m ? kb + j : p.k;
  }
  return p;
}
// what a lane hands to the wave's sum and to its arg-max once the row's maximum M is known
MSC_LSE_HD float lane_scaled_sum(const LanePart &p, float M) { return p.s * lse_term(p.m, M); }   // (at the maximum: times exactly 1)
MSC_LSE_HD int32_t lane_candidate(const LanePart &p, float M) { return p.m == M ? p.k : 0x7fffffff; }

}  // namespace lse
}  // namespace msc
