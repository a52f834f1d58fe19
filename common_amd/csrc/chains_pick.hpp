// chains_pick.hpp -- the two discrete draws of msc_chains_sample_predictive (kernels_chains_pred.hip) as plain functions,
// so that the host compiler builds the same arithmetic (tests/test_chains_predictive_cpu.py holds it to numpy without a
// GPU).  Nothing here touches a state.
//
// Both draws pick an index from unnormalised LOG terms a_0 .. a_{n-1} with one uniform u in (0, 1), everything in double:
//   M = max a_i,  e_i = exp(a_i - M) (0 for -inf),  S = sum e_i in ascending i;
//   the pick is the smallest i whose running sum e_0 + .. + e_i exceeds u S; if rounding lets none exceed it, the last i
//   with e_i > 0 (Running).
// The chain draw (pick_index) forms M, S and the running sum in three passes over the terms: the running sum repeats the
// additions of S.  It gives -1 -- the row is skipped -- when no term is finite or one is NaN or +inf.
// The group draw cannot afford its terms three times (each is a row's total against a group: a gather per feature), so
// its first pass forms (M, S) together (Online: S is rescaled when the maximum rises, the arithmetic of
// chains_merge.hpp's w_push) and its second pass the running sum against u S.  The two sums may differ in their last
// bits; the fallback covers the one case where that matters.
//
// The uniforms of global row R: one Philox4x32-10 block, key = seed ^ kPickKey, counter (R lo, R hi, sweep lo 32 bits,
// 0x80000000); u1 (the chain) from words (w0, w1), u2 (the group) from (w2, w3), each pred_samplers.hpp's two-word
// 53-bit uniform.
#pragma once

#include <cmath>
#include <cstdint>

#include "pred_samplers.hpp"

namespace msc {
namespace cpick {

constexpr uint64_t kPickKey = 0xC2B2AE3D27D4EB4Full;

MSC_PRED_HD double u53_of(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

MSC_PRED_HD void pick_words(uint64_t seed, uint64_t R, uint64_t sweep, uint32_t w[4]) {
  const uint64_t key64 = seed ^ kPickKey;
  const uint32_t key[2] = {(uint32_t)key64, (uint32_t)(key64 >> 32)};
  const uint32_t ctr[4] = {(uint32_t)R, (uint32_t)(R >> 32), (uint32_t)sweep, pred::kStreamTag};
  pred::philox4x32_10(key, ctr, w);
}
MSC_PRED_HD void pick_uniforms(uint64_t seed, uint64_t R, uint64_t sweep, double &u1, double &u2) {
  uint32_t w[4];
  pick_words(seed, R, sweep, w);
  u1 = u53_of(w[0], w[1]);
  u2 = u53_of(w[2], w[3]);
}

MSC_PRED_HD bool neg_inf(double v) { return v < 0.0 && v - v != 0.0; }
MSC_PRED_HD bool nan_or_pos_inf(double v) { return v != v || (v > 0.0 && v - v != 0.0); }
// exp(a - M), exactly 0 for a term of -inf (also against M = -inf, where a - M is NaN)
MSC_PRED_HD double term(double a, double M) { return neg_inf(a) ? 0.0 : exp(a - M); }

// the running sum against a target: push the e_i in ascending i, then result()
struct Running {
  double acc;
  int32_t hit, last;     // the first i whose running sum exceeded the target; the last i with e_i > 0 (-1: none yet)
};
MSC_PRED_HD Running running_start() { return Running{0.0, -1, -1}; }
MSC_PRED_HD void running_push(Running &r, int32_t i, double e, double target) {
  r.acc += e;
  if (e > 0.0) r.last = i;
  if (r.hit < 0 && r.acc > target) r.hit = i;
}
MSC_PRED_HD int32_t running_result(const Running &r) { return r.hit >= 0 ? r.hit : r.last; }

// (M, S) in one pass
struct Online {
  double M, S;
};
MSC_PRED_HD Online online_start() { return Online{-(double)INFINITY, 0.0}; }
MSC_PRED_HD void online_push(Online &p, double a) {
  if (neg_inf(a)) return;
  if (a > p.M) {
    p.S = p.S * exp(p.M - a) + 1.0;                          // (from the start: 0 * exp(-inf) + 1)
    p.M = a;
  } else {
    p.S += exp(a - p.M);
  }
}

// the chain draw: a(i) gives term i (called three times per i, ascending)
template <class F>
MSC_PRED_HD int32_t pick_index(uint32_t n, double u, F a) {
  double M = -(double)INFINITY;
  bool bad = false;
  for (uint32_t i = 0; i < n; i++) {
    const double v = a(i);
    bad |= nan_or_pos_inf(v);
    M = v > M ? v : M;
  }
  if (bad || neg_inf(M)) return -1;
  double S = 0.0;
  for (uint32_t i = 0; i < n; i++) S += term(a(i), M);
  const double target = u * S;
  Running r = running_start();
  for (uint32_t i = 0; i < n; i++) running_push(r, (int32_t)i, term(a(i), M), target);
  return running_result(r);
}

}  // namespace cpick
}  // namespace msc
