// splitmerge_math.hpp -- the arithmetic of the split-merge Metropolis-Hastings move (msc_split_merge,
// kernels_splitmerge.hip; Jain & Neal 2004 / 2007 with an uncollapsed launch): the Philox key and streams, the anchors,
// the two-way label probabilities and the log acceptance ratio, as plain functions -- the host compiler builds the same
// code (tests/test_splitmerge_cpu.py holds it against the f64 oracle without a GPU).
//
// Streams.  Every random number of proposal p of a call is Philox-4x32-10 under a key made from seed ^ kSmKey:
//   stream_key(seed, s) = (seed ^ kSmKey) + s * kStreamStride          (mod 2^64)
// with the call's sweep counter sweep + p and, where a row is meant, its GLOBAL id row_id0 + offset in the counter:
//   s = kStreamProposal   darts uniform01(key, sweep + p, c), c = 0 .. 4: anchor i from darts 0 and 1, anchor j from
//                         darts 2 and 3 (pick_index: 48 bits each), the acceptance dart from c = 4
//   s = kStreamCoin       the initial label of a free row: uniform01(key, sweep + p, row id) >= 0.5 -> label 1
//   s = kStreamPass0 + t  pass t = 0 .. launch_iters (the last one gives theta* and the final labels):
//                         the parameters of pair slot k, feature f: pred::Stream(key, k, sweep + p, f), the stick fraction
//                         V_0 takes feature blocked::kStickTag -- the blocked sweep's draws (blocked_post.hpp) under this
//                         key; a free row's label dart: uniform01(key, sweep + p, row id), label 0 when dart < P(label 0)
// uniform01 is the sweep kernels' dart (score_block.hpp philox_uniform01, the oracle's uniform01): counter words
// (row, row >> 32, sweep, sweep >> 32), the first output word's top 24 bits.  A parameter stream's last counter word has
// its top bit set, a dart's has not (sweep < 2^63): under one key the two never meet.
#pragma once

#include "pred_samplers.hpp"

namespace msc {
namespace sm {

constexpr uint64_t kSmKey = 0xA0761D6478BD642Full;         // the move's key is seed ^ this (+ the stream's stride)
constexpr uint64_t kStreamStride = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kStreamProposal = 0, kStreamCoin = 1, kStreamPass0 = 2;
constexpr uint32_t kSplit = 0, kMerge = 1, kVoid = 2;      // a proposal's kind, as the log reports it
constexpr uint64_t kDartAnchorI = 0, kDartAnchorJ = 2, kDartAccept = 4;

MSC_PRED_HD uint64_t stream_key(uint64_t seed, uint32_t stream) { return (seed ^ kSmKey) + (uint64_t)stream * kStreamStride; }

MSC_PRED_HD float uniform01(uint64_t key, uint64_t sweep, uint64_t row) {
  const uint32_t k[2] = {(uint32_t)key, (uint32_t)(key >> 32)};
  const uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32)};
  uint32_t o[4];
  pred::philox4x32_10(k, c, o);
  return (float)(o[0] >> 8) * (1.0f / 16777216.0f);
}

// an index uniform over [0, n) from two darts: u = hi + lo 2^-24 carries 48 bits (n < 2^48)
MSC_PRED_HD uint64_t pick_index(float hi, float lo, uint64_t n) {
  const double u = (double)hi + (double)lo * (1.0 / 16777216.0);
  const uint64_t i = (uint64_t)(u * (double)n);
  return i < n ? i : n - 1;
}

// the ordered pair of distinct offsets (i, j), uniform over the n (n - 1) pairs (n >= 2)
MSC_PRED_HD void anchors(uint64_t key, uint64_t sweep, uint64_t n, uint64_t *i, uint64_t *j) {
  *i = pick_index(uniform01(key, sweep, kDartAnchorI), uniform01(key, sweep, kDartAnchorI + 1), n);
  const uint64_t t = pick_index(uniform01(key, sweep, kDartAnchorJ), uniform01(key, sweep, kDartAnchorJ + 1), n - 1);
  *j = t >= *i ? t + 1 : t;
}

MSC_PRED_HD float fast_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(x);
#else
  return expf(x);
#endif
}
MSC_PRED_HD float fast_log(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __logf(x);
#else
  return logf(x);
#endif
}

// log P(label 0), log P(label 1) and P(label 0) of a row with scores s0, s1 (finite): one exp, one log.  The larger
// score's log-probability is -log(1 + e), the smaller's -|d| - log(1 + e), e = exp(-|d|), d = s1 - s0: both finite at
// any gap, and their exponentials sum to one within rounding.
MSC_PRED_HD void two_way(float s0, float s1, float *lp0, float *lp1, float *p0) {
  const float d = s1 - s0, a = fabsf(d);
  const float e = fast_exp(-a);
  const float l = fast_log(1.0f + e);
  const float big = -l, small = -a - l;
  const float inv = 1.0f / (1.0f + e);
  const bool one = d > 0.0f;                               // slot 1 has the larger score
  *lp0 = one ? small : big;
  *lp1 = one ? big : small;
  *p0 = one ? e * inv : inv;
}

// the prior's part of a split's ratio: log alpha + lgamma(n0) + lgamma(n1) - lgamma(n0 + n1) (n0, n1 >= 1: each block
// holds its anchor)
MSC_PRED_HD double log_crp_split(double log_alpha, double n0, double n1) {
  return log_alpha + lgamma(n0) + lgamma(n1) - lgamma(n0 + n1);
}

// log A of a proposal: sd0, sd1, sdS = the sums over features of score_data of the two blocks and of their union,
// logq = the sum over free rows of log P(final label | theta*)
MSC_PRED_HD double log_accept(uint32_t kind, double log_alpha, double n0, double n1, double sd0, double sd1, double sdS,
                              double logq) {
  const double t = log_crp_split(log_alpha, n0, n1) + sd0 + sd1 - sdS;
  return kind == kSplit ? t - logq : -t + logq;
}

}  // namespace sm
}  // namespace msc
