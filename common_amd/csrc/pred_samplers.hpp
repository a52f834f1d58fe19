// pred_samplers.hpp -- the variate generators of the posterior predictive draws (msc_sample_predictive,
// kernels_pred.hip), written as plain functions of Philox-4x32-10 words so that the host compiler builds the same code
// (tests/test_predictive_cpu.py checks it against scipy without a GPU).  Nothing here touches a state.
//
// The stream of one drawn entry (row, feature): key = seed, counter block b =
//   c0 = row, c1 = row >> 32, c2 = sweep (low 32 bits), c3 = 0x80000000 | (feature & 0x7fff) << 16 | b
// and its words are taken in order, w0 .. w3 of block 0, then of block 1, ...  A sweep's dart (score_block.hpp
// philox_uniform01) has c3 = sweep >> 32 < 2^31 and the hp grid draw's the same: no draw here shares a counter with them.
//   one-uniform draws (bb, bbnc, dd):    u = (w0 >> 8) 2^-24 of block 0
//   every other uniform:                 two consecutive words a, b: u = ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53, in (0, 1)
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MSC_PRED_HD __host__ __device__ inline
#else
#define MSC_PRED_HD inline
#endif

namespace msc {
namespace pred {

constexpr uint32_t kStreamTag = 0x80000000u;
constexpr int kMaxTries = 64;          // rejection loops: attempts before the last candidate is taken (P(all fail) < 1e-60)
constexpr double kPtrsFrom = 10.0;     // Poisson: inversion below this rate, PTRS from it on

MSC_PRED_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Philox-4x32-10 (Salmon et al. SC'11), the rounds of score_block.hpp philox_uniform01, all four words out
MSC_PRED_HD void philox4x32_10(const uint32_t key[2], const uint32_t ctr[4], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; r++) {
    const uint32_t h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the word stream of one entry (see the header comment)
struct Stream {
  // (scalars, not arrays: a dynamically indexed array of a lane would be moved to LDS or scratch)
  uint32_t k0, k1, c0, c1, c2, c3;
  uint32_t w0, w1, w2, w3;
  uint32_t block, pos;
  bool has_spare;
  double spare;
  MSC_PRED_HD Stream(uint64_t seed, uint64_t row, uint64_t sweep, uint32_t feature)
      : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), c0((uint32_t)row), c1((uint32_t)(row >> 32)),
        c2((uint32_t)sweep), c3(kStreamTag | (feature & 0x7fffu) << 16), w0(0), w1(0), w2(0), w3(0), block(0), pos(4),
        has_spare(false), spare(0.0) {}
  MSC_PRED_HD uint32_t next() {
    if (pos == 4) {
      const uint32_t key[2] = {k0, k1}, c[4] = {c0, c1, c2, c3 | (block & 0xffffu)};
      uint32_t o[4];
      philox4x32_10(key, c, o);
      w0 = o[0]; w1 = o[1]; w2 = o[2]; w3 = o[3];
      block++;
      pos = 0;
    }
    const uint32_t p = pos++;
    return p == 0 ? w0 : p == 1 ? w1 : p == 2 ? w2 : w3;
  }
  // the one-uniform draws' u: first word, 24 bits (what the sweep's dart keeps)
  MSC_PRED_HD double u24() { return (double)(next() >> 8) * (1.0 / 16777216.0); }
  MSC_PRED_HD double u53() {
    const uint32_t a = next(), b = next();
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
  }
  // Box-Muller: two uniforms, two normals (the second is kept for the next call)
  MSC_PRED_HD double normal() {
    if (has_spare) { has_spare = false; return spare; }
    const double u = u53(), v = u53();
    const double r = sqrt(-2.0 * log(u)), t = 6.283185307179586 * v;
    spare = r * sin(t);
    has_spare = true;
    return r * cos(t);
  }
};

// Gamma(shape, 1): Marsaglia-Tsang (ACM TOMS 26, 2000), with the u^(1/shape) boost below shape 1
MSC_PRED_HD double gamma1(Stream &s, double shape) {
  double boost = 1.0;
  if (shape < 1.0) {
    boost = exp(log(s.u53()) / shape);
    shape += 1.0;
  }
  const double d = shape - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double out = d;
  for (int t = 0; t < kMaxTries; t++) {
    const double x = s.normal();
    double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    out = d * v;
    const double u = s.u53(), x2 = x * x;
    if (u < 1.0 - 0.0331 * x2 * x2) break;
    if (log(u) < 0.5 * x2 + d * (1.0 - v + log(v))) break;
  }
  return out * boost;
}

MSC_PRED_HD double beta(Stream &s, double a, double b) {
  const double x = gamma1(s, a), y = gamma1(s, b);
  return x / (x + y);
}
MSC_PRED_HD double chi2(Stream &s, double dof) { return 2.0 * gamma1(s, 0.5 * dof); }
MSC_PRED_HD double student_t(Stream &s, double nu) {
  const double z = s.normal();
  return z / sqrt(chi2(s, nu) / nu);
}

// Poisson(lam): inversion below kPtrsFrom, PTRS (Hormann, Insurance Math. Econom. 12, 1993) from it on
MSC_PRED_HD uint32_t poisson(Stream &s, double lam) {
  if (!(lam > 0.0)) return 0u;
  if (!(lam < 4294967295.0)) return 0xffffffffu;    // (an infinite rate, e.g. a bnb Beta draw at 0: the largest count)
  if (lam < kPtrsFrom) {
    double p = exp(-lam), u = s.u53();
    uint32_t k = 0;
    while (u > p && k < 1000u) {
      u -= p;
      k++;
      p *= lam / (double)k;
    }
    return k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  double k = floor(lam);
  for (int t = 0; t < kMaxTries; t++) {
    const double U = s.u53() - 0.5, V = s.u53(), us = 0.5 - fabs(U);
    k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) break;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) break;
  }
  if (k < 0.0) k = 0.0;
  return k >= 4294967295.0 ? 0xffffffffu : (uint32_t)k;
}

}  // namespace pred
}  // namespace msc
