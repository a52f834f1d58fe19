// Host build of common_amd/csrc/pred_samplers.hpp for tests/test_predictive_cpu.py: the generators the predictive
// kernels run, driven from ctypes.  Draw i of a batch reads the stream of (seed, row = i, sweep = 0, feature = 0).
#include <cstdint>

#include "pred_samplers.hpp"

using namespace msc::pred;

extern "C" {

void pred_philox(const uint32_t *key, const uint32_t *ctr, uint32_t *out) { philox4x32_10(key, ctr, out); }

// the first n words of the stream of one entry
void pred_stream_words(uint64_t seed, uint64_t row, uint64_t sweep, uint32_t feature, uint32_t n, uint32_t *out) {
  Stream s(seed, row, sweep, feature);
  for (uint32_t i = 0; i < n; i++) out[i] = s.next();
}

// kind: 0 Gamma(a, 1), 1 Beta(a, b), 2 chi2(a), 3 Student-t(a), 4 Poisson(a), 5 standard normal, 6 u53
void pred_draw(int kind, double a, double b, uint64_t n, uint64_t seed, double *out) {
  for (uint64_t i = 0; i < n; i++) {
    Stream s(seed, i, 0, 0);
    switch (kind) {
      case 0: out[i] = gamma1(s, a); break;
      case 1: out[i] = beta(s, a, b); break;
      case 2: out[i] = chi2(s, a); break;
      case 3: out[i] = student_t(s, a); break;
      case 4: out[i] = (double)poisson(s, a); break;
      case 5: out[i] = s.normal(); break;
      default: out[i] = s.u53(); break;
    }
  }
}
}
