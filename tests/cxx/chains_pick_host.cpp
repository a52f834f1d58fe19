// Host build of common_amd/csrc/chains_pick.hpp for tests/test_chains_predictive_cpu.py: the two discrete draws of
// msc_chains_sample_predictive and their Philox block, as the kernels call them, driven from ctypes.
#include <cstdint>

#include "chains_pick.hpp"

using namespace msc::cpick;

extern "C" {

// the block of (seed, global row id, sweep): its four words, and the two uniforms taken from them
void cp_words(uint64_t seed, uint64_t R, uint64_t sweep, uint32_t *w) { pick_words(seed, R, sweep, w); }
void cp_uniforms(uint64_t seed, uint64_t R, uint64_t sweep, double *u) { pick_uniforms(seed, R, sweep, u[0], u[1]); }

// the chain draw over n terms (k_chains_pick's call)
int32_t cp_pick(const double *a, uint32_t n, double u) {
  return pick_index(n, u, [=](uint32_t i) { return a[i]; });
}

// the group draw over K float totals as k_chains_draw takes it: (max, sum) online, then the running sum; -1 where the
// kernel skips the row
int32_t cp_group(const float *t, uint32_t K, double u) {
  Online on = online_start();
  for (uint32_t k = 0; k < K; k++) online_push(on, (double)t[k]);
  if (neg_inf(on.M) || !(on.S > 0.0)) return -1;
  const double target = u * on.S;
  Running run = running_start();
  for (uint32_t k = 0; k < K && run.hit < 0; k++) running_push(run, (int32_t)k, term((double)t[k], on.M), target);
  return running_result(run);
}

}
