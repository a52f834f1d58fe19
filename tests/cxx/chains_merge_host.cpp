// Host build of common_amd/csrc/chains_merge.hpp for tests/test_chains_marginal_cpu.py: the reductions of
// msc_chains_score_marginal in the order the kernels take them, driven from ctypes.
#include <cstdint>
#include <vector>

#include "chains_merge.hpp"

using namespace msc::cmerge;

extern "C" {

// lw[n] = logw[n] - logsumexp(logw) by the header's own runs and tree steps, called as k_chains_marginal_prep calls them
// (a loop over t where the kernel has its threads and a barrier)
void cm_weights(const double *logw, uint32_t n, double *lw) {
  double red[kWRuns];
  bool bad = false;
  for (unsigned t = 0; t < kWRuns; t++) red[t] = w_run_max(logw, n, t, bad);
  for (unsigned o = kWRuns / 2; o > 0; o >>= 1)
    for (unsigned t = 0; t < kWRuns; t++) w_tree_step<true>(red, t, o);
  const double big = red[0];
  for (unsigned t = 0; t < kWRuns; t++) red[t] = w_run_sum(logw, n, t, big);
  for (unsigned o = kWRuns / 2; o > 0; o >>= 1)
    for (unsigned t = 0; t < kWRuns; t++) w_tree_step<false>(red, t, o);
  for (uint32_t i = 0; i < n; i++) lw[i] = w_normalised(logw[i], big, red[0], bad);
}

// mix of one row: the chains' terms lw[c] + L[c], chains cut into nslices slices of ceil(n / nslices) consecutive chains
// (the launcher's cut), each slice pushed in ascending chain order, the slices merged in ascending slice order
float cm_mix(const double *lw, const double *L, uint32_t n, uint32_t nslices) {
  const uint32_t per = (n + nslices - 1) / nslices;
  WPart all = w_empty();
  for (uint32_t s = 0; s < nslices; s++) {
    WPart w = w_empty();
    for (uint32_t c = s * per; c < n && c < (s + 1) * per; c++) w_push(w, lw[c] + L[c]);
    if (nslices == 1) return w_finish(w);
    all = w_merge(all, w);
  }
  return w_finish(all);
}

// the merge of explicit parts, in the order given
float cm_merge_parts(const double *M, const double *S, uint32_t n) {
  WPart all = w_empty();
  for (uint32_t i = 0; i < n; i++) all = w_merge(all, WPart{M[i], S[i]});
  return w_finish(all);
}

// L of one chain's row: the K totals pushed in batches of 8 (a short last batch padded with -inf), finished in double
double cm_row(const float *t, uint32_t K, double log_norm) {
  RowPart p = row_empty();
  for (uint32_t k0 = 0; k0 < K; k0 += 8) {
    float b[8];
    for (uint32_t j = 0; j < 8; j++) b[j] = k0 + j < K ? t[k0 + j] : -INFINITY;
    row_push(p, b);
  }
  return row_logp(p, log_norm);
}

}
