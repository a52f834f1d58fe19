// Host build of common_amd/csrc/lse_merge.hpp for tests/test_marginal_cpu.py: a row's log-sum-exp and arg-max in the two
// chunkings the kernels of msc_score_marginal use, driven from ctypes.
#include <cstdint>
#include <vector>

#include "lse_merge.hpp"

using namespace msc::lse;

extern "C" {

// mode 0 (k_row_lse): lane l pushes the entries 4 l + 256 i .. + 3 in ascending order (the sum in double), the 64 parts
// are merged pairwise, the lower lanes' first.
// mode 1 (the fused kernels, G = 1 .. 16 entries a lane, K <= 1024): lane l forms the part of entries G l .. G l + G - 1
// (lane_part, the kernels' own), the wave takes the maximum of the 64, scales every lane's sum to it and adds them pairwise; the
// arg-max is the lowest index over the lanes at the maximum.
void lse_row(int mode, const float *v, uint32_t K, double log_norm, float *logp, int32_t *map, float *logresp) {
  if (mode == 0) {
    Part<double> lane[64];
    for (int l = 0; l < 64; l++) {
      lane[l] = lse_empty<double>();
      for (uint32_t k = 4u * l; k < K; k += 256u)
        for (uint32_t j = k; j < K && j < k + 4; j++) lse_push(lane[l], v[j], (int32_t)j);
    }
    for (int off = 1; off < 64; off <<= 1)
      for (int l = 0; l < 64; l += 2 * off) lane[l] = lse_merge(lane[l], lane[l + off]);
    const Result r = lse_finish<double>(lane[0].m, lane[0].s, log_norm);
    *logp = r.logp, *map = lane[0].k, *logresp = r.logresp;
    return;
  }
  const uint32_t G = K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;   // (the launcher's choice)
  LanePart part[64];
  float M = -INFINITY;
  for (uint32_t l = 0; l < 64; l++) {
    float t[16];
    for (uint32_t j = 0; j < 16; j++) t[j] = j < G && G * l + j < K ? v[G * l + j] : -INFINITY;
    switch (G) {
      case 1: part[l] = lane_part<1, true>(reinterpret_cast<const float(&)[1]>(t), (int32_t)(G * l)); break;
      case 2: part[l] = lane_part<2, true>(reinterpret_cast<const float(&)[2]>(t), (int32_t)(G * l)); break;
      case 4: part[l] = lane_part<4, true>(reinterpret_cast<const float(&)[4]>(t), (int32_t)(G * l)); break;
      case 8: part[l] = lane_part<8, true>(reinterpret_cast<const float(&)[8]>(t), (int32_t)(G * l)); break;
      default: part[l] = lane_part<16, true>(t, (int32_t)(G * l)); break;
    }
    M = part[l].m > M ? part[l].m : M;
  }
  float s[64];
  int32_t best = 0x7fffffff;
  for (int l = 0; l < 64; l++) {
    s[l] = lane_scaled_sum(part[l], M);
    const int32_t c = lane_candidate(part[l], M);
    best = c < best ? c : best;
  }
  for (int off = 1; off < 64; off <<= 1)
    for (int l = 0; l < 64; l += 2 * off) s[l] += s[l + off];
  const Result r = lse_finish<float>(M, s[0], log_norm);
  *logp = r.logp, *map = is_neg_inf(M) ? 0 : best, *logresp = r.logresp;
}

}
