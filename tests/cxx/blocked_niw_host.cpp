// Host build of common_amd/csrc/blocked_niw.hpp for tests/test_blocked_niw_cpu.py and tests/test_gpu_blocked_niw.py: the
// posterior and the parameter draw of the blocked Gibbs sampler's niw feature, driven from ctypes.  Draw i of a batch
// reads the streams of (seed ^ kKey, slot = slot0 + i, sweep, tag), as that slot of a device draw with that seed does.
#include <cstdint>
#include <vector>

#include "blocked_niw.hpp"

using namespace msc;
using namespace msc::blocked;

extern "C" {

uint32_t niw_max_dim() { return kNiwMaxDim; }

// out = {kappa_n, nu_n, mu_n[d], Psi_n[d][d] (both triangles)}
void niw_post_host(uint32_t d, const float *hp, double n, const float *sx, const float *sxx, double *out) {
  std::vector<double> A(ntri(d));
  niw_post(d, hp, n, sx, sxx, &out[0], &out[1], out + 2, A.data(), 0u, 1u, NoSync());
  for (uint32_t i = 0; i < d; i++)
    for (uint32_t j = 0; j <= i; j++) out[2 + d + i * d + j] = out[2 + d + j * d + i] = A[tri(i, j)];
}

// nslots draws from one slot's (hp, suff-stats): mean = double[nslots][d], whiten = double[nslots][d (d + 1) / 2] (packed
// lower triangle of V), vmu = double[nslots][d], c = float[nslots]
void niw_draw_host(uint32_t d, const float *hp, double n, const float *sx, const float *sxx, uint32_t slot0, uint32_t nslots,
                   uint64_t seed, uint64_t sweep, uint32_t tag, double *mean, double *whiten, double *vmu, float *c) {
  const uint64_t key = seed ^ kKey;
  const size_t nt = ntri(d);
  std::vector<double> Li(nt), mun(d), z(d);
  for (uint32_t i = 0; i < nslots; i++)
    draw_niw(d, hp, n, sx, sxx, key, slot0 + i, sweep, tag, whiten + i * nt, Li.data(), mun.data(), z.data(), vmu + (size_t)i * d,
             mean + (size_t)i * d, c + i, 0u, 1u, NoSync());
}
}
