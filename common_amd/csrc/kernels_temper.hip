// kernels_temper.hip -- gfx950 kernels of a tempered ensemble's two steps between sweeps (msc_chains_exchange /
// msc_chains_anneal_weights, include/microscopes_hip.h).
//   k_chains_exchange        one thread per ladder of nrungs chains: the neighbouring rung pairs of this parity are
//                            proposed in rung order and an accepted pair swaps its two chains' beta and rung entries
//   k_chains_anneal_weights  one thread per chain: logw[c] += (beta_to[c] - beta_from[c]) L_c
// Both read the chains' joint rows as k_chains_score_joint left them and do their arithmetic in double through
// temper_math.hpp, the functions the host restatement is built from.  A ladder is walked by ONE thread, so the pairs of a
// ladder are decided one after another, no two threads write one entry, and the result does not depend on the launch's
// shape.  The work is a few dozen doubles a ladder: the launch, not the kernel, is what an exchange costs.
// The device error word (device_error.hpp) reaches k_chains_exchange as an ARGUMENT, not through a copy of the pointer
// bound into this unit: the call has the context at hand, and nothing has to be bound before the first launch.
#include "device_error.hpp"
#include "launchers.hpp"
#include "score_block.hpp"
#include "temper_math.hpp"

namespace msc {

constexpr int kTemperThreads = 64;

// the uniform of the pair (j, j + 1) of a ladder: philox_uniform01(seed, sweep, ladder * nrungs + j)
struct PairUniform {
  uint64_t seed, sweep, at;
  MSC_DEV float operator()(uint32_t j) const { return philox_uniform01(seed, sweep, at + j); }
};

__global__ __launch_bounds__(kTemperThreads) void k_chains_exchange(uint32_t nladders, uint32_t nfeat,
                                                                    const double *__restrict__ joint, uint64_t ld_joint,
                                                                    uint32_t nrungs, float *beta, int32_t *rung,
                                                                    uint64_t parity, uint64_t seed, uint64_t sweep,
                                                                    uint32_t *proposed, uint32_t *accepted,
                                                                    uint32_t *err_word) {
  const uint32_t l = blockIdx.x * kTemperThreads + threadIdx.x;
  if (l >= nladders) return;
  const size_t c0 = (size_t)l * nrungs, p0 = (size_t)l * temper::ladder_pairs(nrungs);
  const PairUniform u01 = {seed, sweep, (uint64_t)c0};
  if (!temper::exchange_ladder(joint + c0 * ld_joint, ld_joint, nfeat, nrungs, beta + c0, rung + c0, parity, u01,
                               proposed + p0, accepted + p0) &&
      err_word != nullptr) {
    // report_device_error's protocol on the word handed in: code BITS, the detail stays the first error's
    const uint32_t before = __hip_atomic_fetch_or(err_word, (uint32_t)MSC_DEVERR_TEMPER, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
    if (before == 0u) __hip_atomic_store(err_word + 1, l, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(kTemperThreads) void k_chains_anneal_weights(uint32_t nchains, uint32_t nfeat,
                                                                          const double *__restrict__ joint,
                                                                          uint64_t ld_joint,
                                                                          const float *__restrict__ beta_from,
                                                                          const float *__restrict__ beta_to, double *logw) {
  const uint32_t c = blockIdx.x * kTemperThreads + threadIdx.x;
  if (c >= nchains) return;
  double w = logw[c];
  if (temper::anneal_step(beta_from[c], beta_to[c], temper::chain_loglik(joint + (size_t)c * ld_joint, nfeat), &w)) logw[c] = w;
}

int launch_chains_exchange(hipStream_t stream, uint32_t nchains, uint32_t nfeat, const double *joint, uint64_t ld_joint,
                           uint32_t nrungs, float *beta, int32_t *rung, uint64_t parity, uint64_t seed, uint64_t sweep,
                           uint32_t *proposed, uint32_t *accepted, uint32_t *err_word_dev) {
  const uint32_t nladders = nchains / nrungs;
  hipLaunchKernelGGL(k_chains_exchange, dim3((nladders + kTemperThreads - 1) / kTemperThreads), dim3(kTemperThreads), 0,
                     stream, nladders, nfeat, joint, ld_joint, nrungs, beta, rung, parity, seed, sweep, proposed, accepted,
                     err_word_dev);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_chains_anneal_weights(hipStream_t stream, uint32_t nchains, uint32_t nfeat, const double *joint, uint64_t ld_joint,
                                 const float *beta_from, const float *beta_to, double *logw) {
  hipLaunchKernelGGL(k_chains_anneal_weights, dim3((nchains + kTemperThreads - 1) / kTemperThreads), dim3(kTemperThreads), 0,
                     stream, nchains, nfeat, joint, ld_joint, beta_from, beta_to, logw);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
