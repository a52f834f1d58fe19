// kernels_joint.hip -- gfx950 kernels of the log joint log p(X, z | hp, alpha) of a state, or of every chain of an
// ensemble (msc_score_joint / msc_chains_score_joint / msc_chains_keep_best, include/microscopes_hip.h):
//   k_score_joint          one workgroup: the row of nfeatures + 3 doubles of one state (the layout: joint_math.hpp)
//   k_chains_score_joint   the same body on a grid of chains, workgroup c on chain c's tables and row
//   k_joint_priors, k_chains_joint_priors   the hyper-prior entries past the first launch's kJointCoords, added to the
//                          row's p in entry order; the total is then added up again from the row
//   k_chains_keep_best     one workgroup per chain: where the chain's total beats its best, its z row is kept
// One body, two kernels (as k_hp_slice / k_hp_slice_chains): a chain does the arithmetic of the single-state call on its
// state in the same order, whatever the width of the launch, so the two calls give the same bits.  The order of every sum:
//   a     score_assignment(alpha) as k_crp_grid_score and the slice target's alpha branch write it: thread t sums
//         lgamma(n_k), n_k and the occupied slots over k = t, t + 256, ... in ascending order, the 256 partials fold in an
//         LDS tree (t += t + w for w = 128, 64, ..., 1), then occ ln alpha + lg + lgamma(alpha) - lgamma(N + alpha);
//   d_f   thread t sums hp_eval over the counted slots k = t, t + 256, ... in ascending order, a wave folds its 64
//         partials by xor butterflies (offsets 32, 16, ..., 1), the four waves' sums are added (w0 + w1) + (w2 + w3);
//   p     one thread, the entries in the caller's order from 0.0;
//   [0]   joint_math.hpp joint_total.
// Everything in double, no atomics.  Slots are read in place from the raw tables, each once; a slot that is not counted is
// not read.  The scalar families' hp blocks sit in registers, dd / dm read their alphas in place.
#include "family_math.hpp"
#include "joint_math.hpp"
#include "launchers.hpp"

namespace msc {

constexpr int kJointThreads = 256;
constexpr int kJointWaves = kJointThreads / kWave;
static_assert(kJointWaves == 4, "score_joint_body adds four wave partials");

// this thread's part of d_f, in slot order
template <int FAM>
MSC_DEV double joint_pass(const FeatDesc *fd, uint32_t K, uint32_t kpad, const uint32_t *__restrict__ cnt,
                          const uint8_t *__restrict__ slots) {
  constexpr uint32_t hpf = FAM == MSC_NICH ? 4u : FAM == MSC_BNB ? 3u : (FAM == MSC_DD || FAM == MSC_DM) ? 0u : 2u;
  const float *hp = fd->hp;
  float h[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (uint32_t i = 0; i < hpf; i++) h[i] = hp[i];
  const uint32_t *su = fd->raw_u32;
  const float *sf = fd->raw_f32;
  const uint32_t dim = fd->dim;
  double acc = 0.0;
  for (uint32_t k = threadIdx.x; k < K; k += kJointThreads) {
    if (!(slots ? slots[k] != 0 : cnt[k] != 0u)) continue;
    acc += hp_eval(FAM, dim, h, hp, su, sf, k, kpad);
  }
  return acc;
}

// the value an entry's prior is taken at, and its partner's: floats of the device hp blocks (or alpha), widened
MSC_DEV double joint_prior_term(const FeatDesc *feats, float alpha, const JointCoord &c) {
  if (c.feature == MSC_HP_CLUSTER) return slice_log_prior(c.prior, (double)alpha, (double)c.prior_a, (double)c.prior_b, 0.0);
  const float *hp = feats[c.feature].hp;
  return slice_log_prior(c.prior, (double)hp[c.coord], (double)c.prior_a, (double)c.prior_b, (double)hp[c.partner]);
}

// One state, one workgroup.  cs: entries [0, n) of the call, n <= kJointCoords.
MSC_DEV void score_joint_body(const FeatDesc *__restrict__ feats, uint32_t nfeat, uint32_t K, uint32_t kpad,
                              const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ slots, float alpha,
                              const JointCoords &cs, uint32_t n, double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double lg_s[kJointThreads];
  __shared__ unsigned long long nn_s[kJointThreads];
  __shared__ uint32_t occ_s[kJointThreads];
  __shared__ double wred[kJointWaves];
  // a: the group counts' part as k_crp_grid_score reduces it, then the alpha branch of the slice target
  double l = 0.0;
  unsigned long long nn = 0;
  uint32_t o = 0;
  for (uint32_t k = threadIdx.x; k < K; k += kJointThreads) {
    const uint32_t c = cnt[k];
    if (c) {
      l += lgamma((double)c);
      nn += c;
      o++;
    }
  }
  lg_s[threadIdx.x] = l;
  nn_s[threadIdx.x] = nn;
  occ_s[threadIdx.x] = o;
  for (uint32_t w = kJointThreads / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) {
      lg_s[threadIdx.x] += lg_s[threadIdx.x + w];
      nn_s[threadIdx.x] += nn_s[threadIdx.x + w];
      occ_s[threadIdx.x] += occ_s[threadIdx.x + w];
    }
  }
  __syncthreads();
  const double x = (double)alpha;
  const double a = (double)occ_s[0] * log(x) + lg_s[0] + lgamma(x) - lgamma((double)nn_s[0] + x);
  if (threadIdx.x == 0) out[joint::kJointAssign] = a;
  double total = a;
  for (uint32_t f = 0; f < nfeat; f++) {
    const FeatDesc *fd = feats + f;
    double acc = 0.0;
    switch (fd->family) {                            // (the same for every thread: no barrier is skipped)
      case MSC_BB: acc = joint_pass<MSC_BB>(fd, K, kpad, cnt, slots); break;
      case MSC_BBNC: acc = joint_pass<MSC_BBNC>(fd, K, kpad, cnt, slots); break;
      case MSC_GP: acc = joint_pass<MSC_GP>(fd, K, kpad, cnt, slots); break;
      case MSC_BNB: acc = joint_pass<MSC_BNB>(fd, K, kpad, cnt, slots); break;
      case MSC_NICH: acc = joint_pass<MSC_NICH>(fd, K, kpad, cnt, slots); break;
      case MSC_DD: acc = joint_pass<MSC_DD>(fd, K, kpad, cnt, slots); break;
      case MSC_DM: acc = joint_pass<MSC_DM>(fd, K, kpad, cnt, slots); break;
      default: break;                                // noop: 0 (niw never gets here: the entry points refuse it)
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    __syncthreads();                                 // (the feature before has been read)
    if ((threadIdx.x & (kWave - 1)) == 0) wred[threadIdx.x / kWave] = acc;
    __syncthreads();
    const double d = (wred[0] + wred[1]) + (wred[2] + wred[3]);
    if (threadIdx.x == 0) out[joint::kJointData + f] = d;
    total = total + d;                               // joint_total's order
  }
  if (threadIdx.x == 0) {
    double p = 0.0;
    for (uint32_t i = 0; i < n; i++) p += joint_prior_term(feats, alpha, cs.e[i]);
    out[joint::joint_prior_at(nfeat)] = p;
    out[joint::kJointTotal] = total + p;
  }
}

// entries past the first launch's: p goes on in entry order, the total is added up again from the row
MSC_DEV void joint_priors_body(const FeatDesc *__restrict__ feats, uint32_t nfeat, float alpha, const JointCoords &cs,
                               uint32_t n, double *out) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  double p = out[joint::joint_prior_at(nfeat)];
  for (uint32_t i = 0; i < n; i++) p += joint_prior_term(feats, alpha, cs.e[i]);
  out[joint::joint_prior_at(nfeat)] = p;
  out[joint::kJointTotal] = joint::joint_total(out, nfeat);
}

__global__ __launch_bounds__(kJointThreads) void k_score_joint(const FeatDesc *__restrict__ feats, uint32_t nfeat, uint32_t K,
                                                               uint32_t kpad, const uint32_t *__restrict__ cnt,
                                                               const uint8_t *__restrict__ slots, float alpha,
                                                               JointCoords cs, uint32_t n, double *__restrict__ out) {
  score_joint_body(feats, nfeat, K, kpad, cnt, slots, alpha, cs, n, out);
}

// grid (chains), block kJointThreads: workgroup c takes chain c
__global__ __launch_bounds__(kJointThreads) void k_chains_score_joint(const JointChain *__restrict__ chains, uint32_t nfeat,
                                                                      uint32_t K, uint32_t kpad, JointCoords cs, uint32_t n) {
  const JointChain &C = chains[blockIdx.x];
  score_joint_body(C.feats, nfeat, K, kpad, C.cnt, C.slots, C.alpha, cs, n, C.out);
}

__global__ __launch_bounds__(kWave) void k_joint_priors(const FeatDesc *__restrict__ feats, uint32_t nfeat, float alpha,
                                                        JointCoords cs, uint32_t n, double *out) {
  joint_priors_body(feats, nfeat, alpha, cs, n, out);
}

__global__ __launch_bounds__(kWave) void k_chains_joint_priors(const JointChain *__restrict__ chains, uint32_t nfeat,
                                                               JointCoords cs, uint32_t n) {
  const JointChain &C = chains[blockIdx.x];
  joint_priors_body(C.feats, nfeat, C.alpha, cs, n, C.out);
}

// grid (chains), block 256.  A chain has ONE workgroup, and every thread of it has compared against best[c] before one
// of them rewrites it.
__global__ __launch_bounds__(256) void k_chains_keep_best(const double *__restrict__ joint, uint64_t ld_joint,
                                                          const int32_t *__restrict__ z, uint64_t ld_z, uint64_t nrows,
                                                          int64_t iter, double *best, int32_t *__restrict__ best_z,
                                                          uint64_t ld_best, int64_t *__restrict__ best_iter) {
  const size_t c = blockIdx.x;
  const double j = joint[c * ld_joint];
  const bool wins = joint::keep_best_wins(j, best[c]);
  __syncthreads();
  if (!wins) return;
  const int32_t *src = z + c * ld_z;
  int32_t *dst = best_z + c * ld_best;
  for (uint64_t i = threadIdx.x; i < nrows; i += 256) dst[i] = src[i];
  if (threadIdx.x == 0) {
    best[c] = j;
    best_iter[c] = iter;
  }
}

static JointCoords joint_chunk(const JointCoord *coords, uint32_t at, uint32_t n) {
  JointCoords cs = {};
  for (uint32_t i = 0; i < n; i++) cs.e[i] = coords[at + i];
  return cs;
}

int launch_score_joint(hipStream_t stream, const FeatDesc *feats_dev, uint32_t nfeat, uint32_t K, uint32_t kpad,
                       const uint32_t *cnt, const uint8_t *slots, float alpha, const JointCoord *coords, uint32_t n,
                       double *out) {
  const uint32_t n0 = std::min(n, kJointCoords);
  hipLaunchKernelGGL(k_score_joint, dim3(1), dim3(kJointThreads), 0, stream, feats_dev, nfeat, K, kpad, cnt, slots, alpha,
                     joint_chunk(coords, 0, n0), n0, out);
  for (uint32_t at = n0; at < n; at += kJointCoords) {
    const uint32_t m = std::min(n - at, kJointCoords);
    hipLaunchKernelGGL(k_joint_priors, dim3(1), dim3(kWave), 0, stream, feats_dev, nfeat, alpha, joint_chunk(coords, at, m), m,
                       out);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_chains_score_joint(hipStream_t stream, const JointChain *chains_dev, uint32_t nchains, uint32_t nfeat, uint32_t K,
                              uint32_t kpad, const JointCoord *coords, uint32_t n) {
  const uint32_t n0 = std::min(n, kJointCoords);
  hipLaunchKernelGGL(k_chains_score_joint, dim3(nchains), dim3(kJointThreads), 0, stream, chains_dev, nfeat, K, kpad,
                     joint_chunk(coords, 0, n0), n0);
  for (uint32_t at = n0; at < n; at += kJointCoords) {
    const uint32_t m = std::min(n - at, kJointCoords);
    hipLaunchKernelGGL(k_chains_joint_priors, dim3(nchains), dim3(kWave), 0, stream, chains_dev, nfeat,
                       joint_chunk(coords, at, m), m);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_chains_keep_best(hipStream_t stream, uint32_t nchains, const double *joint, uint64_t ld_joint, const int32_t *z,
                            uint64_t ld_z, uint64_t nrows, int64_t iter, double *best, int32_t *best_z, uint64_t ld_best,
                            int64_t *best_iter) {
  hipLaunchKernelGGL(k_chains_keep_best, dim3(nchains), dim3(256), 0, stream, joint, ld_joint, z, ld_z, nrows, iter, best,
                     best_z, ld_best, best_iter);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
