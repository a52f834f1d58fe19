// kernels_hp.hip -- gfx950 kernels of grid hyper-parameter inference (msc_hp_grid_*, include/microscopes_hip.h):
//   k_hp_grid_score   per (grid, point, group block): sum over the counted slots of score_data(hp = point, group) in double
//   k_hp_grid_reduce  the group blocks' partial sums of a point, added in block order
//   k_crp_grid_score  score_assignment(alpha) of the group counts for every alpha of a grid (group_manager.hpp:207-218)
//   k_hp_grid_draw    one wave per grid: prior + likelihood, softmax, a Philox dart, the chosen block into the device hp
// The hp is held PER LANE (lane <-> grid point) and the groups stream past as LDS broadcasts: the per-group formulas are
// family_math.hpp's *_score_data (through its hp_eval), the ones k_score_data evaluates with one hp per feature.  Every
// sum runs in a fixed order (slots in index order inside a block, blocks in order, lanes' chunks in lane order): no
// atomics, so two calls on the same tables give the same bits, and so do the ranks of a sharded sweep.
#include "family_math.hpp"
#include "launchers.hpp"
#include "score_block.hpp"

namespace msc {

constexpr int kHpPoints = 256;                     // grid points of a workgroup, one per lane
constexpr int kHpSlots = 64;                       // group slots staged in LDS at a time
constexpr int kHpRows = 1 + (int)kMaxDDDim;        // raw table rows a family has at most (dd: count_sum + 128 counts)

// grid (point blocks, group blocks, grids).  Group block y covers slots [y * per_blk, (y + 1) * per_blk) of [0, K); a slot
// counts when slots[k] != 0 (a caller's mask) or, without a mask, when its group count is not zero; no other slot is read.
__global__ __launch_bounds__(kHpPoints) void k_hp_grid_score(const HpJob *__restrict__ jobs, uint32_t K, uint32_t kpad,
                                                             const uint32_t *__restrict__ cnt,
                                                             const uint8_t *__restrict__ slots, uint32_t per_blk,
                                                             double *__restrict__ part) {
  __shared__ uint32_t tab[kHpRows * kHpSlots];
  __shared__ uint32_t idx[kHpSlots];
  __shared__ uint32_t nidx;
  const HpJob &J = jobs[blockIdx.z];
  const uint32_t G = J.npoints;
  if (blockIdx.x * kHpPoints >= G) return;          // (the launch is sized for the largest grid)
  const uint32_t p = blockIdx.x * kHpPoints + threadIdx.x;
  const bool live = p < G;
  const float *hp = J.grid + (size_t)(live ? p : G - 1) * J.hpf;   // (a dead lane evaluates a real point, stores nothing)
  float h[4];                                       // the scalar families' blocks, in registers
#pragma unroll
  for (int i = 0; i < 4; i++) h[i] = (uint32_t)i < J.hpf ? hp[i] : 0.f;
  const int family = J.family;
  const uint32_t rows = J.nu32 + J.nf32;
  const uint32_t s0 = blockIdx.y * per_blk, s1 = min(K, s0 + per_blk);
  const uint32_t *su = tab;
  const float *sf = reinterpret_cast<const float *>(tab + (size_t)J.nu32 * kHpSlots);
  double acc = 0.0;
  for (uint32_t c0 = s0; c0 < s1; c0 += kHpSlots) {
    __syncthreads();                                // (the previous block is consumed)
    if (threadIdx.x < kHpSlots) {                   // wave 0 lists the counted slots of the block, in index order
      const uint32_t k = c0 + threadIdx.x;
      const bool counted = k < s1 && (slots ? slots[k] != 0 : cnt[k] != 0u);
      const uint64_t b = __ballot(counted);
      if (counted) idx[__popcll(b & ((1ull << threadIdx.x) - 1ull))] = k;
      if (threadIdx.x == 0) nidx = (uint32_t)__popcll(b);
    }
    __syncthreads();
    const uint32_t n = nidx;
    for (uint32_t e = threadIdx.x; e < rows * n; e += kHpPoints) {
      const uint32_t r = e / n, j = e - r * n, k = idx[j];
      tab[r * kHpSlots + j] = r < J.nu32 ? J.raw_u32[(size_t)r * kpad + k]
                                         : __float_as_uint(J.raw_f32[(size_t)(r - J.nu32) * kpad + k]);
    }
    __syncthreads();
    for (uint32_t j = 0; j < n; j++) acc += hp_eval(family, J.dim, h, hp, su, sf, j, kHpSlots);
  }
  if (live) part[J.part_off + (size_t)blockIdx.y * G + p] = acc;
}

// grid (point blocks, grids): out[point] = the point's partial sums, group block 0 first
__global__ __launch_bounds__(256) void k_hp_grid_reduce(const HpJob *__restrict__ jobs, uint32_t nblk,
                                                        const double *__restrict__ part, double *__restrict__ out) {
  const HpJob &J = jobs[blockIdx.y];
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= J.npoints) return;
  double s = 0.0;
  for (uint32_t b = 0; b < nblk; b++) s += part[J.part_off + (size_t)b * J.npoints + p];
  out[J.out_off + p] = s;
}

// score_assignment(alpha) = K_occ ln alpha + sum_k lgamma(n_k) + lgamma(alpha) - lgamma(N + alpha) over the non-zero counts.
// Every workgroup reduces the counts the same way (strided partials, then a fixed LDS tree), then scores its points.
__global__ __launch_bounds__(256) void k_crp_grid_score(const HpJob *__restrict__ job, const uint32_t *__restrict__ cnt,
                                                        uint32_t K, double *__restrict__ out) {
  __shared__ double lg[256];
  __shared__ unsigned long long nn[256];
  __shared__ uint32_t occ[256];
  double l = 0.0;
  unsigned long long n = 0;
  uint32_t o = 0;
  for (uint32_t k = threadIdx.x; k < K; k += 256) {
    const uint32_t c = cnt[k];
    if (c) {
      l += lgamma((double)c);
      n += c;
      o++;
    }
  }
  lg[threadIdx.x] = l;
  nn[threadIdx.x] = n;
  occ[threadIdx.x] = o;
  for (uint32_t w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) {
      lg[threadIdx.x] += lg[threadIdx.x + w];
      nn[threadIdx.x] += nn[threadIdx.x + w];
      occ[threadIdx.x] += occ[threadIdx.x + w];
    }
  }
  __syncthreads();
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= job->npoints) return;
  const double a = job->grid[p];
  out[job->out_off + p] = (double)occ[0] * log(a) + lg[0] + lgamma(a) - lgamma((double)nn[0] + a);
}

// One wave per grid.  s_g = likelihood + prior; p_g = exp(s_g - max s); the CDF is taken in index order as lane chunks --
// lane l owns points [l per, (l + 1) per), sums its p_g in order, the chunk sums are prefixed in lane order -- and the
// point drawn is the first g with CDF_g > u * total, u = Philox(seed, sweep, stream).  The chosen block is copied into the
// feature's device hp (and, dd / dm, its alpha sum into the descriptor) right here; chosen[grid] = the index, or npoints
// when no point has a finite positive weight (nothing is installed then).
__global__ __launch_bounds__(64) void k_hp_grid_draw(const HpJob *__restrict__ jobs, const double *__restrict__ scores,
                                                     uint64_t seed, uint64_t sweep, uint32_t *__restrict__ chosen) {
  __shared__ double pre[kWave + 1];
  __shared__ uint32_t pick;
  const HpJob &J = jobs[blockIdx.x];
  const uint32_t G = J.npoints, lane = threadIdx.x;
  const uint32_t per = (G + kWave - 1) / kWave;
  const uint32_t g0 = min(G, lane * per), g1 = min(G, g0 + per);
  const double *lik = scores + J.out_off;
  double m = -INFINITY;
  for (uint32_t g = g0; g < g1; g++) {
    const double s = lik[g] + (J.logprior ? J.logprior[g] : 0.0);
    if (J.scores_out) J.scores_out[g] = s;
    m = fmax(m, s);
  }
  for (int off = kWave / 2; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  double c = 0.0;
  for (uint32_t g = g0; g < g1; g++) c += exp(lik[g] + (J.logprior ? J.logprior[g] : 0.0) - m);
  pre[lane + 1] = c;
  if (lane == 0) pick = G;
  __syncthreads();
  if (lane == 0) {
    double t = 0.0;
    for (int l = 0; l < kWave; l++) {
      const double cl = pre[l + 1];
      pre[l] = t;
      t += cl;
    }
    pre[kWave] = t;
  }
  __syncthreads();
  const double total = pre[kWave];
  const double u = (double)philox_uniform01(seed, sweep, J.stream) * total;
  if (total > 0.0 && total < INFINITY && pre[lane] <= u && u < pre[lane + 1]) {   // exactly one lane's chunk holds the dart
    double r = 0.0;
    uint32_t at = g1 - 1;
    for (uint32_t g = g0; g < g1; g++) {
      r += exp(lik[g] + (J.logprior ? J.logprior[g] : 0.0) - m);
      if (pre[lane] + r > u) {
        at = g;
        break;
      }
    }
    pick = at;
  }
  __syncthreads();
  const uint32_t k = pick;
  if (lane == 0) chosen[blockIdx.x] = k;
  if (k >= G || J.hp_dst == nullptr) return;
  const float *src = J.grid + (size_t)k * J.hpf;
  for (uint32_t i = lane; i < J.hpf; i += kWave) J.hp_dst[i] = src[i];
  if (lane == 0 && J.aux_dst) {                      // (msc_state_set_hp's sum: the block's floats in order, in double)
    double asum = 0.0;
    for (uint32_t i = 0; i < J.hpf; i++) asum += (double)src[i];
    *J.aux_dst = asum;
  }
}

int launch_hp_grid_score(hipStream_t stream, const HpJob *jobs_dev, uint32_t njobs, uint32_t max_points, uint32_t K,
                         uint32_t kpad, const uint32_t *cnt, const uint8_t *slots, uint32_t nblk, double *part,
                         double *out) {
  const uint32_t pblk = (max_points + kHpPoints - 1) / kHpPoints;
  const uint32_t per_blk = (((K + nblk - 1) / nblk) + kHpSlots - 1) / kHpSlots * kHpSlots;
  hipLaunchKernelGGL(k_hp_grid_score, dim3(pblk, nblk, njobs), dim3(kHpPoints), 0, stream, jobs_dev, K, kpad, cnt, slots,
                     per_blk, part);
  hipLaunchKernelGGL(k_hp_grid_reduce, dim3((max_points + 255) / 256, njobs), dim3(256), 0, stream, jobs_dev, nblk, part,
                     out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_crp_grid_score(hipStream_t stream, const HpJob *job_dev, uint32_t npoints, const uint32_t *cnt, uint32_t K,
                          double *out) {
  hipLaunchKernelGGL(k_crp_grid_score, dim3((npoints + 255) / 256), dim3(256), 0, stream, job_dev, cnt, K, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_hp_grid_draw(hipStream_t stream, const HpJob *jobs_dev, uint32_t njobs, const double *scores, uint64_t seed,
                        uint64_t sweep, uint32_t *chosen) {
  hipLaunchKernelGGL(k_hp_grid_draw, dim3(njobs), dim3(kWave), 0, stream, jobs_dev, scores, seed, sweep, chosen);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
