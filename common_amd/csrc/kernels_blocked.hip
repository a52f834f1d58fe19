// kernels_blocked.hip -- gfx950 kernels of the blocked (uncollapsed) Gibbs sampler for the truncated stick-breaking
// mixture (msc_blocked_*, include/microscopes_hip.h; Ishwaran & James, JASA 2001):
//   k_blocked_sticks    one workgroup: V_k ~ Beta(1 + n_k, alpha + sum_{l > k} n_l) for every slot, then
//                       log pi_k = log V_k + sum_{l < k} log(1 - V_l), summed in slot order in double
//   k_blocked_draw      one thread per (feature, slot): the slot's parameters from their conjugate posterior, stored as
//                       the float slices the assign kernels read (blocked_post.hpp); a thread's work is
//                       blocked_draw.hpp's blk_draw_slot, as a slot's stick draw is its blk_stick_slot: k_sm_chains
//                       (kernels_chains_sm.hip) calls the same two
//   k_blocked_assign    lane <-> row: s_k = log pi_k + sum_f loglik_f(x_rf | slot k) over all slots, eight slots at a
//                       time with the slots' slices as wave-uniform operands; pass 1 keeps an online max and sum of exp,
//                       pass 2 recomputes the scores and walks the CDF to u sum.  No cross-lane work.
//                       <MODE_NICH1>  a single nich column: the row's value in a register
//                       <MODE_STAGED> the workgroup's row values staged once in LDS as [feature][row] codes
//                       <MODE_GLOBAL> any feature count: the codes re-read from the columns
//   k_blocked_top_slot  the highest occupied slot
// The row's value codes and the scores of eight slots (blk_code, blk_tile_scores) are blocked_score.hpp's, shared with
// the split-merge move.
#include "blocked_draw.hpp"
#include "blocked_post.hpp"
#include "blocked_score.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "score_block.hpp"

namespace msc {

constexpr uint32_t kStickChunk = 1024;

// ---- the draws -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blocked_sticks(const uint32_t *__restrict__ cnt, uint32_t K, float alpha,
                                                         uint64_t key, uint64_t sweep, double *__restrict__ work,
                                                         float *__restrict__ logw) {
  __shared__ double sh[kStickChunk];
  __shared__ double carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0.0;
  // from the last chunk to the first: the members of the slots after each one (exact in double below 2^53)
  for (int64_t c0 = (int64_t)((K - 1) / kStickChunk) * kStickChunk; c0 >= 0; c0 -= kStickChunk) {
    const uint32_t n = (uint32_t)(K - c0 < kStickChunk ? K - c0 : kStickChunk);
    for (uint32_t i = t; i < n; i += blockDim.x) sh[i] = (double)cnt[c0 + i];
    __syncthreads();
    if (t == 0) {
      double run = carry;
      for (uint32_t i = n; i-- > 0;) {
        const double c = sh[i];
        sh[i] = run;
        run += c;
      }
      carry = run;
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += blockDim.x) {
      const uint32_t k = (uint32_t)c0 + i;
      double lv, l1;
      blk_stick_slot((double)cnt[k], sh[i], (double)alpha, key, k, sweep, k + 1 == K, &lv, &l1);
      work[k] = lv;
      work[(size_t)K + k] = l1;
    }
    __syncthreads();
  }
  if (t == 0) carry = 0.0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < K; c0 += kStickChunk) {
    const uint32_t n = K - c0 < kStickChunk ? K - c0 : kStickChunk;
    for (uint32_t i = t; i < n; i += blockDim.x) sh[i] = work[(size_t)K + c0 + i];
    __syncthreads();
    if (t == 0) {
      double run = carry;
      for (uint32_t i = 0; i < n; i++) {
        const double v = sh[i];
        sh[i] = run;
        run += v;
      }
      carry = run;
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += blockDim.x) logw[c0 + i] = blocked::fin(work[c0 + i] + sh[i]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_blocked_draw(const BlkFeat *__restrict__ fs, uint32_t K, uint32_t kpad,
                                                      uint64_t key, uint64_t sweep, float *__restrict__ tab) {
  const BlkFeat &bf = fs[blockIdx.y];
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K || bf.nslices == 0) return;
  blk_draw_slot(bf, k, kpad, key, sweep, tab);
}

__global__ __launch_bounds__(256) void k_blocked_top_slot(const uint32_t *__restrict__ cnt, uint32_t K,
                                                           uint32_t *__restrict__ out) {
  __shared__ uint32_t top;
  if (threadIdx.x == 0) top = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t k = threadIdx.x; k < K; k += blockDim.x)
    if (cnt[k] != 0) mine = k;
  if (mine) atomicMax(&top, mine);
  __syncthreads();
  if (threadIdx.x == 0) *out = top;
}

// ---- the assignment --------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_blocked_assign(const BlkFeat *__restrict__ fs, int nfeat,
                                                         const float *__restrict__ tab, uint32_t K, uint32_t kpad,
                                                         uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                                         int32_t *__restrict__ z, uint64_t seed, uint64_t sweep) {
  extern __shared__ uint32_t blk_codes[];          // MODE_STAGED: [nfeat][blockDim.x]
  const uint32_t B = blockDim.x;
  const uint64_t r = (uint64_t)blockIdx.x * B + threadIdx.x;
  const bool has_row = r < nrows;
  const uint64_t vrow = row0 + (has_row ? r : 0);  // (a lane without a row scores row0's values and stores nothing)
  uint32_t code1 = kBlkMasked;
  if (MODE == MODE_STAGED) {
    for (int f = 0; f < nfeat; f++) blk_codes[(size_t)f * B + threadIdx.x] = blk_code(fs[f], vrow);
    // (every lane reads back its own column only: no barrier)
  } else if (MODE == MODE_NICH1) {
    code1 = blk_code(fs[0], vrow);
  }
  const uint32_t *codes = blk_codes + threadIdx.x;
  // pass 1: online max and sum of exp (the max is kept finite: a score that overflowed to -inf then adds exp(-inf) = 0)
  float m = -INFINITY, S = 0.f;
  for (uint32_t k0 = 0; k0 < K; k0 += kBlkTile) {
    float s[kBlkTile];
    blk_tile_scores<MODE>(fs, nfeat, tab, kpad, k0, codes, B, vrow, code1, s);
    float tm = m;
#pragma unroll
    for (int j = 0; j < kBlkTile; j++) tm = k0 + j < K ? fmaxf(tm, s[j]) : tm;
    tm = fmaxf(tm, -3.0e38f);
    float add = 0.f;
#pragma unroll
    for (int j = 0; j < kBlkTile; j++) add += k0 + j < K ? __expf(s[j] - tm) : 0.f;
    S = S * __expf(m - tm) + add;                  // (m = -inf at the first tile: exp gives 0)
    m = tm;
  }
  // pass 2: the first slot whose running sum reaches u S = the number of slots whose running sum stays below it
  const float t = philox_uniform01(seed, sweep, row_id0 + r) * S;
  float acc = 0.f;
  uint32_t pick = 0;
  for (uint32_t k0 = 0; k0 < K; k0 += kBlkTile) {
    float s[kBlkTile];
    blk_tile_scores<MODE>(fs, nfeat, tab, kpad, k0, codes, B, vrow, code1, s);
#pragma unroll
    for (int j = 0; j < kBlkTile; j++) {
      if (k0 + j < K) {
        acc += __expf(s[j] - m);
        pick += acc < t ? 1u : 0u;
      }
    }
    if (__all(!(acc < t))) break;                  // (wave-uniform: every lane of the wave has its slot)
  }
  if (pick >= K) {
    // rounding left the last sum short of u S (pass 1 summed in another order): the last slot that added anything
    pick = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += kBlkTile) {
      float s[kBlkTile];
      blk_tile_scores<MODE>(fs, nfeat, tab, kpad, k0, codes, B, vrow, code1, s);
#pragma unroll
      for (int j = 0; j < kBlkTile; j++)
        if (k0 + j < K && __expf(s[j] - m) > 0.f) pick = k0 + j;
    }
  }
  if (has_row) z[r] = (int32_t)pick;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int launch_blocked_draw(hipStream_t stream, const BlkFeat *fs_dev, uint32_t nfeat, uint32_t K, uint32_t kpad,
                        const uint32_t *cnt, float alpha, uint64_t seed, uint64_t sweep, double *work, float *tab) {
  const uint64_t key = seed ^ blocked::kKey;
  hipLaunchKernelGGL(k_blocked_sticks, dim3(1), dim3(256), 0, stream, cnt, K, alpha, key, sweep, work, tab);
  if (nfeat)
    hipLaunchKernelGGL(k_blocked_draw, dim3((K + 63) / 64, nfeat), dim3(64), 0, stream, fs_dev, K, kpad, key, sweep, tab);
  return launch_status("k_blocked_draw");
}

int launch_blocked_assign(hipStream_t stream, BlockedKernel kernel, uint32_t block, const BlkFeat *fs_dev, int nfeat,
                          const float *tab, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                          int32_t *z, uint64_t seed, uint64_t sweep) {
  if (nrows == 0) return 0;
  const dim3 grid((unsigned)((nrows + block - 1) / block));
  switch (kernel) {
    case BlockedKernel::nich1:
      hipLaunchKernelGGL((k_blocked_assign<MODE_NICH1>), (note_kernel(1, "k_blocked_assign<2>"), grid), dim3(block), 0,
                         stream, fs_dev, nfeat, tab, K, kpad, row0, nrows, row_id0, z, seed, sweep);
      break;
    case BlockedKernel::staged:
      hipLaunchKernelGGL((k_blocked_assign<MODE_STAGED>), (note_kernel(1, "k_blocked_assign<1>"), grid), dim3(block),
                         (size_t)nfeat * block * sizeof(uint32_t), stream, fs_dev, nfeat, tab, K, kpad, row0, nrows,
                         row_id0, z, seed, sweep);
      break;
    case BlockedKernel::global:
      hipLaunchKernelGGL((k_blocked_assign<MODE_GLOBAL>), (note_kernel(1, "k_blocked_assign<0>"), grid), dim3(block), 0,
                         stream, fs_dev, nfeat, tab, K, kpad, row0, nrows, row_id0, z, seed, sweep);
      break;
    case BlockedKernel::niw1:                      // (kernels_blocked_niw.hip launch_blocked_assign_niw)
      return fail(MSC_EHIP, "k_blocked_assign: no route sends a niw state here");
  }
  return launch_status("k_blocked_assign");
}

int launch_blocked_top_slot(hipStream_t stream, const uint32_t *cnt, uint32_t K, uint32_t *out) {
  hipLaunchKernelGGL(k_blocked_top_slot, dim3(1), dim3(256), 0, stream, cnt, K, out);
  return launch_status("k_blocked_top_slot");
}

}  // namespace msc
