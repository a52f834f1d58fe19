// kernels_linkage.hip -- Prim's chain of scipy's single linkage over a dense z-matrix (msc_linkage_single,
// include/microscopes_hip.h; the algorithm, the tie rule and the host restatement: linkage_host.hpp).
//   k_linkage_prim<C, VEC>  ONE workgroup carries the chain, as k_sweep_seq does: step i + 1 reads the row step i chose.
//                 A thread owns C columns (linkage::column), keeps their D in registers and their unmerged flags in one
//                 64-bit mask.  Per step: the owner of x clears its flag; every thread loads its elements of row x
//                 (VEC: 16 bytes a group of four columns, 8 bytes at C = 2 -- the launcher asks for it when every row
//                 starts on a multiple of that; otherwise one float at a time), lowers D and forms its minimum of
//                 (D[j], j); the wave reduces the key and then the column among the lanes at that key (DPP, no LDS);
//                 lane 0 of every wave writes the wave's minimum into one of two LDS slot rows, ONE barrier, and every
//                 wave reduces the wave minima for itself, so all of them know y without a second barrier.  The slot
//                 rows alternate: a wave can write row i % 2 again only after the barrier of step i + 1, which every
//                 wave reaches after it has read step i's.  A single wave skips the slots and the barrier.  Lane 0 of
//                 wave 0 appends (x, y, d).  The step is one basic block: no branch a column, every load issued.
// The matrix is only read, the diagonal's value never used (x is merged before its row is scanned).  One float at a time nothing
// outside columns [0, n) of row x is read; VEC reads whole groups, up to 3 floats past column n - 1 inside the row's
// ld floats (include/microscopes_hip.h says so), and never uses them.
#include "launchers.hpp"
#include "linkage_host.hpp"

namespace msc {

using namespace linkage;

// unsigned minimum over the wave, in every lane.  "v_min_u32_dpp v, v, v <ctrl>" computes min(moved v, v) in the lanes
// that have a source and leaves the others alone; lane 63 ends with the minimum of all 64 (kernels_sweep.hip
// MSC_DPP_REDUCE: s_nop 1 = the two wait states a DPP read needs after a VALU write of its source).
__device__ __forceinline__ uint32_t lk_wave_min(uint32_t v) {
  asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
               "s_nop 1"
               : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the same over lanes 0 .. 15 alone (the wave minima: at most 16 waves)
__device__ __forceinline__ uint32_t lk_row_min(uint32_t v) {
  asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1"
               : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
}

template <int C, bool VEC>
__global__ __launch_bounds__(kMaxThreads) void k_linkage_prim(const float *__restrict__ z, uint64_t ld, uint32_t n,
                                                              double *__restrict__ edges) {
  constexpr uint32_t V = C < 4 ? C : 4, G = C / V;
  // groups whose loads are in flight together: at 64 columns a thread D alone is half of the 128 registers a wave of a
  // 1024-thread workgroup has, so a step takes the row in two halves
  constexpr uint32_t kBatch = C > 32 ? G / 2 : G;
  __shared__ uint32_t slot_key[2][16], slot_j[2][16];
  const uint32_t T = C == 1 ? blockDim.x : kMaxThreads;   // (the launcher's shapes: linkage::shape_for)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, nw = T >> 6;
  float D[C];
  uint64_t unmerged = 0;
#pragma unroll
  for (int k = 0; k < C; k++) {
    D[k] = INFINITY;
    if (column(t, T, V, k) < n) unmerged |= 1ull << k;
  }
  uint32_t x = 0;
  for (uint32_t i = 0; i + 1 < n; i++) {
    {
      const uint32_t q = x / V, owner = C == 1 ? q : q % kMaxThreads, k = C == 1 ? 0u : (q / kMaxThreads) * V + x % V;
      if (t == owner) unmerged &= ~(1ull << k);
    }
    const float *__restrict__ row = z + (uint64_t)x * ld;
    float best = INFINITY;
    uint32_t bk = kNone;
    // (the offsets below do not change from step to step, and the compiler would keep every one of them in a register
    // of its own for the whole chain; from a thread index it cannot see through it works them out again each step)
    uint32_t ts = t;
    asm volatile("" : "+v"(ts));
#pragma unroll
    for (uint32_t g0 = 0; g0 < G; g0 += kBatch) {
      // every load is issued, whatever the lane owns: a group (VEC) or a column at or past n reads the row's first
      // instead, and its value is never used (such a column is never unmerged).  No branch, so the loads of a batch
      // are in flight together.  VEC: a group that begins below n lies inside the row's ld floats (ld % V == 0).
      float v[kBatch * V];
#pragma unroll
      for (uint32_t g = 0; g < kBatch; g++) {
        const uint32_t j0 = V * (ts + T * (g0 + g));
        if (VEC && V == 4) {
          const float4 w = *reinterpret_cast<const float4 *>(row + (j0 < n ? j0 : 0u));
          v[4 * g] = w.x, v[4 * g + 1] = w.y, v[4 * g + 2] = w.z, v[4 * g + 3] = w.w;
        } else if (VEC && V == 2) {
          const float2 w = *reinterpret_cast<const float2 *>(row + (j0 < n ? j0 : 0u));
          v[2 * g] = w.x, v[2 * g + 1] = w.y;
        } else {
#pragma unroll
          for (uint32_t e = 0; e < V; e++) v[V * g + e] = row[j0 + e < n ? j0 + e : 0u];
        }
      }
      // D against the row, and the thread's minimum so far.  Ascending k is ascending j, so the strict comparison keeps
      // the lowest column among equal distances.  D of a merged column goes on being updated and is never looked at.
      // (The minimum is remembered as k, a constant of the unrolled code, and turned into its column once a step.)
#pragma unroll
      for (uint32_t e = 0; e < kBatch * V; e++) {
        const uint32_t k = g0 * V + e;
        D[k] = fminf(D[k], 1.0f - v[e]);
        const bool better = ((unmerged >> k) & 1ull) != 0ull && D[k] < best;
        best = better ? D[k] : best;
        bk = better ? k : bk;
      }
      if (kBatch < G) __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t key = kNone, j = kNone;
    if (bk != kNone) {
      key = float_key(best), j = column(t, T, V, bk);
    } else if (unmerged != 0ull) {
      j = column(t, T, V, (uint32_t)__builtin_ctzll(unmerged));   // (linkage_host.hpp Cand)
    }
    uint32_t kmin = lk_wave_min(key);
    uint32_t jmin = lk_wave_min(key == kmin ? j : kNone);
    if (nw > 1) {
      const uint32_t b = i & 1u;
      if (lane == 0) slot_key[b][wave] = kmin, slot_j[b][wave] = jmin;
      __syncthreads();
      const uint32_t wk = lane < nw ? slot_key[b][lane & 15u] : kNone;
      const uint32_t wj = lane < nw ? slot_j[b][lane & 15u] : kNone;
      kmin = lk_row_min(wk);
      jmin = lk_row_min(wk == kmin ? wj : kNone);
    }
    if (t == 0) {
      double *e = edges + 3 * (uint64_t)i;
      e[0] = (double)x, e[1] = (double)jmin, e[2] = cand_distance(kmin);
    }
    x = jmin;
  }
}

template <int C>
static void launch_prim(hipStream_t stream, bool vec, uint32_t threads, const float *z, uint64_t ld, uint32_t n,
                        double *edges) {
  note_kernel(2, "k_linkage_prim<%d, %s>", C, tf(vec));
  if constexpr (C > 1) {   // (one column a thread has no wide form)
    if (vec) {
      hipLaunchKernelGGL((k_linkage_prim<C, true>), dim3(1), dim3(threads), 0, stream, z, ld, n, edges);
      return;
    }
  }
  hipLaunchKernelGGL((k_linkage_prim<C, false>), dim3(1), dim3(threads), 0, stream, z, ld, n, edges);
}

int launch_linkage_prim(hipStream_t stream, const float *z, uint64_t ld, uint32_t n, double *edges) {
  const Shape s = shape_for(n);
  if (s.threads == 0) return -2;
  // wide loads: every row must start on a multiple of the load's width
  const uint32_t bytes = 4 * vec_of(s.cols);
  const bool vec = s.cols > 1 && reinterpret_cast<uintptr_t>(z) % bytes == 0 && (ld * 4) % bytes == 0;
  switch (s.cols) {
    case 1: launch_prim<1>(stream, false, s.threads, z, ld, n, edges); break;
    case 2: launch_prim<2>(stream, vec, s.threads, z, ld, n, edges); break;
    case 4: launch_prim<4>(stream, vec, s.threads, z, ld, n, edges); break;
    case 8: launch_prim<8>(stream, vec, s.threads, z, ld, n, edges); break;
    case 16: launch_prim<16>(stream, vec, s.threads, z, ld, n, edges); break;
    case 32: launch_prim<32>(stream, vec, s.threads, z, ld, n, edges); break;
    case 64: launch_prim<64>(stream, vec, s.threads, z, ld, n, edges); break;
    default: return -2;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
