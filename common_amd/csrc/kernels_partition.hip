// kernels_partition.hip -- gfx950 kernels that score candidate partitions against the z-matrix accumulator's counts
// (msc_zmatrix_partition_sums / msc_zmatrix_partition_loss, include/microscopes_hip.h):
//   k_zm_partition_gather  one lane per (selected row, candidate): lab[c][a] = cand[c][rows[a]], 0 in the last band's padding
//   k_zm_partition_sums    the hot path.  A workgroup owns one 64-row band and a batch of CB candidates and walks every
//                          column tile of the band: tile (min, max) of the upper triangle, read transposed below the
//                          diagonal, so no atomics on global memory and no second pass.  Lane = row, wave = a quarter of
//                          the tile's columns: a thread keeps its 16 counts in registers over the whole batch and the 16
//                          column labels of a candidate are wave-uniform (scalar loads); a pair costs a compare, a select
//                          and an add.  Writes w[c][a] = sum of C[a][b] over the b that c puts with a, and size[c][a].
//   k_zm_partition_loss    one workgroup per candidate: the integer sums of size - 1 and w - V and the double sum of
//                          log2 size - 2 log2 w over a, every thread its rows ascending, then a fixed tree; writes
//                          binder_num and vi_lb, or T = sum_{a<b} C[a][b] from the all-in-one partition
// Exactness: every sum is an integer sum.  PACKED (the accumulator has seen fewer than 2^20 samples, so every count is
// below 2^20): a count travels as count + 2^24, the 16 selected ones of a tile add up to at most 16 (2^20 - 1) < 2^24 in
// the low 24 bits and to at most 16 in the high 8, and the tile's partial is widened into a 64-bit accumulator holding
// w (< 2^18 2^20 = 2^38) in its low 40 bits and size (<= 2^18) above them.  Otherwise counts are added in 64 bits and
// the matches counted apart.  Columns b >= m are masked (the tiles' padding is not zero: a padded row holds label 0 in
// every sample); rows a >= m are computed and not stored.
#include "launchers.hpp"

namespace msc {

constexpr int kZpThreads = 256;
constexpr uint32_t kZpCount = 1u << 24;          // PACKED: one match, above the 24 bits of a tile's partial sum

__host__ __device__ inline uint64_t zp_tile_base(uint32_t ti, uint32_t tj, uint32_t nt) {   // kernels_query.hip's layout
  const uint64_t t = (uint64_t)ti;
  return ((t * nt - t * (t - 1) / 2) + (tj - ti)) * (uint64_t)(kZmTile * kZmTile);
}

__global__ __launch_bounds__(kZpThreads) void k_zm_partition_gather(const int32_t *__restrict__ cand, uint64_t ld,
                                                                    uint32_t ncand, const uint32_t *__restrict__ rows,
                                                                    uint32_t m, uint32_t mpad, int32_t *__restrict__ lab) {
  const uint32_t a = blockIdx.x * kZpThreads + threadIdx.x;
  if (a >= mpad) return;
  const uint32_t row = a < m ? rows[a] : 0u;
  for (uint32_t c = blockIdx.y; c < ncand; c += gridDim.y)
    lab[(uint64_t)c * mpad + a] = a < m ? cand[(uint64_t)c * ld + row] : 0;
}

// lab: [ncand][mpad] (mpad = 64 nt) of the launch's candidates; w_out / size_out: [ncand][m], either may be null.
// CB candidates a workgroup: blockIdx.y picks the batch, blockIdx.x the band.
template <bool PACKED, int CB>
__global__ __launch_bounds__(kZpThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_zm_partition_sums(const uint32_t *__restrict__ counts, uint32_t nt, uint32_t m, const int32_t *__restrict__ lab,
                         uint32_t ncand, uint64_t *__restrict__ w_out, uint32_t *__restrict__ size_out) {
  __shared__ int32_t s_row[CB][kZmTile];                    // the band's row labels of the batch
  __shared__ unsigned long long s_w[CB][kZmTile];           // sums over the four waves (PACKED: size above bit 40)
  __shared__ uint32_t s_size[PACKED ? 1 : CB][kZmTile];
  const uint32_t ti = blockIdx.x, c0 = blockIdx.y * CB;
  const uint32_t nc = min((uint32_t)CB, ncand - c0);        // (the grid has no batch past ncand)
  const int t = threadIdx.x, lane = t & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t mpad = nt * kZmTile;
  for (int q = t; q < CB * (int)kZmTile; q += kZpThreads) {
    const uint32_t c = q >> 6, r = q & 63;
    s_row[c][r] = c < nc ? lab[(uint64_t)(c0 + c) * mpad + ti * kZmTile + r] : 0;
    s_w[c][r] = 0ull;
    if (!PACKED) s_size[c][r] = 0u;
  }
  __syncthreads();
  unsigned long long acc[CB];
  uint32_t cnt[PACKED ? 1 : CB];
#pragma unroll
  for (int c = 0; c < CB; c++) acc[c] = 0ull;
  if (!PACKED) {
#pragma unroll
    for (int c = 0; c < CB; c++) cnt[c] = 0u;
  }
  for (uint32_t tj = 0; tj < nt; tj++) {
    // this thread's pairs: row `lane` of band ti with columns 16 wave + k of band tj
    uint32_t v[16];
    if (tj >= ti) {
      const uint4 *p = reinterpret_cast<const uint4 *>(counts + zp_tile_base(ti, tj, nt) + lane * kZmTile + wave * 16);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint4 x = p[k];
        v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
      }
    } else {
      const uint32_t *p = counts + zp_tile_base(tj, ti, nt) + wave * 16 * kZmTile + lane;   // transposed: 256 bytes a wave load
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] = p[k * kZmTile];
    }
    const uint32_t b0 = tj * kZmTile + wave * 16;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      if (PACKED)
        v[k] = b0 + k < m ? v[k] + kZpCount : 0u;
      else if (b0 + k >= m)
        v[k] = 0u;
    }
    const int32_t *colp = lab + (uint64_t)c0 * mpad + b0;
#pragma unroll
    for (int c = 0; c < CB; c++) {
      if ((uint32_t)c < nc) {                                // wave-uniform (a break instead sends acc[] to scratch)
        const int32_t *cl = colp + (uint64_t)c * mpad;       // 16 labels at a wave-uniform address: scalar loads
        const int32_t mine = s_row[c][lane];
        if (PACKED) {
          uint32_t part = 0u;
#pragma unroll
          for (int k = 0; k < 16; k++) part += cl[k] == mine ? v[k] : 0u;
          acc[c] += (unsigned long long)(part & (kZpCount - 1u)) + ((unsigned long long)(part >> 24) << 40);
        } else {
          unsigned long long part = 0ull;
          uint32_t n = 0u;
#pragma unroll
          for (int k = 0; k < 16; k++) {
            const bool eq = cl[k] == mine && b0 + k < m;
            part += eq ? v[k] : 0u;
            n += eq ? 1u : 0u;
          }
          acc[c] += part;
          cnt[c] += n;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CB; c++) {
    if ((uint32_t)c < nc) {
      atomicAdd(&s_w[c][lane], acc[c]);                      // integer adds in LDS: any order gives the same sum
      if (!PACKED) atomicAdd(&s_size[c][lane], cnt[c]);
    }
  }
  __syncthreads();
  const uint32_t a = ti * kZmTile + lane;
  if (a >= m) return;
  for (uint32_t c = wave; c < nc; c += kZpThreads / 64) {
    const unsigned long long s = s_w[c][lane];
    const uint64_t o = (uint64_t)(c0 + c) * m + a;
    if (w_out) w_out[o] = PACKED ? (s & ((1ull << 40) - 1ull)) : s;
    if (size_out) size_out[o] = PACKED ? (uint32_t)(s >> 40) : s_size[c][lane];
  }
}

// w / size: [ncand][m] of this launch's candidates.  tmode: the single candidate is the all-in-one partition, whose Q is
// T = sum_{a<b} C[a][b]: *T_io and *valid (nullable) are written.  Otherwise *T_io is read and binder[c], vi[c] (either
// may be null) are written.
__global__ __launch_bounds__(kZpThreads) void k_zm_partition_loss(const uint32_t *__restrict__ counts,
                                                                  const uint64_t *__restrict__ w,
                                                                  const uint32_t *__restrict__ size, uint32_t m,
                                                                  bool tmode, uint64_t *__restrict__ T_io,
                                                                  int64_t *__restrict__ binder, double *__restrict__ vi,
                                                                  uint64_t *__restrict__ valid) {
  __shared__ unsigned long long s_p[kZpThreads], s_q[kZpThreads];
  __shared__ double s_v[kZpThreads];
  const uint32_t c = blockIdx.x;
  const int t = threadIdx.x;
  const uint64_t V = counts[0];                              // C[0][0]: every valid sample puts a row with itself
  const uint64_t *wc = w + (uint64_t)c * m;
  const uint32_t *sc = size + (uint64_t)c * m;
  unsigned long long p2 = 0ull, q2 = 0ull;
  double lv = 0.0;
  const bool want_vi = !tmode && vi != nullptr;
  for (uint32_t a = t; a < m; a += kZpThreads) {
    const uint64_t wa = wc[a];
    const uint32_t sa = sc[a];
    p2 += sa - 1u;
    q2 += wa - V;
    if (want_vi) lv += log2((double)sa) - 2.0 * log2((double)wa);
  }
  s_p[t] = p2, s_q[t] = q2, s_v[t] = lv;
  __syncthreads();
  for (int h = kZpThreads / 2; h > 0; h >>= 1) {             // a fixed tree: the same bits from run to run
    if (t < h) {
      s_p[t] += s_p[t + h];
      s_q[t] += s_q[t + h];
      s_v[t] += s_v[t + h];
    }
    __syncthreads();
  }
  if (t != 0) return;
  if (tmode) {
    *T_io = s_q[0] / 2ull;                                   // all rows together: Q = sum_{a<b} C[a][b]
    if (valid) *valid = V;
    return;
  }
  // binder_num = T + V P - 2 Q, P = p2 / 2 (p2 counts ordered pairs: even), Q = q2 / 2
  if (binder) binder[c] = (int64_t)(*T_io + V * (s_p[0] / 2ull) - s_q[0]);
  if (vi) vi[c] = s_v[0] / (double)m + 2.0 * log2((double)V);
}

uint32_t zm_partition_chunk(uint32_t nt) {
  const uint64_t mpad = (uint64_t)nt * kZmTile;
  const uint64_t c = ((1ull << 23) / mpad) / 64 * 64;        // labels: at most 32 MiB
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c, 64), 512);
}

int launch_zm_partition_gather(hipStream_t stream, const int32_t *cand, uint64_t ld, uint32_t ncand, const uint32_t *rows,
                               uint32_t m, uint32_t nt, int32_t *lab) {
  const uint32_t mpad = nt * kZmTile;
  hipLaunchKernelGGL(k_zm_partition_gather, dim3(mpad / kZpThreads + (mpad % kZpThreads != 0), std::min(ncand, 65535u)),
                     dim3(kZpThreads), 0, stream, cand, ld, ncand, rows, m, mpad, lab);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_zm_partition_sums(hipStream_t stream, const uint32_t *counts, uint32_t nt, uint32_t m, bool packed,
                             const int32_t *lab, uint32_t ncand, uint64_t *w_out, uint32_t *size_out) {
  if (ncand == 0 || nt == 0 || (uint64_t)nt * kZmTile < m) return -2;
  if (packed) {
    constexpr int CB = kZmPartBatch;
    hipLaunchKernelGGL((k_zm_partition_sums<true, CB>),
                       (note_kernel(2, "k_zm_partition_sums<true, %d>", CB), dim3(nt, (ncand + CB - 1) / CB)),
                       dim3(kZpThreads), 0, stream, counts, nt, m, lab, ncand, w_out, size_out);
  } else {
    constexpr int CB = kZmPartBatch / 2;
    hipLaunchKernelGGL((k_zm_partition_sums<false, CB>),
                       (note_kernel(2, "k_zm_partition_sums<false, %d>", CB), dim3(nt, (ncand + CB - 1) / CB)),
                       dim3(kZpThreads), 0, stream, counts, nt, m, lab, ncand, w_out, size_out);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_zm_partition_loss(hipStream_t stream, const uint32_t *counts, const uint64_t *w, const uint32_t *size,
                             uint32_t m, uint32_t ncand, bool tmode, uint64_t *T_io, int64_t *binder, double *vi,
                             uint64_t *valid) {
  if (ncand == 0 || (tmode && ncand != 1)) return -2;
  hipLaunchKernelGGL(k_zm_partition_loss, (note_kernel(2, "k_zm_partition_loss"), dim3(ncand)), dim3(kZpThreads), 0,
                     stream, counts, w, size, m, tmode, T_io, binder, vi, valid);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
