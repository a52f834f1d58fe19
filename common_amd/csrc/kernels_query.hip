// kernels_query.hip -- gfx950 kernels of the z-matrix accumulator (msc_zmatrix_*, include/microscopes_hip.h):
//   k_zm_check   one lane per (selected row, sample): a label outside [0, nlabels) marks its sample bad (the sample's
//                batch slot, once) and reports MSC_DEVERR_ZMATRIX_LABEL; nothing is addressed by the label
//   k_zm_pack    one lane per (selected row, batch word): gathers the word's samples of the row and writes them into the
//                batch transposed to [row][word], four 8-bit or two 16-bit labels a word; a bad sample packs as 0
//   k_zm_count   one workgroup per pair tile (ti <= tj) of 64 x 64 rows: both bands' words staged in LDS 32 words at a
//                time, 4 x 4 pairs a lane; per pair and word  x = a ^ b,  y = ((x & L) + L) | x | L  (L = 0x7F7F7F7F or
//                0x7FFF7FFF) has 32 - popcount(y) equal labels; the batch's count is added to the u32 tile
//   k_zm_finish  the full m x m matrix from the upper-triangle tiles: mirrored, reordered, as u32 counts or count / S
// Exactness: a pair's count is an integer sum of per-word equal-label counts.  Every label that is not a sample's -- the
// zero padding after the batch's last sample and up to the chunk of 32 words, and the zeros a bad sample packs as -- is
// equal in both rows of every pair, so the batch adds  (words processed) x (labels per word) - (valid samples)  too many
// to every pair, and k_zm_count subtracts exactly that (the bad samples' number is counted on the device).
#include "device_error.hpp"
#include "launchers.hpp"

namespace msc {

constexpr int kZmThreads = 256;
constexpr int kZmChunk = 32;                 // batch words a band stages in LDS at a time
constexpr int kZmLdsStride = kZmChunk + 4;   // (words) 36: the 16 rows a ds_read_b128 lane group reads hit 16 disjoint bank quads

// the two instructions the compiler does not pick for the count's inner loop by itself: it splits a | b | c into two ORs
// and gives v_bcnt a zero accumulator followed by an add (seven instructions a word instead of five)
MSC_DEV uint32_t zm_or3(uint32_t a, uint32_t b, uint32_t c_uniform) {
  uint32_t d;
  asm("v_or3_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c_uniform));
  return d;
}
MSC_DEV uint32_t zm_bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t d;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
  return d;
}
// popcount(y) + acc, y = ((x & L) + L) | x | L: bit 7 (15) of a byte (half) of y is set iff that label of x is not 0, the
// other bits always, so popcount(y) = 32 - (equal labels)
template <uint32_t L>
MSC_DEV uint32_t zm_neq_acc(uint32_t a, uint32_t b, uint32_t acc) {
  const uint32_t x = a ^ b;
  return zm_bcnt_acc(zm_or3((x & L) + L, x, L), acc);
}

// upper-triangle tile (ti, tj), ti <= tj < nt: first count of its 64 x 64 block
__host__ __device__ inline uint64_t zm_tile_base(uint32_t ti, uint32_t tj, uint32_t nt) {
  const uint64_t t = (uint64_t)ti;
  return ((t * nt - t * (t - 1) / 2) + (tj - ti)) * (uint64_t)(kZmTile * kZmTile);
}

__global__ __launch_bounds__(kZmThreads) void k_zm_check(const int32_t *__restrict__ z, uint64_t ld, uint32_t nsamples,
                                                         const uint32_t *__restrict__ rows, uint32_t m, uint32_t nlabels,
                                                         uint32_t slot0, uint32_t *__restrict__ bad) {
  const uint32_t r = blockIdx.x * kZmThreads + threadIdx.x;
  if (r >= m) return;
  const uint32_t row = rows[r];
  for (uint32_t s = blockIdx.y; s < nsamples; s += gridDim.y) {
    const int32_t v = z[(uint64_t)s * ld + row];
    if ((uint32_t)v >= nlabels) {
      // (bad[kZmBatchMax] counts the bad samples of the batch: the lane that marks the slot first adds it)
      if (atomicExch(&bad[slot0 + s], 1u) == 0u) {
        atomicAdd(&bad[kZmBatchMax], 1u);
        report_device_error(MSC_DEVERR_ZMATRIX_LABEL, row);
      }
    }
  }
}

// word w of the batch holds slots [w * PW, w * PW + PW); this call's samples fill slots [slot0, slot0 + nsamples)
template <int PW>
__global__ __launch_bounds__(kZmThreads) void k_zm_pack(const int32_t *__restrict__ z, uint64_t ld, uint32_t nsamples,
                                                        const uint32_t *__restrict__ rows, uint32_t m, uint32_t slot0,
                                                        const uint32_t *__restrict__ bad, uint32_t *__restrict__ batch,
                                                        uint32_t w0, uint32_t nw) {
  const uint32_t r = blockIdx.x * kZmThreads + threadIdx.x;
  if (r >= m) return;
  constexpr uint32_t kBits = 32 / PW, kMask = (1u << kBits) - 1u;
  const uint32_t row = rows[r];
  for (uint32_t wi = blockIdx.y; wi < nw; wi += gridDim.y) {
    const uint32_t w = w0 + wi;
    uint32_t word = 0;
    bool whole = true;
#pragma unroll
    for (int k = 0; k < PW; k++) {
      const uint32_t slot = w * PW + k;
      if (slot < slot0 || slot >= slot0 + nsamples) {
        whole = false;
        continue;
      }
      const uint32_t v = (uint32_t)z[(uint64_t)(slot - slot0) * ld + row];
      if (bad[slot] == 0u) word |= (v & kMask) << (kBits * k);
    }
    uint32_t *dst = batch + (uint64_t)r * kZmBatchWords + w;
    if (whole)
      *dst = word;
    else if (word != 0u)
      atomicOr(dst, word);   // a word shared with the previous or the next call (the batch is zero where nothing is yet)
  }
}

// one workgroup per (tj, ti) of the launch grid; blocks with ti > tj leave at once
template <bool WIDE>
__global__ __launch_bounds__(kZmThreads) void k_zm_count(const uint32_t *__restrict__ batch, uint32_t nt, uint32_t nw,
                                                         uint32_t base, const uint32_t *__restrict__ bad,
                                                         uint32_t *__restrict__ counts) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (ti > tj) return;
  __shared__ __attribute__((aligned(16))) uint32_t sa[kZmTile * kZmLdsStride];
  __shared__ __attribute__((aligned(16))) uint32_t sb[kZmTile * kZmLdsStride];
  constexpr uint32_t L = WIDE ? 0x7FFF7FFFu : 0x7F7F7F7Fu;
  const int t = threadIdx.x;
  const int lj = t & 15, li = t >> 4;            // this lane's pairs: rows li + 16 r of band ti, lj + 16 c of band tj
  const uint32_t *ga = batch + (uint64_t)ti * kZmTile * kZmBatchWords;
  const uint32_t *gb = batch + (uint64_t)tj * kZmTile * kZmBatchWords;
  uint32_t acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] = 0u;
  for (uint32_t c0 = 0; c0 < nw; c0 += kZmChunk) {
    __syncthreads();
    // 64 rows x 32 words a band: 512 quads, two a lane (row q / 8, quad q % 8)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int q = t + h * kZmThreads, row = q >> 3, col = (q & 7) * 4;
      const uint4 va = *reinterpret_cast<const uint4 *>(ga + (uint64_t)row * kZmBatchWords + c0 + col);
      const uint4 vb = *reinterpret_cast<const uint4 *>(gb + (uint64_t)row * kZmBatchWords + c0 + col);
      *reinterpret_cast<uint4 *>(&sa[row * kZmLdsStride + col]) = va;
      *reinterpret_cast<uint4 *>(&sb[row * kZmLdsStride + col]) = vb;
    }
    __syncthreads();
#pragma unroll 2
    for (int w = 0; w < kZmChunk; w += 4) {
      uint4 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; r++) a[r] = *reinterpret_cast<const uint4 *>(&sa[(li + 16 * r) * kZmLdsStride + w]);
#pragma unroll
      for (int c = 0; c < 4; c++) b[c] = *reinterpret_cast<const uint4 *>(&sb[(lj + 16 * c) * kZmLdsStride + w]);
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          uint32_t s = acc[r][c];
          s = zm_neq_acc<L>(a[r].x, b[c].x, s);
          s = zm_neq_acc<L>(a[r].y, b[c].y, s);
          s = zm_neq_acc<L>(a[r].z, b[c].z, s);
          s = zm_neq_acc<L>(a[r].w, b[c].w, s);
          acc[r][c] = s;
        }
    }
  }
  // equal labels over the words processed, less the padding and the bad samples (see the head of the file):
  // base = (32 - labels per word) x words processed + samples staged; acc = the popcounts (32 - equal per word)
  const uint32_t delta0 = base - bad[kZmBatchMax];
  uint32_t *tile = counts + zm_tile_base(ti, tj, nt);
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      uint32_t *p = tile + (li + 16 * r) * kZmTile + (lj + 16 * c);
      *p += delta0 - acc[r][c];
    }
}

// out[a][b] = Z[i][j], i = order[a], j = order[b] (identity without order); Z from the tile holding (min, max)
template <bool NORM>
__global__ __launch_bounds__(kZmThreads) void k_zm_finish(const uint32_t *__restrict__ counts, uint32_t nt, uint32_t m,
                                                          const uint32_t *__restrict__ order, float S,
                                                          void *__restrict__ out, uint64_t ld) {
  const uint32_t b = blockIdx.x * kZmThreads + threadIdx.x;
  if (b >= m) return;
  const uint32_t j = order ? order[b] : b;
  for (uint32_t a = blockIdx.y; a < m; a += gridDim.y) {
    const uint32_t i = order ? order[a] : a;
    const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
    const uint32_t c = counts[zm_tile_base(lo / kZmTile, hi / kZmTile, nt) + (lo % kZmTile) * kZmTile + (hi % kZmTile)];
    if (NORM)
      static_cast<float *>(out)[(uint64_t)a * ld + b] = __fdiv_rn((float)c, S);   // IEEE division: count / S as numpy rounds it
    else
      static_cast<uint32_t *>(out)[(uint64_t)a * ld + b] = c;
  }
}

static inline uint32_t grid_y_cap(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n, 1), 65535); }

int launch_zm_stage(hipStream_t stream, const int32_t *z, uint64_t ld, uint32_t nsamples, const uint32_t *rows,
                    uint32_t m, uint32_t nlabels, bool wide, uint32_t slot0, uint32_t *bad, uint32_t *batch) {
  if (nsamples == 0 || slot0 + nsamples > zm_batch_cap(wide)) return -2;
  const uint32_t gx = (m + kZmThreads - 1) / kZmThreads;
  hipLaunchKernelGGL(k_zm_check, (note_kernel(2, "k_zm_check"), dim3(gx, grid_y_cap(nsamples))), dim3(kZmThreads), 0,
                     stream, z, ld, nsamples, rows, m, nlabels, slot0, bad);
  const uint32_t pw = wide ? 2u : 4u;
  const uint32_t w0 = slot0 / pw, w1 = (slot0 + nsamples + pw - 1) / pw;
  if (wide)
    hipLaunchKernelGGL(k_zm_pack<2>, (note_kernel(2, "k_zm_pack<2>"), dim3(gx, grid_y_cap(w1 - w0))), dim3(kZmThreads), 0,
                       stream, z, ld, nsamples, rows, m, slot0, bad, batch, w0, w1 - w0);
  else
    hipLaunchKernelGGL(k_zm_pack<4>, (note_kernel(2, "k_zm_pack<4>"), dim3(gx, grid_y_cap(w1 - w0))), dim3(kZmThreads), 0,
                       stream, z, ld, nsamples, rows, m, slot0, bad, batch, w0, w1 - w0);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_zm_count(hipStream_t stream, const uint32_t *batch, uint32_t nt, bool wide, uint32_t staged,
                    const uint32_t *bad, uint32_t *counts) {
  const uint32_t pw = wide ? 2u : 4u;
  if (staged == 0 || staged > zm_batch_cap(wide) || nt == 0 || nt > 65535) return -2;
  const uint32_t nw = ((staged + pw - 1) / pw + kZmChunk - 1) / kZmChunk * kZmChunk;   // words processed (<= kZmBatchWords)
  const uint32_t base = (32u - pw) * nw + staged;
  if (wide)
    hipLaunchKernelGGL(k_zm_count<true>, (note_kernel(2, "k_zm_count<true>"), dim3(nt, nt)), dim3(kZmThreads), 0, stream,
                       batch, nt, nw, base, bad, counts);
  else
    hipLaunchKernelGGL(k_zm_count<false>, (note_kernel(2, "k_zm_count<false>"), dim3(nt, nt)), dim3(kZmThreads), 0, stream,
                       batch, nt, nw, base, bad, counts);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_zm_finish(hipStream_t stream, const uint32_t *counts, uint32_t nt, uint32_t m, const uint32_t *order,
                     bool norm, float S, void *out, uint64_t ld) {
  const dim3 grid((m + kZmThreads - 1) / kZmThreads, grid_y_cap(m));
  if (norm)
    hipLaunchKernelGGL(k_zm_finish<true>, (note_kernel(2, "k_zm_finish<true>"), grid), dim3(kZmThreads), 0, stream, counts,
                       nt, m, order, S, out, ld);
  else
    hipLaunchKernelGGL(k_zm_finish<false>, (note_kernel(2, "k_zm_finish<false>"), grid), dim3(kZmThreads), 0, stream, counts,
                       nt, m, order, S, out, ld);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

MSC_DEFINE_BIND_ERROR_WORD(bind_error_word_query)

}  // namespace msc
