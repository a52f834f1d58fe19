// kernels_refine.hip -- gfx950 kernels that refine a partition by greedy row moves against the z-matrix accumulator's
// counts until no single move lowers Binder's loss (msc_zmatrix_partition_refine, include/microscopes_hip.h gives the rule):
//   k_zm_refine_init    one workgroup per start: the gathered int32 labels of the positions become 16-bit ids numbered
//                       from 0 in the order of first position (an LDS hash table label -> first position, then ranks).
//                       More than max_clusters distinct labels: MSC_DEVERR_REFINE_CLUSTERS, the start stays inactive.
//   k_zm_refine_sweep   the hot path, one launch per sweep, one workgroup per start.  A sweep is sequential over the
//                       positions; the parallelism is inside a position (its m columns) and across the starts, whose
//                       workgroups walk the same rows of the dense counts at about the same time.  Ids (16 bit), cluster
//                       sizes and four sets of bins of s_k live in LDS.  A thread takes four consecutive columns at a time
//                       (one 16-byte load, one 8-byte LDS read of the ids), merges equal neighbours and adds what is left
//                       into its wave's set of bins with LDS atomics; a wave whose 256 columns all carry one id reduces
//                       them in registers instead (the all-in-one start would otherwise serialise 64 lanes on one
//                       bin).  The next step's columns (4096, or 16384 past 4096 positions) -- of this row, or the head of the next position's row, which is
//                       known whatever this position does -- are fetched into registers while these are reduced.  Then
//                       the bins are summed over the sets, g_k = 2 s_k - V n'_k, an argmax over (g_k, lowest id) and a
//                       min over the free ids run across the workgroup, and thread 0 applies the move.  A start whose
//                       previous sweep moved nothing returns at once.
//   k_zm_refine_finish  one workgroup per start: labels numbered by first position, binder_num = the start's less the
//                       decreases, sweeps, moves.
// Exactness: all integer.  s_k <= V m < 2^32 2^15 and g_k fit 64 bits with room; there is no packed form: the bins are
// 64-bit, or 32-bit where nsamples x m < 2^32 shows that no s_k passes 32 bits (the launcher is told).  Zero counts (and
// the masked columns b >= m, b == a) are not added at all.
#include "device_error.hpp"
#include "launchers.hpp"

namespace msc {

constexpr int kZrThreads = 256;
// the sweep: sixteen waves, four a SIMD -- a position's work is a few dozen vector instructions a column, and one wave a
// SIMD issues one every four cycles -- over kZrBinSets sets of bins (wave mod kZrBinSets adds into a set)
constexpr int kZrSweepThreads = 1024;
constexpr int kZrSweepWaves = kZrSweepThreads / 64;
constexpr int kZrBinSets = 4;
constexpr uint32_t kZrLoad = 4 * kZrSweepThreads;           // columns of one 16-byte load a thread
constexpr uint32_t kZrTable = 2 * kZmRefineMaxClusters;     // k_zm_refine_init's hash table
constexpr uint32_t kZrNone = 0xFFFFFFFFu;

__device__ inline uint32_t zr_hash(uint32_t x) {
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x & (kZrTable - 1u);
}

// lab: [nstarts][mpad] gathered labels (k_zm_partition_gather); ids: [nstarts][ldi]
__global__ __launch_bounds__(kZrThreads) void k_zm_refine_init(const int32_t *__restrict__ lab, uint32_t mpad, uint32_t m,
                                                               uint32_t max_clusters, uint16_t *__restrict__ ids,
                                                               uint64_t ldi, RefineStart *__restrict__ st) {
  __shared__ unsigned long long s_key[kZrTable];            // the label (zero-extended), all ones = empty
  __shared__ uint32_t s_first[kZrTable];
  __shared__ uint16_t s_rank[kZrTable];
  __shared__ uint32_t s_cnt, s_err;
  const uint32_t start = blockIdx.x;
  const int t = threadIdx.x;
  const int32_t *l = lab + (uint64_t)start * mpad;
  uint16_t *out = ids + (uint64_t)start * ldi;
  for (uint32_t q = t; q < kZrTable; q += kZrThreads) s_key[q] = ~0ull, s_first[q] = kZrNone;
  if (t == 0) s_cnt = 0u, s_err = 0u;
  __syncthreads();
  for (uint32_t a = t; a < m; a += kZrThreads) {
    if (*(volatile uint32_t *)&s_cnt > max_clusters) break;  // (already an error: do not fill the table)
    const unsigned long long key = (uint32_t)l[a];
    const uint32_t h = zr_hash((uint32_t)key);
    bool placed = false;
    for (uint32_t p = 0; p < kZrTable && !placed; p++) {
      const uint32_t slot = (h + p) & (kZrTable - 1u);
      const unsigned long long old = atomicCAS(&s_key[slot], ~0ull, key);
      if (old == ~0ull) atomicAdd(&s_cnt, 1u);
      if (old == ~0ull || old == key) {
        atomicMin(&s_first[slot], a);
        placed = true;
      }
    }
    if (!placed) s_err = 1u;
  }
  __syncthreads();
  if (s_err != 0u || s_cnt > max_clusters) {                 // (uniform)
    for (uint32_t a = t; a < ldi; a += kZrThreads) out[a] = 0;
    if (t == 0) {
      report_device_error(MSC_DEVERR_REFINE_CLUSTERS, start);
      st[start] = RefineStart{0, 0ull, 0u, 0u};
    }
    return;
  }
  for (uint32_t q = t; q < kZrTable; q += kZrThreads) {
    const uint32_t f = s_first[q];
    if (f == kZrNone) continue;
    uint32_t r = 0u;
    for (uint32_t o = 0; o < kZrTable; o++) r += s_first[o] < f ? 1u : 0u;   // (kZrNone is never below)
    s_rank[q] = (uint16_t)r;
  }
  __syncthreads();
  for (uint32_t a = t; a < ldi; a += kZrThreads) {
    uint16_t id = 0;
    if (a < m) {
      const unsigned long long key = (uint32_t)l[a];
      uint32_t slot = zr_hash((uint32_t)key);
      while (s_key[slot] != key) slot = (slot + 1u) & (kZrTable - 1u);       // (it is there)
      id = s_rank[slot];
    }
    out[a] = id;
  }
  if (t == 0) st[start] = RefineStart{0, 0ull, 0u, 1u};
}

__device__ inline unsigned long long zr_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// dense: [m][ldd] u32 counts, ldd a multiple of 4 and at most MP; order: nullable.  NL: the 16-byte loads a thread has in
// flight, NL kZrLoad columns a step (MP a multiple of that): 1 up to 4096 positions, 4 -- a whole row of 16384 -- beyond
// NARROW: V m < 2^32, so no s_k passes 32 bits and the bins are u32 (half the LDS traffic of the adds); otherwise u64.
template <int MP, int NL, bool NARROW>
__global__ __launch_bounds__(kZrSweepThreads) void k_zm_refine_sweep(const uint32_t *__restrict__ dense, uint64_t ldd,
                                                                uint32_t m, uint32_t max_clusters,
                                                                const uint32_t *__restrict__ order,
                                                                uint16_t *__restrict__ ids, RefineStart *__restrict__ st) {
  __shared__ __attribute__((aligned(16))) uint16_t s_id[MP];
  using bin_t = typename std::conditional<NARROW, uint32_t, unsigned long long>::type;
  __shared__ bin_t s_bin[kZrBinSets][kZmRefineMaxClusters];
  __shared__ uint32_t s_n[kZmRefineMaxClusters];
  __shared__ long long s_wg[kZrSweepWaves], s_gcur;
  __shared__ uint32_t s_wk[kZrSweepWaves], s_wf[kZrSweepWaves];
  const uint32_t start = blockIdx.x;
  RefineStart *me = st + start;
  if (me->active == 0u) return;                              // (uniform) converged, or never started
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  uint16_t *mine = ids + (uint64_t)start * ldd;
  for (uint32_t b = t; b < (uint32_t)MP; b += kZrSweepThreads) s_id[b] = b < m ? mine[b] : (uint16_t)0;
  for (uint32_t k = t; k < kZmRefineMaxClusters; k += kZrSweepThreads) {
    s_n[k] = 0u;
#pragma unroll
    for (int w = 0; w < kZrBinSets; w++) s_bin[w][k] = 0;
  }
  __syncthreads();
  for (uint32_t b = t; b < m; b += kZrSweepThreads) atomicAdd(&s_n[s_id[b]], 1u);
  __syncthreads();
  constexpr uint32_t kStep = NL * kZrLoad;
  static_assert(MP % kStep == 0, "whole steps");
  const unsigned long long V = dense[0];
  const uint32_t nsteps = ((uint32_t)ldd + kStep - 1u) / kStep;
  bin_t *bins = s_bin[wave % kZrBinSets];
  uint64_t moves = 0ull;                                     // (thread 0's)
  long long dec = 0;
  uint4 cur[NL], nxt[NL];
  auto load_step = [&](uint32_t pos, uint32_t step, uint4(&v)[NL]) {
    const uint32_t *row = dense + (uint64_t)pos * ldd;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const uint32_t b0 = step * kStep + j * kZrLoad + 4u * t;
      v[j] = b0 < ldd ? *reinterpret_cast<const uint4 *>(row + b0) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  uint32_t a = order ? order[0] : 0u;
  load_step(a, 0, cur);
  for (uint32_t i = 0; i < m; i++) {
    const uint32_t a_next = i + 1u < m ? (order ? order[i + 1u] : i + 1u) : a;
    const uint32_t c = s_id[a];
    for (uint32_t step = 0; step < nsteps; step++) {
      if (step + 1u < nsteps)
        load_step(a, step + 1u, nxt);
      else
        load_step(a_next, 0, nxt);
#pragma unroll
      for (int j = 0; j < NL; j++) {
        const uint32_t b0 = step * kStep + j * kZrLoad + 4u * t;               // < MP
        const uint2 packed = *reinterpret_cast<const uint2 *>(&s_id[b0]);
        const uint32_t id[4] = {packed.x & 0xFFFFu, packed.x >> 16, packed.y & 0xFFFFu, packed.y >> 16};
        const uint32_t raw[4] = {cur[j].x, cur[j].y, cur[j].z, cur[j].w};
        bin_t v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = (b0 + e < m && b0 + e != a) ? raw[e] : 0u;
        const uint32_t f = __builtin_amdgcn_readfirstlane(id[0]);
        if (__all(id[0] == f && id[1] == f && id[2] == f && id[3] == f)) {
          const bin_t s = (bin_t)zr_wave_sum((unsigned long long)v[0] + v[1] + v[2] + v[3]);
          if (lane == 0u && s != 0) atomicAdd(&bins[f], s);
        } else {
          bin_t acc = v[0];
          uint32_t k = id[0];
#pragma unroll
          for (int e = 1; e < 4; e++) {
            if (id[e] == k) {
              acc += v[e];
            } else {
              if (acc != 0) atomicAdd(&bins[k], acc);
              k = id[e], acc = v[e];
            }
          }
          if (acc != 0) atomicAdd(&bins[k], acc);
        }
      }
#pragma unroll
      for (int j = 0; j < NL; j++) cur[j] = nxt[j];
    }
    __syncthreads();                                         // the bins hold s_k, a share in every set
    long long bg = 0;
    uint32_t bk = kZrNone, bf = kZrNone;
    for (uint32_t k = t; k < max_clusters; k += kZrSweepThreads) {
      unsigned long long s = 0ull;
#pragma unroll
      for (int w = 0; w < kZrBinSets; w++) s += s_bin[w][k], s_bin[w][k] = 0;
      const uint32_t nk = s_n[k], np = nk - (k == c ? 1u : 0u);
      const long long g = (long long)(2ull * s) - (long long)(V * np);
      if (np > 0u && (bk == kZrNone || g > bg)) bg = g, bk = k;       // (k ascending: the lowest id among equals)
      if (k == c) s_gcur = np > 0u ? g : 0;
      if (nk == 0u && bf == kZrNone) bf = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long og = __shfl_xor(bg, o);
      const uint32_t ok = __shfl_xor(bk, o), of = __shfl_xor(bf, o);
      if (ok != kZrNone && (bk == kZrNone || og > bg || (og == bg && ok < bk))) bg = og, bk = ok;
      bf = of < bf ? of : bf;
    }
    if (lane == 0u) s_wg[wave] = bg, s_wk[wave] = bk, s_wf[wave] = bf;
    __syncthreads();
    if (t == 0u) {
#pragma unroll
      for (int w = 1; w < kZrSweepWaves; w++) {
        const long long og = s_wg[w];
        const uint32_t ok = s_wk[w], of = s_wf[w];
        if (ok != kZrNone && (bk == kZrNone || og > bg || (og == bg && ok < bk))) bg = og, bk = ok;
        bf = of < bf ? of : bf;
      }
      const long long g_cur = s_gcur;
      const bool with_others = s_n[c] > 1u;                  // n'_c > 0
      uint32_t target = kZrNone;
      long long gain = 0;
      if (bk != kZrNone && bg > g_cur)
        target = bk, gain = bg;
      else if (with_others && g_cur < 0 && bf != kZrNone)
        target = bf;                                         // alone, into the lowest free id
      if (target != kZrNone) {
        s_id[a] = (uint16_t)target;
        s_n[c] -= 1u;
        s_n[target] += 1u;
        dec += gain - g_cur;
        moves++;
      }
    }
    __syncthreads();
    a = a_next;
  }
  for (uint32_t b = t; b < m; b += kZrSweepThreads) mine[b] = s_id[b];
  if (t == 0u) {
    me->dec += dec;
    me->moves += moves;
    me->sweeps += 1u;
    me->active = moves != 0ull ? 1u : 0u;
  }
}

// labels: [nstarts][m]; every output is nullable
__global__ __launch_bounds__(kZrThreads) void k_zm_refine_finish(const uint16_t *__restrict__ ids, uint64_t ldi, uint32_t m,
                                                                 uint32_t max_clusters,
                                                                 const RefineStart *__restrict__ st,
                                                                 const int64_t *__restrict__ binder0,
                                                                 int32_t *__restrict__ labels, int64_t *__restrict__ binder,
                                                                 uint32_t *__restrict__ sweeps, uint64_t *__restrict__ moves) {
  __shared__ uint32_t s_first[kZmRefineMaxClusters];
  __shared__ uint32_t s_rank[kZmRefineMaxClusters];
  const uint32_t start = blockIdx.x, t = threadIdx.x;
  const uint16_t *mine = ids + (uint64_t)start * ldi;
  if (t == 0u) {
    if (binder) binder[start] = binder0[start] - st[start].dec;
    if (sweeps) sweeps[start] = st[start].sweeps;
    if (moves) moves[start] = st[start].moves;
  }
  if (labels == nullptr) return;
  for (uint32_t k = t; k < max_clusters; k += kZrThreads) s_first[k] = kZrNone;
  __syncthreads();
  for (uint32_t a = t; a < m; a += kZrThreads) atomicMin(&s_first[mine[a]], a);
  __syncthreads();
  for (uint32_t k = t; k < max_clusters; k += kZrThreads) {
    const uint32_t f = s_first[k];
    uint32_t r = 0u;
    if (f != kZrNone)
      for (uint32_t o = 0; o < max_clusters; o++) r += s_first[o] < f ? 1u : 0u;
    s_rank[k] = r;
  }
  __syncthreads();
  for (uint32_t a = t; a < m; a += kZrThreads) labels[(uint64_t)start * m + a] = (int32_t)s_rank[mine[a]];
}

int launch_zm_refine_init(hipStream_t stream, const int32_t *lab, uint32_t mpad, uint32_t m, uint32_t max_clusters,
                          uint32_t nstarts, uint16_t *ids, uint64_t ldi, RefineStart *st) {
  if (nstarts == 0 || m == 0 || m > kZmRefineMaxRows || max_clusters == 0 || max_clusters > kZmRefineMaxClusters ||
      max_clusters > m || ldi < m || mpad < m)
    return -2;
  hipLaunchKernelGGL(k_zm_refine_init, dim3(nstarts), dim3(kZrThreads), 0, stream, lab, mpad, m, max_clusters, ids, ldi,
                     st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int MP, int NL, bool NARROW>
static void zr_launch_sweep(hipStream_t stream, const uint32_t *dense, uint64_t ldd, uint32_t m, uint32_t max_clusters,
                            const uint32_t *order, uint32_t nstarts, uint16_t *ids, RefineStart *st) {
  hipLaunchKernelGGL((k_zm_refine_sweep<MP, NL, NARROW>),
                     (note_kernel(2, "k_zm_refine_sweep<%d, %d, %s>", MP, NL, NARROW ? "true" : "false"), dim3(nstarts)),
                     dim3(kZrSweepThreads), 0, stream, dense, ldd, m, max_clusters, order, ids, st);
}

int launch_zm_refine_sweep(hipStream_t stream, const uint32_t *dense, uint64_t ldd, uint32_t m, uint32_t max_clusters,
                           const uint32_t *order, bool narrow, uint32_t nstarts, uint16_t *ids, RefineStart *st) {
  if (nstarts == 0 || m == 0 || m > kZmRefineMaxRows || max_clusters == 0 || max_clusters > kZmRefineMaxClusters ||
      max_clusters > m || ldd < m || ldd % 4u != 0u || ldd > kZmRefineMaxRows)
    return -2;
  constexpr int kSmall = (int)kZrLoad, kLarge = (int)kZmRefineMaxRows;
  if (ldd <= kZrLoad) {
    if (narrow)
      zr_launch_sweep<kSmall, 1, true>(stream, dense, ldd, m, max_clusters, order, nstarts, ids, st);
    else
      zr_launch_sweep<kSmall, 1, false>(stream, dense, ldd, m, max_clusters, order, nstarts, ids, st);
  } else {
    if (narrow)
      zr_launch_sweep<kLarge, 4, true>(stream, dense, ldd, m, max_clusters, order, nstarts, ids, st);
    else
      zr_launch_sweep<kLarge, 4, false>(stream, dense, ldd, m, max_clusters, order, nstarts, ids, st);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_zm_refine_finish(hipStream_t stream, const uint16_t *ids, uint64_t ldi, uint32_t m, uint32_t max_clusters,
                            uint32_t nstarts, const RefineStart *st, const int64_t *binder0, int32_t *labels,
                            int64_t *binder, uint32_t *sweeps, uint64_t *moves) {
  if (nstarts == 0 || max_clusters == 0 || max_clusters > kZmRefineMaxClusters) return -2;
  hipLaunchKernelGGL(k_zm_refine_finish, dim3(nstarts), dim3(kZrThreads), 0, stream, ids, ldi, m, max_clusters, st,
                     binder0, labels, binder, sweeps, moves);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

MSC_DEFINE_BIND_ERROR_WORD(bind_error_word_refine)

}  // namespace msc
