// kernels_refine_vi.hip -- gfx950 kernels that refine partitions by greedy row moves under the exact posterior expected
// variation of information (msc_partition_refine_vi; include/microscopes_hip.h gives the rule).  Everything is integer:
// the gains are differences of G(n) = F(n + 1) - F(n), F(n) = rint(n log2 n 2^24), read from the host's table
// (msc_vi_table), never computed here.
//   k_vi_canon      one workgroup per partition (a sample or a start): the int32 labels become 16-bit ids numbered from 0
//                   in the order of first row (canon_ids.hpp: an LDS hash table label -> first row, then ranks).  More
//                   than `cap` distinct labels: MSC_DEVERR_VI_CLUSTERS, ids all 0, one cluster reported (so that every
//                   later index stays in bounds); such a start stays inactive.
//   k_vi_offsets    one workgroup: off[s] = the sum of the cluster counts L of the samples before s, off[S] = the total.
//   k_vi_transpose  row[a][s] = off[s] + id_s[a], u32 [m][S]: the index of the stretch of cells N[s][l_s][.] that row a
//                   touches in sample s; a row's S of them are one contiguous read.
//   k_vi_count      cell(off[s] + id_s[a], id_start[a]) of the start += 1 over all (a, s): u16 counts (at most m <= 32768),
//                   two to a 32-bit atomic, which cannot carry into each other.  The cells were zeroed before.  A
//                   start's cells lie in blocks of 32 ids: block b holds, stretch after stretch, the 64 bytes of ids
//                   [32 b, 32 b + 32) (vi_cell), so the ids in use -- the low ones, whatever max_clusters allows --
//                   are one dense region: 1.4 MiB for 22 clusters in 1024 samples, where stretches of max_clusters =
//                   1024 cells spread them over 46 MiB.
//   k_vi_sweep      the hot path, one launch per sweep, one workgroup of sixteen waves per start, sequential over the
//                   rows.  Ids (16 bit), cluster sizes, the sums and the head of G live in LDS.  For a row the lanes take
//                   ids and the waves stride over the samples: a thread reads its sample's stretch of cells, looks G up
//                   (the count clamped to m - 1 first, so no cell value can index outside the table) and adds into 64-bit
//                   registers.  While the ids in use fit 32 (16, 8) lanes a wave takes 2 (4, 8) samples at a time and
//                   folds the lane groups by shuffles.  The waves' sums meet in LDS (one 64-bit LDS add per wave and id
//                   in use, not per cell), then D_k, the (smallest D, lowest id) and lowest-free-id reductions run across
//                   the workgroup, thread 0 decides, and on a move thread s moves its sample's two cells by plain
//                   stores (every s has its own stretch).  Ids from the highest one ever in use + 1 on are not visited.
//                   A start whose previous sweep moved nothing returns at once.
//   k_vi_finish     one workgroup per start: labels numbered by first row, decrease, sweeps, moves.
// Bounds: an id is below its partition's cluster count <= cap by construction (k_vi_canon); row[a][s] < off[S], the number
// of stretches a start's cells have; there are kcap / 32 blocks of ids, kcap >= max_clusters, and the sweep reads and
// writes ids below max_clusters only.  The cells of a start are read and written by its own workgroup alone.
#include "canon_ids.hpp"
#include "device_error.hpp"
#include "launchers.hpp"

namespace msc {

constexpr int kViThreads = 256;
constexpr int kViSweepThreads = 1024;
constexpr int kViSweepWaves = kViSweepThreads / 64;
constexpr uint32_t kViLdsG = 2048;                          // G(n) for n below this sits in LDS, beyond in L2
constexpr uint32_t kViNone = 0xFFFFFFFFu;
constexpr int kViBatch = 8;                                  // samples a thread has in flight while the ids in use fit 32 lanes

// where the count of (stretch, id k) lies in a start's cells: nstretch = off[S] stretches, blocks of kViCellPad ids
__host__ __device__ inline uint64_t vi_cell(uint32_t nstretch, uint32_t stretch, uint32_t k) {
  return ((uint64_t)(k / kViCellPad) * nstretch + stretch) * kViCellPad + (k % kViCellPad);
}
static_assert(kViSweepThreads >= (int)kViMaxClusters, "the reductions give every id a thread");

// lab: [n][ld] labels; ids: [n][ldi], ldi >= m (the tail is zeroed); count (nullable): [n] cluster counts; st (nullable):
// the starts' running totals.  part0: the index of the first partition in its set (the detail of a reported error)
__global__ __launch_bounds__(kViThreads) void k_vi_canon(const int32_t *__restrict__ lab, uint64_t ld, uint32_t m,
                                                         uint32_t cap, uint32_t part0, uint16_t *__restrict__ ids,
                                                         uint64_t ldi, uint32_t *__restrict__ count,
                                                         RefineStart *__restrict__ st) {
  __shared__ CanonTable<kViMaxClusters> tab;
  const uint32_t part = blockIdx.x;
  const uint32_t k = canon_ids<kViMaxClusters, kViThreads>(tab, lab + (uint64_t)part * ld, m, cap,
                                                           ids + (uint64_t)part * ldi, ldi);
  if (threadIdx.x != 0u) return;
  if (k == 0u) report_device_error(MSC_DEVERR_VI_CLUSTERS, part0 + part);
  if (count) count[part] = k == 0u ? 1u : k;
  if (st) st[part] = RefineStart{0, 0ull, 0u, k == 0u ? 0u : 1u};
}

// L: [S] cluster counts; off: [S + 1]
__global__ __launch_bounds__(1024) void k_vi_offsets(const uint32_t *__restrict__ L, uint32_t S, uint32_t *__restrict__ off) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (S + 1023u) / 1024u;
  const uint32_t lo = min(t * per, S), hi = min(lo + per, S);
  uint32_t mine = 0u;
  for (uint32_t s = lo; s < hi; s++) mine += L[s];
  s_sum[t] = mine;
  __syncthreads();
  for (uint32_t o = 1u; o < 1024u; o <<= 1) {               // inclusive scan of the threads' sums
    const uint32_t v = t >= o ? s_sum[t - o] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint32_t run = s_sum[t] - mine;
  for (uint32_t s = lo; s < hi; s++) off[s] = run, run += L[s];
  if (t == 1023u) off[S] = s_sum[t];
}

// ids: [S][ldi]; row: [m][S]
__global__ __launch_bounds__(kViThreads) void k_vi_transpose(const uint16_t *__restrict__ ids, uint64_t ldi,
                                                             const uint32_t *__restrict__ off, uint32_t S, uint32_t m,
                                                             uint32_t *__restrict__ row) {
  __shared__ uint32_t tile[64][65];
  const uint32_t tx = threadIdx.x & 63u, ty = threadIdx.x >> 6;
  const uint32_t a0 = blockIdx.x * 64u, s0 = blockIdx.y * 64u;
  for (uint32_t r = ty; r < 64u; r += 4u) {
    const uint32_t s = s0 + r, a = a0 + tx;
    tile[r][tx] = (s < S && a < m) ? off[s] + ids[(uint64_t)s * ldi + a] : 0u;
  }
  __syncthreads();
  for (uint32_t r = ty; r < 64u; r += 4u) {
    const uint32_t a = a0 + r, s = s0 + tx;
    if (a < m && s < S) row[(uint64_t)a * S + s] = tile[tx][r];
  }
}

// cells: [nstarts][cells_per_start] u16, zero; cells_per_start = nstretch * kcap, nstretch = off[S]
__global__ __launch_bounds__(kViThreads) void k_vi_count(const uint32_t *__restrict__ row, uint32_t S, uint32_t m,
                                                         const uint16_t *__restrict__ ids, uint64_t ldi,
                                                         const RefineStart *__restrict__ st, uint32_t nstretch,
                                                         uint16_t *__restrict__ cells, uint64_t cells_per_start) {
  const uint32_t start = blockIdx.y;
  if (st[start].active == 0u) return;                        // (uniform) a start with too many clusters
  const uint16_t *id = ids + (uint64_t)start * ldi;
  uint32_t *words = reinterpret_cast<uint32_t *>(cells + (uint64_t)start * cells_per_start);
  const uint64_t total = (uint64_t)m * S;
  for (uint64_t i = (uint64_t)blockIdx.x * kViThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kViThreads) {
    const uint32_t a = (uint32_t)(i / S);
    const uint64_t cell = vi_cell(nstretch, row[i], id[a]);
    atomicAdd(&words[cell >> 1], (cell & 1ull) ? 0x10000u : 1u);
  }
}

struct ViLds {
  uint16_t id[kViMaxRows];
  long long G[kViLdsG];
  unsigned long long sum[kViMaxClusters];                    // sum over the samples of G(n'^s_{k, l_s})
  uint32_t n[kViMaxClusters];
  long long wd[kViSweepWaves], dcur;
  uint32_t wk[kViSweepWaves], wf[kViSweepWaves];
  uint32_t khi, target;
};

// G(n') of a cell's count: the row's own cell counts the row itself; the clamp keeps any count inside the table
__device__ inline unsigned long long vi_g(const ViLds &l, const int64_t *__restrict__ G, uint32_t top, uint32_t count,
                                          bool own) {
  uint32_t n = own ? (count > 0u ? count - 1u : 0u) : count;
  n = n < top ? n : top;
  return (unsigned long long)(n < kViLdsG ? l.G[n] : G[n]);
}

// NK: the 64-id slots a thread keeps sums for in one pass over the samples
template <int NK>
__global__ __launch_bounds__(kViSweepThreads) void k_vi_sweep(const ViSweepArgs p) {
  __shared__ ViLds l;
  const uint32_t start = blockIdx.x;
  RefineStart *me = p.st + start;
  if (me->active == 0u) return;                              // (uniform) converged, or never started
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t m = p.m, S = p.S, top = m - 1u;
  const uint32_t nstretch = (uint32_t)(p.cells_per_start / p.kcap);
  uint16_t *mine = p.ids + (uint64_t)start * p.ldi;
  uint16_t *cells = p.cells + (uint64_t)start * p.cells_per_start;     // (read and written: neither const nor restrict)
  const int64_t *__restrict__ G = p.G;
  for (uint32_t b = t; b < m; b += kViSweepThreads) l.id[b] = mine[b];
  for (uint32_t n = t; n < kViLdsG; n += kViSweepThreads) l.G[n] = n < m ? G[n] : 0;
  for (uint32_t k = t; k < kViMaxClusters; k += kViSweepThreads) l.n[k] = 0u, l.sum[k] = 0ull;
  if (t == 0u) l.khi = 0u;
  __syncthreads();
  for (uint32_t b = t; b < m; b += kViSweepThreads) {
    const uint32_t k = l.id[b];
    atomicAdd(&l.n[k], 1u);
    atomicMax(&l.khi, k + 1u);
  }
  __syncthreads();
  uint64_t moves = 0ull;                                     // (thread 0's)
  long long dec = 0;
  for (uint32_t i = 0; i < m; i++) {
    const uint32_t a = p.order ? p.order[i] : i;
    const uint32_t c = l.id[a], khi = l.khi;                 // khi <= max_clusters <= kcap
    const uint32_t *__restrict__ ra = p.row + (uint64_t)a * S;
    if (khi <= 32u) {
      // w lanes a sample, 64 / w samples a wave at a time
      const uint32_t shift = khi <= 8u ? 3u : khi <= 16u ? 4u : 5u, w = 1u << shift, per = 64u >> shift;
      const uint32_t k = lane & (w - 1u);
      const uint32_t kk = k < khi ? k : khi - 1u, step = kViSweepWaves * per;
      unsigned long long acc = 0ull;
      // kViBatch samples at a time: their stretch indices, then their cells, are in flight together (a sample past the
      // end reads stretch 0 and is not added)
      for (uint32_t s0 = wave * per + (lane >> shift); s0 < S; s0 += kViBatch * step) {
        uint32_t stretch[kViBatch], count[kViBatch];
#pragma unroll
        for (int u = 0; u < kViBatch; u++) stretch[u] = s0 + u * step < S ? ra[s0 + u * step] : 0u;
#pragma unroll
        for (int u = 0; u < kViBatch; u++) count[u] = cells[vi_cell(nstretch, stretch[u], kk)];
#pragma unroll
        for (int u = 0; u < kViBatch; u++)
          if (s0 + u * step < S && k < khi) acc += vi_g(l, G, top, count[u], k == c);
      }
      for (uint32_t o = w; o < 64u; o <<= 1) acc += __shfl_xor(acc, o);
      if (lane < khi && acc != 0ull) atomicAdd(&l.sum[lane], acc);
    } else {
      // 64 NK ids a pass over the samples: one pass up to 512 ids in use, two beyond (the sums stay in registers)
      for (uint32_t base = 0u; base < khi; base += 64u * NK) {
        unsigned long long acc[NK];
#pragma unroll
        for (int j = 0; j < NK; j++) acc[j] = 0ull;
        for (uint32_t s = wave; s < S; s += kViSweepWaves) {
          const uint32_t stretch = ra[s];
          uint32_t count[NK];
#pragma unroll
          for (int j = 0; j < NK; j++) {
            const uint32_t k = base + 64u * j + lane;
            count[j] = cells[vi_cell(nstretch, stretch, k < khi ? k : khi - 1u)];
          }
#pragma unroll
          for (int j = 0; j < NK; j++) {
            const uint32_t k = base + 64u * j + lane;
            if (k < khi) acc[j] += vi_g(l, G, top, count[j], k == c);
          }
        }
#pragma unroll
        for (int j = 0; j < NK; j++) {
          const uint32_t k = base + 64u * j + lane;
          if (k < khi && acc[j] != 0ull) atomicAdd(&l.sum[k], acc[j]);
        }
      }
    }
    __syncthreads();                                         // the sums are whole
    long long bd = 0;
    uint32_t bk = kViNone, bf = kViNone;
    if (t < p.max_clusters && t <= khi) {                    // (id khi is empty: it may be the lowest free one)
      const uint32_t k = t, nk = l.n[k];
      if (k < khi) {
        const uint32_t np = nk - (k == c ? 1u : 0u);
        const long long d = (long long)((unsigned long long)S * vi_g(l, G, top, np, false)) - (long long)(2ull * l.sum[k]);
        l.sum[k] = 0ull;
        if (np > 0u) bd = d, bk = k;
        if (k == c) l.dcur = np > 0u ? d : 0;
      }
      if (nk == 0u) bf = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long od = __shfl_xor(bd, o);
      const uint32_t ok = __shfl_xor(bk, o), of = __shfl_xor(bf, o);
      if (ok != kViNone && (bk == kViNone || od < bd || (od == bd && ok < bk))) bd = od, bk = ok;
      bf = of < bf ? of : bf;
    }
    if (lane == 0u) l.wd[wave] = bd, l.wk[wave] = bk, l.wf[wave] = bf;
    __syncthreads();
    if (t == 0u) {
#pragma unroll
      for (int v = 1; v < kViSweepWaves; v++) {
        const long long od = l.wd[v];
        const uint32_t ok = l.wk[v], of = l.wf[v];
        if (ok != kViNone && (bk == kViNone || od < bd || (od == bd && ok < bk))) bd = od, bk = ok;
        bf = of < bf ? of : bf;
      }
      const long long d_cur = l.dcur;
      const bool with_others = l.n[c] > 1u;                  // n'_c > 0
      uint32_t target = bk;
      long long d_target = bd;
      if (with_others && bf != kViNone && bd > 0) target = bf, d_target = 0;   // alone, into the lowest free id
      if (target != kViNone && d_target < d_cur) {
        l.id[a] = (uint16_t)target;
        l.n[c] -= 1u;
        l.n[target] += 1u;
        if (target >= khi) l.khi = target + 1u;
        dec += d_cur - d_target;
        moves++;
      } else {
        target = kViNone;
      }
      l.target = target;
    }
    __syncthreads();
    const uint32_t target = l.target;
    if (target != kViNone) {                                 // (uniform)
      for (uint32_t s = t; s < S; s += kViSweepThreads) {
        const uint32_t stretch = ra[s];
        cells[vi_cell(nstretch, stretch, c)] -= 1u;
        cells[vi_cell(nstretch, stretch, target)] += 1u;
      }
      __syncthreads();                                       // the next row reads these cells
    }
  }
  for (uint32_t b = t; b < m; b += kViSweepThreads) mine[b] = l.id[b];
  if (t == 0u) {
    me->dec += dec;
    me->moves += moves;
    me->sweeps += 1u;
    me->active = moves != 0ull ? 1u : 0u;
  }
}

// labels: [nstarts][m]; every output is nullable
__global__ __launch_bounds__(kViThreads) void k_vi_finish(const uint16_t *__restrict__ ids, uint64_t ldi, uint32_t m,
                                                          uint32_t max_clusters, const RefineStart *__restrict__ st,
                                                          int32_t *__restrict__ labels, int64_t *__restrict__ decrease,
                                                          uint32_t *__restrict__ sweeps, uint64_t *__restrict__ moves) {
  __shared__ uint32_t s_first[kViMaxClusters];
  __shared__ uint32_t s_rank[kViMaxClusters];
  const uint32_t start = blockIdx.x, t = threadIdx.x;
  const uint16_t *mine = ids + (uint64_t)start * ldi;
  if (t == 0u) {
    if (decrease) decrease[start] = st[start].dec;
    if (sweeps) sweeps[start] = st[start].sweeps;
    if (moves) moves[start] = st[start].moves;
  }
  if (labels == nullptr) return;
  for (uint32_t k = t; k < max_clusters; k += kViThreads) s_first[k] = kViNone;
  __syncthreads();
  for (uint32_t a = t; a < m; a += kViThreads) atomicMin(&s_first[mine[a]], a);      // (an id is below max_clusters)
  __syncthreads();
  for (uint32_t k = t; k < max_clusters; k += kViThreads) {
    const uint32_t f = s_first[k];
    uint32_t r = 0u;
    if (f != kViNone)
      for (uint32_t o = 0; o < max_clusters; o++) r += s_first[o] < f ? 1u : 0u;
    s_rank[k] = r;
  }
  __syncthreads();
  for (uint32_t a = t; a < m; a += kViThreads) labels[(uint64_t)start * m + a] = (int32_t)s_rank[mine[a]];
}

static bool vi_shape_ok(uint32_t m, uint32_t n) { return n != 0 && m != 0 && m <= kViMaxRows; }

int launch_vi_canon(hipStream_t stream, const int32_t *lab, uint64_t ld, uint32_t m, uint32_t cap, uint32_t nparts,
                    uint32_t part0, uint16_t *ids, uint64_t ldi, uint32_t *count, RefineStart *st) {
  if (!vi_shape_ok(m, nparts) || cap == 0 || cap > kViMaxClusters || ld < m || ldi < m) return -2;
  hipLaunchKernelGGL(k_vi_canon, dim3(nparts), dim3(kViThreads), 0, stream, lab, ld, m, cap, part0, ids, ldi, count, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_vi_rows(hipStream_t stream, const uint16_t *ids, uint64_t ldi, const uint32_t *L, uint32_t S, uint32_t m,
                   uint32_t *off, uint32_t *row) {
  if (!vi_shape_ok(m, S) || S > kViMaxSamples || ldi < m) return -2;
  hipLaunchKernelGGL(k_vi_offsets, dim3(1), dim3(1024), 0, stream, L, S, off);
  hipLaunchKernelGGL(k_vi_transpose, dim3((m + 63u) / 64u, (S + 63u) / 64u), dim3(kViThreads), 0, stream, ids, ldi, off, S,
                     m, row);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_vi_count(hipStream_t stream, int num_cus, const ViSweepArgs &p, uint32_t nstarts) {
  if (!vi_shape_ok(p.m, nstarts) || p.S == 0 || p.kcap == 0 || p.kcap % kViCellPad != 0u || p.cells_per_start % p.kcap != 0u)
    return -2;
  const uint64_t total = (uint64_t)p.m * p.S;
  const uint32_t want = (uint32_t)std::min<uint64_t>((total + kViThreads - 1) / kViThreads, 65535);
  const uint32_t share = std::max(1u, 8u * (uint32_t)std::max(num_cus, 1) / nstarts);   // about 8 workgroups a CU in all
  hipLaunchKernelGGL(k_vi_count, dim3(std::min(want, share), nstarts), dim3(kViThreads), 0, stream, p.row, p.S, p.m, p.ids,
                     p.ldi, p.st, (uint32_t)(p.cells_per_start / p.kcap), p.cells, p.cells_per_start);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int NK>
static void vi_launch_sweep(hipStream_t stream, const ViSweepArgs &p, uint32_t nstarts) {
  hipLaunchKernelGGL((k_vi_sweep<NK>), (note_kernel(2, "k_vi_sweep<%d>", NK), dim3(nstarts)), dim3(kViSweepThreads), 0,
                     stream, p);
}

int launch_vi_sweep(hipStream_t stream, const ViSweepArgs &p, uint32_t nstarts) {
  if (!vi_shape_ok(p.m, nstarts) || p.S == 0 || p.max_clusters == 0 || p.max_clusters > p.kcap ||
      p.kcap > kViMaxClusters || p.kcap % kViCellPad != 0u || p.cells_per_start % p.kcap != 0u || p.max_clusters > p.m ||
      p.ldi < p.m)
    return -2;
  switch (route_vi_refine(p.kcap)) {
    case 1: vi_launch_sweep<1>(stream, p, nstarts); break;
    case 2: vi_launch_sweep<2>(stream, p, nstarts); break;
    case 4: vi_launch_sweep<4>(stream, p, nstarts); break;
    case 8: vi_launch_sweep<8>(stream, p, nstarts); break;
    default: return -2;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_vi_finish(hipStream_t stream, const uint16_t *ids, uint64_t ldi, uint32_t m, uint32_t max_clusters,
                     uint32_t nstarts, const RefineStart *st, int32_t *labels, int64_t *decrease, uint32_t *sweeps,
                     uint64_t *moves) {
  if (!vi_shape_ok(m, nstarts) || max_clusters == 0 || max_clusters > kViMaxClusters || ldi < m) return -2;
  hipLaunchKernelGGL(k_vi_finish, dim3(nstarts), dim3(kViThreads), 0, stream, ids, ldi, m, max_clusters, st, labels,
                     decrease, sweeps, moves);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

MSC_DEFINE_BIND_ERROR_WORD(bind_error_word_refine_vi)

}  // namespace msc
