// kernels_distance.hip -- gfx950 kernels behind msc_partition_distances (include/microscopes_hip.h states the definitions):
// the contingency sums of every partition of one set against every partition of another, over the same m rows.
//   k_pd_log2    tab[n] = log2 n for 0 < n <= m in float64, filled once per context and m.
//   k_pd_canon   one workgroup per partition: the int32 labels become 16-bit ids numbered from 0 in the order of first
//                row (an LDS hash table label -> first row, then ranks, as k_zm_refine_init), the cluster sizes are counted
//                and pairs_p = sum C(size, 2), nlogn_p = sum size log2 size (ids ascending: thread t takes ids t, t + 256, ...,
//                then the fixed tree of pd_block_sum) are written.  More than kPdMaxClusters labels:
//                MSC_DEVERR_DISTANCE_CLUSTERS, the cluster count is kPdBad, the outputs are -1 / NaN and the ids are 0.
//   k_pd_pairs   the hot path.  A work item is one a and a tile of kPdTile b's; a workgroup strides over the work items.
//                The ids of a stay in registers for the tile (four rows a thread and step, one 8-byte load).  A pair runs
//                three phases over the rows with a barrier after each: add 1 to cell[id_a K_b + id_b]; read the cell back
//                and accumulate n - 1 (integer) and log2 n (float64, from the table); store 0 to the cell, so that the
//                table is clean for the next pair without a bulk clear.  sum_r (n(r) - 1) = 2 pairs_ab and
//                sum_r log2 n(r) = nlogn_ab, so there is no pass over the cells.  A thread keeps its keys in registers
//                between the phases, merges equal neighbours before it adds, and a wave whose 256 keys are all equal adds
//                once (the all-in-one pair would otherwise put 64 lanes on one address).  The table is in LDS (u32 cells,
//                kPdLdsCells of them) or in the workgroup's slice of a global workspace (kPdSliceCells cells, zeroed when
//                it was allocated): route_pd_table (route_calls.hpp) says which, per pair, from the two cluster counts; a
//                launch computes the pairs of its own route and leaves the others to the other launch.
// Bounds: an id is below its partition's cluster count K <= kPdMaxClusters by construction (k_pd_canon), so a key is below
// K_a K_b, which is at most kPdLdsCells on the LDS route and at most kPdSliceCells on the other.
// Determinism: a pair's float sum runs over the rows in an order and a tree that m alone fixes (the instantiation <T, NS>
// is chosen from m; thread t takes rows 4 (s T + t) .. + 3 for s ascending; then the xor tree of a wave; then the waves
// in order).  The terms are log2 n(r), and n(r) is the same for (a, b) and (b, a), on either route, in any tile.
#include <limits>

#include "device_error.hpp"
#include "launchers.hpp"

namespace msc {

constexpr int kPdCanonThreads = 256;
constexpr uint32_t kPdHash = 2 * kPdMaxClusters;            // k_pd_canon's hash table
constexpr uint32_t kPdNone = 0xFFFFFFFFu;

__device__ inline uint32_t pd_hash(uint32_t x) {
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x & (kPdHash - 1u);
}

__global__ __launch_bounds__(256) void k_pd_log2(double *__restrict__ tab, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i <= n) tab[i] = i == 0u ? 0.0 : log2((double)i);
}

// the workgroup's sums of v (integer) and x (float64) in every thread: the xor tree of a wave, then the waves in order
template <int WAVES>
__device__ inline void pd_block_sum(unsigned long long &v, double &x, unsigned long long *s_v, double *s_x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o), x += __shfl_xor(x, o);
  const uint32_t t = threadIdx.x;
  __syncthreads();                                           // (the last use of s_v, s_x is over)
  if ((t & 63u) == 0u) s_v[t >> 6] = v, s_x[t >> 6] = x;
  __syncthreads();
  v = s_v[0], x = s_x[0];
#pragma unroll
  for (int w = 1; w < WAVES; w++) v += s_v[w], x += s_x[w];
}

// lab: [n][ld] labels; ids: [n][ldi], ldi >= m (the tail is zeroed); k: [n] cluster counts (kPdBad: too many); the other
// outputs are nullable.  part0: the index of the first partition in its set (the detail of a reported error)
__global__ __launch_bounds__(kPdCanonThreads) void k_pd_canon(const int32_t *__restrict__ lab, uint64_t ld, uint32_t m,
                                                              const double *__restrict__ log2tab, uint32_t part0,
                                                              uint16_t *__restrict__ ids, uint64_t ldi,
                                                              uint32_t *__restrict__ k, int64_t *__restrict__ pairs,
                                                              double *__restrict__ nlogn, uint32_t *__restrict__ nclusters) {
  __shared__ unsigned long long s_key[kPdHash];              // the label (zero-extended), all ones = empty
  __shared__ uint32_t s_first[kPdHash];
  __shared__ uint16_t s_rank[kPdHash];
  __shared__ uint32_t s_n[kPdMaxClusters];
  __shared__ unsigned long long s_v[kPdCanonThreads / 64];
  __shared__ double s_x[kPdCanonThreads / 64];
  __shared__ uint32_t s_cnt, s_err;
  const uint32_t part = blockIdx.x;
  const uint32_t t = threadIdx.x;
  const int32_t *l = lab + (uint64_t)part * ld;
  uint16_t *out = ids + (uint64_t)part * ldi;
  for (uint32_t q = t; q < kPdHash; q += kPdCanonThreads) s_key[q] = ~0ull, s_first[q] = kPdNone;
  for (uint32_t q = t; q < kPdMaxClusters; q += kPdCanonThreads) s_n[q] = 0u;
  if (t == 0u) s_cnt = 0u, s_err = 0u;
  __syncthreads();
  for (uint32_t a = t; a < m; a += kPdCanonThreads) {
    if (*(volatile uint32_t *)&s_cnt > kPdMaxClusters) break;  // (already an error: do not fill the table)
    const unsigned long long key = (uint32_t)l[a];
    const uint32_t h = pd_hash((uint32_t)key);
    bool placed = false;
    for (uint32_t p = 0; p < kPdHash && !placed; p++) {
      const uint32_t slot = (h + p) & (kPdHash - 1u);
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
  if (s_err != 0u || s_cnt > kPdMaxClusters) {               // (uniform)
    for (uint32_t a = t; a < ldi; a += kPdCanonThreads) out[a] = 0;
    if (t == 0u) {
      report_device_error(MSC_DEVERR_DISTANCE_CLUSTERS, part0 + part);
      k[part] = kPdBad;
      if (pairs) pairs[part] = -1;
      if (nlogn) nlogn[part] = std::numeric_limits<double>::quiet_NaN();
      if (nclusters) nclusters[part] = kPdBad;
    }
    return;
  }
  for (uint32_t q = t; q < kPdHash; q += kPdCanonThreads) {
    const uint32_t f = s_first[q];
    if (f == kPdNone) continue;
    uint32_t r = 0u;
    for (uint32_t o = 0; o < kPdHash; o++) r += s_first[o] < f ? 1u : 0u;     // (kPdNone is never below)
    s_rank[q] = (uint16_t)r;                                 // < s_cnt <= kPdMaxClusters
  }
  __syncthreads();
  for (uint32_t a = t; a < ldi; a += kPdCanonThreads) {
    uint16_t id = 0;
    if (a < m) {
      const unsigned long long key = (uint32_t)l[a];
      const uint32_t h = pd_hash((uint32_t)key);
      for (uint32_t p = 0; p < kPdHash; p++) {               // (it is there: the walk ends at it)
        const uint32_t slot = (h + p) & (kPdHash - 1u);
        if (s_key[slot] == key) {
          id = s_rank[slot];
          break;
        }
      }
      atomicAdd(&s_n[id], 1u);
    }
    out[a] = id;
  }
  __syncthreads();
  unsigned long long v = 0ull;
  double x = 0.0;
  for (uint32_t q = t; q < kPdMaxClusters; q += kPdCanonThreads) {
    const uint32_t n = s_n[q];                               // <= m
    if (n == 0u) continue;
    v += (unsigned long long)n * (n - 1u) / 2u;
    x += (double)n * log2tab[n];
  }
  pd_block_sum<kPdCanonThreads / 64>(v, x, s_v, s_x);
  if (t == 0u) {
    k[part] = s_cnt;
    if (pairs) pairs[part] = (int64_t)v;
    if (nlogn) nlogn[part] = x;
    if (nclusters) nclusters[part] = s_cnt;
  }
}

// what this launch does with the pair (ai, bj) of its block: 0 nothing (the mirror image or the other route computes
// it), 1 compute, 2 write -1 / NaN (a partition with too many clusters; the LDS launch writes those)
template <bool LDS>
__device__ inline int pd_pair_state(const PdPairArgs &p, uint32_t ai, uint32_t bj, uint32_t ka, uint32_t kb) {
  if (p.mirror != 0u && p.b0 + bj < p.a0 + ai) return 0;
  if (ka == kPdBad || kb == kPdBad) return LDS ? 2 : 0;
  return (route_pd_table(ka, kb) == PdRoute::lds) == LDS ? 1 : 0;
}

template <int T, int NS, bool LDS>
__global__ __launch_bounds__(T) void k_pd_pairs(const PdPairArgs p) {
  constexpr int W = T / 64;
  __shared__ uint32_t s_tab[LDS ? kPdLdsCells : 1u];
  __shared__ unsigned long long s_np[kPdTile][W];
  __shared__ double s_lg[kPdTile][W];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  uint32_t *tab;
  if constexpr (LDS) {
    tab = s_tab;
    for (uint32_t q = t; q < kPdLdsCells; q += T) s_tab[q] = 0u;
    __syncthreads();
  } else {
    tab = p.table + (uint64_t)blockIdx.x * kPdSliceCells;    // (the launcher keeps the grid within the slices)
  }
  const uint32_t ntb = (p.nb + kPdTile - 1u) / kPdTile;
  const uint32_t total = p.na * ntb;
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t ai = w / ntb, j0 = (w % ntb) * kPdTile;
    const uint32_t nj = p.nb - j0 < kPdTile ? p.nb - j0 : kPdTile;
    const uint32_t ka = p.k_a[ai];
    const uint16_t *ra = p.ids_a + (uint64_t)ai * p.ldi;
    uint2 ida[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const uint32_t r0 = 4u * ((uint32_t)s * T + t);
      ida[s] = r0 < p.ldi ? *reinterpret_cast<const uint2 *>(ra + r0) : make_uint2(0u, 0u);
    }
    for (uint32_t jj = 0; jj < nj; jj++) {
      const uint32_t bj = j0 + jj;
      const uint32_t kb = p.k_b[bj];
      if (pd_pair_state<LDS>(p, ai, bj, ka, kb) != 1) continue;      // (uniform)
      const uint16_t *rb = p.ids_b + (uint64_t)bj * p.ldi;
      uint32_t key[NS][4];
      // phase 1: count
#pragma unroll
      for (int s = 0; s < NS; s++) {
        const uint32_t r0 = 4u * ((uint32_t)s * T + t);
        const uint2 idb = r0 < p.ldi ? *reinterpret_cast<const uint2 *>(rb + r0) : make_uint2(0u, 0u);
        const uint32_t a4[4] = {ida[s].x & 0xFFFFu, ida[s].x >> 16, ida[s].y & 0xFFFFu, ida[s].y >> 16};
        const uint32_t b4[4] = {idb.x & 0xFFFFu, idb.x >> 16, idb.y & 0xFFFFu, idb.y >> 16};
#pragma unroll
        for (int e = 0; e < 4; e++) key[s][e] = r0 + e < p.m ? a4[e] * kb + b4[e] : kPdNone;   // < ka kb, or none
        const uint32_t f = __builtin_amdgcn_readfirstlane(key[s][0]);
        if (__all(key[s][0] == f && key[s][1] == f && key[s][2] == f && key[s][3] == f)) {
          if (lane == 0u && f != kPdNone) atomicAdd(&tab[f], 256u);
        } else {
          uint32_t kcur = key[s][0], acc = 1u;
#pragma unroll
          for (int e = 1; e < 4; e++) {
            if (key[s][e] == kcur) {
              acc++;
            } else {
              if (kcur != kPdNone) atomicAdd(&tab[kcur], acc);
              kcur = key[s][e], acc = 1u;
            }
          }
          if (kcur != kPdNone) atomicAdd(&tab[kcur], acc);
        }
      }
      if constexpr (!LDS) __threadfence();
      __syncthreads();
      // phase 2: every row reads its cell back
      unsigned long long np = 0ull;
      double lg = 0.0;
#pragma unroll
      for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (key[s][e] == kPdNone) continue;
          uint32_t n;
          if constexpr (LDS)
            n = tab[key[s][e]];
          else
            n = __hip_atomic_load(&tab[key[s][e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          n = n < p.m ? n : p.m;                             // (1 <= n <= m: the table's extent, whatever the cell holds)
          np += n - 1u;
          lg += p.log2tab[n];
        }
      }
      __syncthreads();
      // phase 3: the table is clean again
#pragma unroll
      for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (key[s][e] == kPdNone) continue;
          if constexpr (LDS)
            tab[key[s][e]] = 0u;
          else
            __hip_atomic_store(&tab[key[s][e]], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o), lg += __shfl_xor(lg, o);
      if (lane == 0u) s_np[jj][wave] = np, s_lg[jj][wave] = lg;
      if constexpr (!LDS) __threadfence();
      __syncthreads();
    }
    __syncthreads();                                         // (a tile with no pair of this launch's has met no barrier)
    if (t < nj) {
      const uint32_t bj = j0 + t;
      const int state = pd_pair_state<LDS>(p, ai, bj, ka, p.k_b[bj]);
      if (state != 0) {
        int64_t pairs = -1;
        double nlogn = std::numeric_limits<double>::quiet_NaN();
        if (state == 1) {
          unsigned long long np = s_np[t][0];
          nlogn = s_lg[t][0];
#pragma unroll
          for (int wv = 1; wv < W; wv++) np += s_np[t][wv], nlogn += s_lg[t][wv];
          pairs = (int64_t)(np / 2ull);
        }
        const uint64_t gi = p.a0 + ai, gj = p.b0 + bj;
        if (p.pairs_ab) p.pairs_ab[gi * p.ldo + gj] = pairs;
        if (p.nlogn_ab) p.nlogn_ab[gi * p.ldo + gj] = nlogn;
        if (p.mirror != 0u && gi != gj) {
          if (p.pairs_ab) p.pairs_ab[gj * p.ldo + gi] = pairs;
          if (p.nlogn_ab) p.nlogn_ab[gj * p.ldo + gi] = nlogn;
        }
      }
    }
    __syncthreads();                                         // (s_np, s_lg are free for the next work item)
  }
}

int launch_pd_log2(hipStream_t stream, double *tab, uint32_t n) {
  if (n == 0 || n > kPdMaxRows) return -2;
  hipLaunchKernelGGL(k_pd_log2, dim3(n / 256u + 1u), dim3(256), 0, stream, tab, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pd_canon(hipStream_t stream, const int32_t *lab, uint64_t ld, uint32_t m, uint32_t nparts, const double *log2tab,
                    uint32_t part0, uint16_t *ids, uint64_t ldi, uint32_t *k, int64_t *pairs, double *nlogn,
                    uint32_t *nclusters) {
  if (nparts == 0 || m == 0 || m > kPdMaxRows || ld < m || ldi < m) return -2;
  hipLaunchKernelGGL(k_pd_canon, dim3(nparts), dim3(kPdCanonThreads), 0, stream, lab, ld, m, log2tab, part0, ids, ldi, k,
                     pairs, nlogn, nclusters);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int T, int NS, bool LDS>
static void pd_launch_pairs(hipStream_t stream, uint32_t grid, const PdPairArgs &p) {
  hipLaunchKernelGGL((k_pd_pairs<T, NS, LDS>), (note_kernel(2, "k_pd_pairs<%d, %d, %s>", T, NS, tf(LDS)), dim3(grid)),
                     dim3(T), 0, stream, p);
}

template <bool LDS>
static void pd_launch_pairs_for(hipStream_t stream, uint32_t grid, const PdPairArgs &p) {
  // <T, NS> from m alone: 4 T NS rows are the most an instantiation takes
  if (p.m <= 1024u)
    pd_launch_pairs<256, 1, LDS>(stream, grid, p);
  else if (p.m <= 4096u)
    pd_launch_pairs<1024, 1, LDS>(stream, grid, p);
  else if (p.m <= 16384u)
    pd_launch_pairs<1024, 4, LDS>(stream, grid, p);
  else
    pd_launch_pairs<1024, 8, LDS>(stream, grid, p);
}

int launch_pd_pairs(hipStream_t stream, int num_cus, PdRoute route, const PdPairArgs &p) {
  if (p.na == 0 || p.nb == 0 || p.m == 0 || p.m > kPdMaxRows || p.ldi < p.m || p.ldi % 4u != 0u ||
      (route == PdRoute::global && p.table == nullptr))
    return -2;
  const uint64_t total = (uint64_t)p.na * ((p.nb + kPdTile - 1u) / kPdTile);
  if (route == PdRoute::lds)
    pd_launch_pairs_for<true>(stream, (uint32_t)std::min<uint64_t>(total, 4ull * (uint64_t)std::max(num_cus, 1)), p);
  else
    pd_launch_pairs_for<false>(stream, (uint32_t)std::min<uint64_t>(total, kPdSlices), p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

MSC_DEFINE_BIND_ERROR_WORD(bind_error_word_distance)

}  // namespace msc
