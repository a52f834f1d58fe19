// kernels_marginal.hip -- msc_score_marginal: a row's log posterior predictive density under the state,
//   logp[r] = logsumexp_k t[r][k] - log(n_r + alpha),   t[r][k] = what msc_score_value(.., MSC_SCORE_CRP_PRIOR) defines,
// with the arg-max group and its log responsibility on the way -- without ever writing the [N, K] matrix.  The scoring
// is the SCORE kernels' (the compensated logarithm, the prior as a (hi, lo) pair added lo first), not the sweeps'
// estimate: a draw forgives 1e-6 of a total, a density that is compared across models does not.
//
//   k_marginal_nich1<G>  one NICH feature, K <= 64 G: every per-group constant in VGPRs (lane l owns groups G l ..
//                        G l + G - 1), rows stream through four at a time; no LDS, no HBM traffic besides x, z and the
//                        4-12 bytes a row of results.  (the structure of k_sweep_nich1)
//   k_marginal_tile      any plan of scalar features, K <= 256: the workgroup tile of score_block.hpp (tables staged
//                        through LDS), reduced from registers.  (the structure of k_score_tile / k_sweep_tile)
//   k_row_lse            everything else: reduces rows of a score chunk that run_score (leave-one-out + prior) wrote
//                        to scratch.  (the shape of k_sample_rows)
// The reduction is lse_merge.hpp's: a lane forms the part (m, s, k) of its own entries, the wave merges the 64 parts.
// A row's result depends on nothing but the row: every launch shape gives the same bits.
#include "family_math.hpp"
#include "launchers.hpp"
#include "lse_merge.hpp"
#include "score_block.hpp"

namespace msc {

// ---- wavefront reductions on the DPP cross-lane path, FOUR values at a time -----------------------------------------
// "v_op_dpp v, v, v <ctrl>" computes op(moved v, v) in the lanes that have a source and leaves the others alone
// (kernels_sweep.hip MSC_DPP_REDUCE, where the why is written down).  A DPP read needs two wait states after a VALU
// write of its source: with four independent chains interleaved the other three instructions of a step are those wait
// states, so a step costs four issue slots for four rows where the one-value form pays three for one.  After the last
// step lane 63 holds the reduction over the wave.  All 64 lanes must be active.
#define MSC_DPP4_STEP(op, ctrl)                                                                   \
  op " %0, %0, %0 " ctrl "\n\t" op " %1, %1, %1 " ctrl "\n\t" op " %2, %2, %2 " ctrl "\n\t" op " %3, %3, %3 " ctrl "\n\t"
#define MSC_DPP4_REDUCE(op, a, b, c, d)                                                           \
  asm volatile("s_nop 1\n\t"                                                                      \
               MSC_DPP4_STEP(op, "row_shr:1 row_mask:0xf bank_mask:0xf")                          \
               MSC_DPP4_STEP(op, "row_shr:2 row_mask:0xf bank_mask:0xf")                          \
               MSC_DPP4_STEP(op, "row_shr:4 row_mask:0xf bank_mask:0xf")                          \
               MSC_DPP4_STEP(op, "row_shr:8 row_mask:0xf bank_mask:0xf")                          \
               MSC_DPP4_STEP(op, "row_bcast:15 row_mask:0xa bank_mask:0xf")                       \
               MSC_DPP4_STEP(op, "row_bcast:31 row_mask:0xc bank_mask:0xf")                       \
               "s_nop 1"                                                                          \
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d))

constexpr int kMargBatch = 4;         // rows reduced together

using lse::LanePart;      // (lse_merge.hpp: lane_part, lane_scaled_sum, lane_candidate -- what the host test builds too)
using lse::lane_part;
// the wave's merge of four rows' lane parts: afterwards m / s / k are the rows' maximum, total and arg-max (wave-uniform)
template <bool MAP>
MSC_DEV void merge_rows(LanePart (&p)[kMargBatch]) {
  float m0 = p[0].m, m1 = p[1].m, m2 = p[2].m, m3 = p[3].m;
  MSC_DPP4_REDUCE("v_max_f32_dpp", m0, m1, m2, m3);
  const float M[kMargBatch] = {lane_bcast(m0, 63), lane_bcast(m1, 63), lane_bcast(m2, 63), lane_bcast(m3, 63)};
  float s[kMargBatch];
  int k[kMargBatch];
#pragma unroll
  for (int i = 0; i < kMargBatch; i++) {
    s[i] = lse::lane_scaled_sum(p[i], M[i]);
    k[i] = lse::lane_candidate(p[i], M[i]);
  }
  MSC_DPP4_REDUCE("v_add_f32_dpp", s[0], s[1], s[2], s[3]);
  if (MAP) MSC_DPP4_REDUCE("v_min_i32_dpp", k[0], k[1], k[2], k[3]);
#pragma unroll
  for (int i = 0; i < kMargBatch; i++) {
    p[i].m = M[i];
    p[i].s = lane_bcast(s[i], 63);
    p[i].k = MAP ? lane_bcast(k[i], 63) : 0;
  }
}

// log(n + alpha) and log(n - 1 + alpha), n = the sum of the group counts: what a row's total is normalised by (the
// second when the row itself is counted in n and leaves for its own evaluation)
__global__ __launch_bounds__(256) void k_marginal_norm(const uint32_t *__restrict__ cnt, uint32_t K, float alpha,
                                                        double *__restrict__ norm) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0ull;
  __syncthreads();
  unsigned long long mine = 0ull;
  for (uint32_t k = threadIdx.x; k < K; k += 256) mine += cnt[k];
  atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)total;
    norm[0] = log(n + (double)alpha);
    norm[1] = log((n >= 1.0 ? n - 1.0 : 0.0) + (double)alpha);
  }
}

MSC_DEV void store_result(const LanePart &p, double log_norm, uint64_t at, float *__restrict__ logp,
                          int32_t *__restrict__ map, float *__restrict__ logresp) {
  const lse::Result r = lse::lse_finish<float>(p.m, p.s, log_norm);
  logp[at] = r.logp;
  if (map != nullptr) map[at] = p.k;
  if (logresp != nullptr) logresp[at] = r.logresp;
}

// ---------------------------------------------------------------------------
// single NICH feature, K <= 64 G
// ---------------------------------------------------------------------------
template <int G, bool MAP>
__global__ __launch_bounds__(256) void k_marginal_nich1(const FeatDesc *__restrict__ feats, uint32_t K, uint32_t kpad,
                                                         uint64_t row0, uint64_t nrows, const int32_t *__restrict__ z,
                                                         const float *__restrict__ crp, const double *__restrict__ norm,
                                                         int chunk_rows, float *__restrict__ logp,
                                                         int32_t *__restrict__ map, float *__restrict__ logresp) {
  const FeatDesc fd = feats[0];
  const int lane = threadIdx.x & 63;
  const int kb = G * lane;
  // per-group constants in registers for the whole kernel: the six rows of the score table and the prior's (hi, lo);
  // a group beyond K carries a prior of -inf, which is all its total ever is
  float mh[G], ml[G], c0[G], c1l[G], c1[G], sc[G], phi[G], plo[G];
  unsigned emask = 0u;                                     // bit j: group kb + j exists and is empty
#pragma unroll
  for (int j = 0; j < G; j++) {
    const uint32_t k = (uint32_t)(kb + j);
    const size_t kc = k < kpad ? k : 0;                    // (kpad >= 64 G only when K needs it)
    mh[j] = fd.tab[(size_t)NICH_MU_HI * kpad + kc];
    ml[j] = fd.tab[(size_t)NICH_MU_LO * kpad + kc];
    c0[j] = fd.tab[(size_t)NICH_C0 * kpad + kc];
    c1l[j] = fd.tab[(size_t)NICH_C1LN2 * kpad + kc];
    c1[j] = fd.tab[(size_t)NICH_C1 * kpad + kc];
    sc[j] = fd.tab[(size_t)NICH_C2 * kpad + kc];
    const float lc = crp[kc];
    const bool exists = k < K;
    if (exists && __builtin_isinf(lc)) emask |= 1u << j;
    phi[j] = exists ? lc : -INFINITY;
    plo[j] = exists ? crp[crp_lo_cnt(kpad) + kc] : 0.f;
  }
  const float le0 = crp[2 * (size_t)kpad], le1 = crp[2 * (size_t)kpad + 1];
  const float le0_lo = crp[2 * (size_t)kpad + 2], le1_lo = crp[2 * (size_t)kpad + 3];
  const double norm0 = norm[0], norm1 = norm[1];
  const float *xcol = reinterpret_cast<const float *>(fd.col) + row0;
  // a wave takes chunk_rows (<= 64) rows at a time, one per lane for the per-row setup and the finish, and streams them
  // past its groups four at a time
  const uint64_t nchunks = (nrows + chunk_rows - 1) / chunk_rows;
  const uint64_t wave_id = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * 4;
  for (uint64_t chunk = wave_id; chunk < nchunks; chunk += nwaves) {
    const uint64_t rb = chunk * chunk_rows;
    const int nr = __builtin_amdgcn_readfirstlane((int)((nrows - rb) < (uint64_t)chunk_rows ? (nrows - rb) : (uint64_t)chunk_rows));
    const bool has_row = lane < nr;
    const float xv = has_row ? xcol[rb + lane] : 0.0f;
    int gz = (has_row && z != nullptr) ? z[rb + lane] : -1;
    if ((uint32_t)gz >= K) gz = -1;                         // (an id outside the table: not assigned, as msc_accumulate reads it)
    const bool my_mask = fd.mask != nullptr && has_row && fd.mask[row0 + rb + lane] != 0;
    const unsigned long long mbits = __builtin_amdgcn_ballot_w64(my_mask);
    float sloo = 0.f, erow = le0, erow_lo = le0_lo;
    if (gz >= 0) {
      // leave-one-out score + prior of the row's own group: the sum k_loo_own forms (the prior's pair and the
      // feature's value added in double, rounded once)
      const float lm1 = crp[kpad + gz];
      const bool single = __builtin_isinf(lm1);             // the row is its group's only member
      double s = single ? (double)le1 + (double)le1_lo : (double)lm1 + (double)crp[crp_lo_cntm1(kpad) + gz];
      if (!my_mask) s += (double)nich_loo_tab_sweep(fd.hp, fd.loo64 + (size_t)gz * kNlooStride, 1, xv);
      sloo = (float)s;
      if (single) {
        erow = le1;
        erow_lo = le1_lo;
      }
    }
    LanePart res = {-INFINITY, 0.f, 0};
    for (int r0 = 0; r0 < nr; r0 += kMargBatch) {
      LanePart part[kMargBatch];
#pragma unroll
      for (int i = 0; i < kMargBatch; i++) {
        const int r = r0 + i;                               // (< 64; a row past nr is evaluated at x = 0 and dropped)
        const float x = lane_bcast(xv, r), eh = lane_bcast(erow, r), el = lane_bcast(erow_lo, r);
        const bool masked = ((mbits >> r) & 1ull) != 0;     // (wave-uniform) a masked value: only the prior speaks
        float t[G];
#pragma unroll
        for (int j = 0; j < G; j++) {
          float v = masked ? 0.f : nich_eval(x, mh[j], ml[j], c0[j], c1l[j], c1[j], sc[j]);
          const bool e = ((emask >> j) & 1u) != 0;
          v += e ? el : plo[j];                             // lo first: the last add then rounds the total once
          v += e ? eh : phi[j];
          t[j] = v;
        }
        const int g = lane_bcast(gz, r);
        if (g >= 0 && lane == g / G) {                      // the own group: its leave-one-out value
          const float sl = lane_bcast(sloo, r);
#pragma unroll
          for (int j = 0; j < G; j++)
            if (j == g % G) t[j] = sl;
        }
        part[i] = lane_part<G, MAP>(t, kb);
      }
      merge_rows<MAP>(part);
#pragma unroll
      for (int i = 0; i < kMargBatch; i++)
        if (lane == r0 + i) res = part[i];
    }
    if (has_row) store_result(res, gz >= 0 ? norm1 : norm0, rb + lane, logp, map, logresp);
  }
}

// ---------------------------------------------------------------------------
// any plan of scalar features, K <= 256: k_score_tile's sums (leave-one-out + prior) over the one k-tile, reduced from
// registers.  grid.x = row chunks of W * R rows (grid-stride), block = W waves.
// ---------------------------------------------------------------------------
template <int R, int W, bool MAP>
__global__ __launch_bounds__(W * 64, W / 4) void k_marginal_tile(const FeatDesc *__restrict__ feats, int nfeat, int nsplit,
                                                                  uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows,
                                                                  const int32_t *__restrict__ z, const float *__restrict__ own,
                                                                  const float *__restrict__ crp, const double *__restrict__ norm,
                                                                  float *__restrict__ logp, int32_t *__restrict__ map,
                                                                  float *__restrict__ logresp) {
  static_assert(R % kMargBatch == 0, "rows are reduced four at a time");
  __shared__ float4 lds[kGrpRows * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t kb = lane * 4;                            // single k-tile: K <= 256
  const uint64_t rows_per_wg = (uint64_t)W * R;
  const uint64_t nchunks = (nrows + rows_per_wg - 1) / rows_per_wg;
  for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const uint64_t rb = chunk * rows_per_wg + (uint64_t)wave * R;       // relative to row0
    const int nr = rb >= nrows ? 0 : (int)((nrows - rb) < (uint64_t)R ? (nrows - rb) : (uint64_t)R);
    int single = 0;                                       // lane r: removing row r empties its group
    if (z != nullptr && lane < nr) {
      const int g0 = z[rb + lane];
      single = g0 >= 0 && (uint32_t)g0 < K && __builtin_isinf(crp[kpad + g0]) ? 1 : 0;
    }
    // the prior is a (hi, lo) pair per group: the sums start from lo, hi is added after the last feature (k_score_tile,
    // where the why is written down); nothing but `single` is held across the tile scorer, which has no register to spare
    float4 acc[R];
    const bool tail_only = nsplit == 0;                    // (score_tile, SPLIT: the prior's lo part is added afterwards then)
    if (!tail_only) {
      const float4 hi0 = ld4(crp + kb), lo = ld4(crp + crp_lo_cnt(kpad) + kb);
      const float e0 = crp[2 * (size_t)kpad + 2], e1 = crp[2 * (size_t)kpad + 3];
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = crp_prior4_lo(hi0, lo, lane_bcast(single, r) ? e1 : e0);
    } else {
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = make_float4(0, 0, 0, 0);
    }
    score_tile<R, W, false, true>(feats, nfeat, nsplit, kpad, 0, lane, row0 + rb, nr, row0, lds, acc);
    const float *again = crp;                             // fetched again (an L2 hit per chunk) rather than held across
    asm volatile("" : "+s"(again));
    const float4 logcnt = ld4(again + kb);
    const float le0 = again[2 * (size_t)kpad], le1 = again[2 * (size_t)kpad + 1];
    if (tail_only) {
      const float4 lo = ld4(again + crp_lo_cnt(kpad) + kb);
      const float e0 = again[2 * (size_t)kpad + 2], e1 = again[2 * (size_t)kpad + 3];
#pragma unroll
      for (int r = 0; r < R; r++) add4(acc[r], crp_prior4_lo(logcnt, lo, lane_bcast(single, r) ? e1 : e0));
    }
    int gz = -1;
    float sloo = 0.f;
    if (z != nullptr && lane < nr) {
      gz = z[rb + lane];
      if ((uint32_t)gz >= K) gz = -1;                       // (an id outside the table: not assigned)
      if (gz >= 0) sloo = own[rb + lane];
    }
    LanePart res = {-INFINITY, 0.f, 0};
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += kMargBatch) {
      LanePart part[kMargBatch];
#pragma unroll
      for (int i = 0; i < kMargBatch; i++) {
        const int r = r0 + i;
        float4 s4 = acc[r];
        add4(s4, crp_prior4(logcnt, lane_bcast(single, r) ? le1 : le0));
        const int g = lane_bcast(gz, r);
        if (g >= 0) replace_own(s4, kb, g, lane_bcast(sloo, r));
        float t[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (kb + j >= K) t[j] = -INFINITY;
        part[i] = lane_part<4, MAP>(t, (int)kb);
      }
      merge_rows<MAP>(part);
#pragma unroll
      for (int i = 0; i < kMargBatch; i++)
        if (lane == r0 + i) res = part[i];
    }
    if (lane < nr) store_result(res, gz >= 0 ? norm[1] : norm[0], rb + lane, logp, map, logresp);
  }
}

// ---------------------------------------------------------------------------
// k_row_lse: a wave per row of a score chunk (ld floats a row, K of them used).  Every lane pushes the entries
// 4 lane + 256 i .. + 3 of its row in ascending order (lse_push, the sum in double: a run is K / 64 entries long), the 64
// parts are merged pairwise (lse_merge).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_row_lse(const float *__restrict__ scores, uint64_t ld, uint32_t K, uint64_t nrows,
                                                  const int32_t *__restrict__ z, const double *__restrict__ norm,
                                                  float *__restrict__ logp, int32_t *__restrict__ map,
                                                  float *__restrict__ logresp) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave_id = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * 4;
  const bool vec_ok = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0);
  for (uint64_t row = wave_id; row < nrows; row += nwaves) {
    const float *s = scores + row * ld;
    lse::Part<double> p = lse::lse_empty<double>();
    for (uint32_t k = 4u * (uint32_t)lane; k < K; k += (uint32_t)kGroupTile) {
      if (vec_ok && k + 3 < K) {
        const float4 v = ld4(s + k);
        lse::lse_push(p, v.x, (int32_t)k);
        lse::lse_push(p, v.y, (int32_t)k + 1);
        lse::lse_push(p, v.z, (int32_t)k + 2);
        lse::lse_push(p, v.w, (int32_t)k + 3);
      } else {
        for (uint32_t j = k; j < K && j < k + 4; j++) lse::lse_push(p, s[j], (int32_t)j);
      }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      lse::Part<double> q;
      q.m = __shfl_xor(p.m, off);
      q.s = __shfl_xor(p.s, off);
      q.k = __shfl_xor(p.k, off);
      p = (lane & off) ? lse::lse_merge(q, p) : lse::lse_merge(p, q);   // (the lower lanes' part first: the same sum on both sides)
    }
    if (lane == 0) {
      const bool assigned = z != nullptr && (uint32_t)z[row] < K;
      const lse::Result r = lse::lse_finish<double>(p.m, p.s, assigned ? norm[1] : norm[0]);
      logp[row] = r.logp;
      if (map != nullptr) map[row] = p.k;
      if (logresp != nullptr) logresp[row] = r.logresp;
    }
  }
}

// ---------------------------------------------------------------------------
static uint64_t grid_for(uint64_t work_items_per_wave_chunk, int num_cus, int waves_per_cu_cap) {
  uint64_t gx = (work_items_per_wave_chunk + 3) / 4;
  const uint64_t cap = (uint64_t)num_cus * waves_per_cu_cap / 4;
  if (gx > cap) gx = cap;
  return gx ? gx : 1;
}

int launch_marginal_norm(hipStream_t stream, const uint32_t *cnt, uint32_t K, float alpha, double *norm) {
  hipLaunchKernelGGL(k_marginal_norm, dim3(1), dim3(256), 0, stream, cnt, K, alpha, norm);
  return launch_status("k_marginal_norm");
}

int launch_marginal_nich1(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, uint32_t K, uint32_t kpad, uint64_t row0,
                          uint64_t nrows, const int32_t *z, const float *crp, const double *norm, float *logp, int32_t *map,
                          float *logresp) {
  if (K > 1024) return fail(MSC_EHIP, "launch_marginal_nich1: K = %u was routed here", K);
  // 64 rows per wave visit once there are enough rows for ~8 waves per SIMD; fewer rows: halve the visit down to 4
  // (every shape gives a row the same bits)
  int chunk_rows = 64;
  while (chunk_rows > 4 && (nrows + chunk_rows - 1) / chunk_rows < (uint64_t)num_cus * 32) chunk_rows >>= 1;
  const dim3 grid((unsigned)grid_for((nrows + chunk_rows - 1) / chunk_rows, num_cus, 16)), block(256);
  const bool want = map != nullptr || logresp != nullptr;
#define MSC_MARG_NICH1(G)                                                                                              \
  do {                                                                                                                 \
    if (want)                                                                                                          \
      hipLaunchKernelGGL((k_marginal_nich1<G, true>), (note_kernel(3, "k_marginal_nich1<" #G ", true>"), grid), block, 0, stream, \
                         feats_dev, K, kpad, row0, nrows, z, crp, norm, chunk_rows, logp, map, logresp);               \
    else                                                                                                               \
      hipLaunchKernelGGL((k_marginal_nich1<G, false>), (note_kernel(3, "k_marginal_nich1<" #G ", false>"), grid), block, 0, stream, \
                         feats_dev, K, kpad, row0, nrows, z, crp, norm, chunk_rows, logp, map, logresp);               \
  } while (0)
  if (K <= 64) MSC_MARG_NICH1(1);
  else if (K <= 128) MSC_MARG_NICH1(2);
  else if (K <= 256) MSC_MARG_NICH1(4);
  else if (K <= 512) MSC_MARG_NICH1(8);
  else MSC_MARG_NICH1(16);
#undef MSC_MARG_NICH1
  return launch_status("k_marginal_nich1");
}

int launch_marginal_tile(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K,
                         uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z, const float *own, const float *crp,
                         const double *norm, float *logp, int32_t *map, float *logresp) {
  if (K > 256) return fail(MSC_EHIP, "launch_marginal_tile: K = %u was routed here", K);
  const uint64_t cap = (uint64_t)num_cus * 4;
  const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nrows + 127) / 128, cap)));
  if (map != nullptr || logresp != nullptr)
    hipLaunchKernelGGL((k_marginal_tile<8, 16, true>), (note_kernel(3, "k_marginal_tile<8, 16, true>"), grid), dim3(1024), 0, stream,
                       feats_dev, nfeat, nsplit, K, kpad, row0, nrows, z, own, crp, norm, logp, map, logresp);
  else
    hipLaunchKernelGGL((k_marginal_tile<8, 16, false>), (note_kernel(3, "k_marginal_tile<8, 16, false>"), grid), dim3(1024), 0, stream,
                       feats_dev, nfeat, nsplit, K, kpad, row0, nrows, z, own, crp, norm, logp, map, logresp);
  return launch_status("k_marginal_tile");
}

int launch_row_lse(hipStream_t stream, int num_cus, const float *scores, uint64_t ld, uint32_t K, uint64_t nrows,
                   const int32_t *z, const double *norm, float *logp, int32_t *map, float *logresp) {
  const uint64_t gx = grid_for(nrows, num_cus, 32);
  hipLaunchKernelGGL(k_row_lse, (note_kernel(3, "k_row_lse"), dim3((unsigned)gx)), dim3(256), 0, stream, scores, ld, K, nrows, z,
                     norm, logp, map, logresp);
  return launch_status("k_row_lse");
}

}  // namespace msc
