// kernels_chains_marginal.hip -- msc_chains_score_marginal: the posterior-averaged row predictive density over the chains
// of an ensemble,
//   mix[r] = logsumexp_c (lw_c + L[c][r]),   L[c][r] = logsumexp_k t_c[r][k] - log(n_c + alpha_c),
// t_c[r][k] what msc_score_value(.., MSC_SCORE_CRP_PRIOR) defines against chain c's tables over the SELECTED features.
// Neither the [chains x rows x K] totals nor (unless asked for) the [chains x rows] matrix L is written.
//
//   k_chains_marginal_prep    block c: log(n_c + alpha_c) of chain c and its normalised log weight lw_c (every block forms
//                             logsumexp(logw) for itself, in one fixed order: the same bits in every block and run).
//   k_chains_marginal         grid (row blocks of 256 x chain slices); one row per lane.  The workgroup walks its slice's
//                             chains in ascending order.  Per chain it stages TG groups of the chain's tables at a time in
//                             LDS -- the CRP term resolved to its (hi, lo) pair, then per selected feature bb 2 rows, dd
//                             dim, gp / bnb the exact table, nich the six constants, each row TS = TG | 1 floats apart so
//                             that lanes selecting different rows of a lookup table hit different banks -- and every lane
//                             takes the groups of the tile in batches of B = 32 (8 when a tile holds fewer): the features'
//                             scores summed per group in registers (seq_feature_score's arithmetic: table lookups,
//                             nich_eval, the beyond-the-table forms of gp and bnb from global memory), the prior added lo
//                             first, the batch pushed onto the lane's (max, sum) of the chain (chains_merge.hpp row_push).
//                             After the last tile L is finished in double and lw_c + L is pushed onto the lane's (M, S) of
//                             the slice (w_push).  A feature whose tables do not fit a tile of kCmMinTile groups beside the
//                             ones before it is read from global memory instead (route_calls.hpp plan_chains_marginal).
//                             The row's values are re-read per batch from the view's columns (the same few cache lines for
//                             every chain and tile: L1 / L2 hits), not staged: up to 256 features of 256 rows do not fit
//                             beside the tables, and a value is one coalesced load per B table reads.
//                             Instantiations: <LARGE, B>.  LARGE holds the large-count forms and runs one wave a SIMD;
//                             the launcher takes it only when a selected count column reaches past the exact table.
//                             With one slice the kernel rounds and writes mix itself; otherwise the slice's (M, S) goes to
//                             part[slice][row] and
//   k_chains_marginal_finish  merges a row's slices in ascending slice order (w_merge) and rounds once.
// A row's results depend on nothing but the row, the tile size and the slice cut, and the host derives those two from the
// ensemble and the bound view's rows alone (route_calls.hpp plan_chains_marginal, route_chains_marginal): a sub-range call gives the whole call's bits.
// No float atomics anywhere: the same bits on every run.
#include "chains_merge.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "score_block.hpp"
#include "seq_score.hpp"

namespace msc {

static_assert(NICH_ROWS == 6, "cm_table_rows (feat_desc.hpp) counts a nich block's rows");

__global__ __launch_bounds__(256) void k_chains_marginal_prep(const MargChain *__restrict__ chains, uint32_t nchains, uint32_t K,
                                                              const double *__restrict__ logw, double *__restrict__ lw,
                                                              double *__restrict__ norm) {
  __shared__ unsigned long long total;
  __shared__ double red[cmerge::kWRuns];
  static_assert(cmerge::kWRuns == 256, "one run a thread");
  __shared__ int bad_any;
  const uint32_t t = threadIdx.x, c = blockIdx.x;
  if (t == 0) {
    total = 0ull;
    bad_any = 0;
  }
  __syncthreads();
  const MargChain ch = chains[c];
  unsigned long long mine = 0ull;
  for (uint32_t k = t; k < K; k += 256) mine += ch.cnt[k];
  atomicAdd(&total, mine);                                  // (integers: any order gives the same sum)
  // logsumexp(logw) in chains_merge.hpp's order: strided runs, then a tree, for the maximum and again for the sum
  bool bad = false;
  red[t] = logw != nullptr ? cmerge::w_run_max(logw, nchains, t, bad) : 0.0;
  if (bad) atomicOr(&bad_any, 1);
  __syncthreads();
  for (uint32_t o = cmerge::kWRuns / 2; o > 0; o >>= 1) {
    cmerge::w_tree_step<true>(red, t, o);
    __syncthreads();
  }
  const double big = red[0];
  __syncthreads();
  red[t] = logw != nullptr ? cmerge::w_run_sum(logw, nchains, t, big) : 0.0;
  __syncthreads();
  for (uint32_t o = cmerge::kWRuns / 2; o > 0; o >>= 1) {
    cmerge::w_tree_step<false>(red, t, o);
    __syncthreads();
  }
  if (t == 0) {
    norm[c] = log((double)total + (double)ch.alpha);
    lw[c] = logw == nullptr ? -log((double)nchains) : cmerge::w_normalised(logw[c], big, red[0], bad_any != 0);
  }
}

// (kCmBatch / kCmBatchWide, the groups a lane sums in registers before it pushes them, and kCmNotStaged: route_calls.hpp)

// acc[j] += score_value of raw value v against the B groups whose table entries are b[row * stride + j]: b is a
// feature's block of the LDS tile (stride TS; entries past the tile's groups lie inside the allocation and are dropped by
// the caller) or its table in global memory (stride kpad; `live` entries only: the last table row ends with the table).
// gp / bnb: v is within the exact table (the caller takes the large-count forms elsewhere) -- clamped all the same.
template <bool GLOBAL, int B>
MSC_DEV void cm_batch_scores(const float *__restrict__ b, uint32_t stride, int fam, uint32_t dim, uint32_t vcap, uint32_t v,
                             uint32_t live, float (&acc)[B]) {
  if (fam == MSC_NICH) {
    const float x = __uint_as_float(v);
#pragma unroll 8
    for (int j = 0; j < B; j++) {
      if (GLOBAL && (uint32_t)j >= live) break;
      acc[j] += nich_eval(x, b[NICH_MU_HI * stride + j], b[NICH_MU_LO * stride + j], b[NICH_C0 * stride + j],
                          b[NICH_C1LN2 * stride + j], b[NICH_C1 * stride + j], b[NICH_C2 * stride + j]);
    }
    return;
  }
  uint32_t r = v < vcap ? v : vcap - 1u;                   // gp, bnb
  if (fam == MSC_BB) r = v != 0 ? 1u : 0u;
  else if (fam == MSC_DD) r = (int)v < 0 ? 0u : ((int)v >= (int)dim ? dim - 1u : v);
  b += (size_t)r * stride;
#pragma unroll
  for (int j = 0; j < B; j++) {
    if (GLOBAL && (uint32_t)j >= live) break;
    acc[j] += b[j];
  }
}

// LARGE: some selected gp / bnb column holds counts beyond the exact table (its vcap is the table's cap): those values take
// the large-count forms, which need some 280 registers a lane; the instantiation without them runs four waves a SIMD
template <bool LARGE, int B>
__global__ __launch_bounds__(256) void k_chains_marginal(const MargChain *__restrict__ chains, const MargFeat *__restrict__ plan,
                                                         uint32_t nsel, uint32_t nchains, uint32_t per_slice, uint32_t K,
                                                         uint32_t kpad, uint32_t TG, uint32_t TS, uint64_t row0, uint64_t nrows,
                                                         const double *__restrict__ lw, const double *__restrict__ norm,
                                                         float *__restrict__ mix, double *__restrict__ part) {
  extern __shared__ float tile[];     // [2 + staged rows][TS] + B: row 0 / 1 the prior's hi / lo, then the features' blocks
  const uint32_t t = threadIdx.x;
  const uint64_t rel = (uint64_t)blockIdx.x * 256 + t;
  const bool has = rel < nrows;
  const uint64_t row = row0 + (has ? rel : 0);
  const uint32_t c0 = blockIdx.y * per_slice, c1 = c0 + per_slice < nchains ? c0 + per_slice : nchains;
  cmerge::WPart w = cmerge::w_empty();
  for (uint32_t c = c0; c < c1; c++) {
    const MargChain ch = chains[c];
    const double lwc = lw[c];
    if (ch.logp == nullptr && cmerge::neg_inf(lwc)) continue;          // (uniform) a chain of weight -inf nobody asked for
    const float *crp = ch.crp;
    const float e_hi = crp[2 * (size_t)kpad], e_lo = crp[2 * (size_t)kpad + 2];
    cmerge::RowPart rp = cmerge::row_empty();
    for (uint32_t k0 = 0; k0 < K; k0 += TG) {
      const uint32_t tg = K - k0 < TG ? K - k0 : TG;
      __syncthreads();                                     // (every lane is done with the tile before)
      for (uint32_t j = t; j < tg; j += 256) {
        const bool used = ch.cnt[k0 + j] != 0u;
        tile[j] = used ? crp[k0 + j] : e_hi;
        tile[TS + j] = used ? crp[crp_lo_cnt(kpad) + k0 + j] : e_lo;
      }
      for (uint32_t i = 0; i < nsel; i++) {
        const MargFeat pf = plan[i];
        if (pf.off == kCmNotStaged) continue;
        const FeatDesc &fd = ch.feats[pf.f];
        const float *src = fd.tab + (size_t)(fd.family == MSC_GP || fd.family == MSC_BNB ? GP_T0 : 0) * kpad + k0;
        for (uint32_t e = t; e < pf.rows * tg; e += 256) {
          const uint32_t r = e / tg, j = e - r * tg;
          tile[pf.off + r * TS + j] = src[(size_t)r * kpad + j];
        }
      }
      __syncthreads();
      for (uint32_t j0 = 0; j0 < tg; j0 += B) {
        float acc[B];
#pragma unroll
        for (int j = 0; j < B; j++) acc[j] = 0.f;
        for (uint32_t i = 0; i < nsel; i++) {
          const MargFeat pf = plan[i];
          const FeatDesc &fd = ch.feats[pf.f];
          const int fam = fd.family;
          if (!has || fam == MSC_NOOP || fd.col == nullptr || load_masked(fd, row, true)) continue;   // (a masked entry adds nothing)
          const uint32_t v = load_raw_value<false>(fd, 0, row, true);
          const bool counts = fam == MSC_GP || fam == MSC_BNB;
          if (LARGE && counts && v >= fd.vcap) {
            const double rowc = fam == MSC_GP ? gp_row_const(v) : 0.0;
#pragma unroll 1
            for (int j = 0; j < B; j++) {           // (one copy of the large-count forms: they are long and rare)
              if (j0 + j >= tg) break;
              const float sc = seq_feature_score(fd, v, k0 + j0 + j, kpad, rowc);
#pragma unroll
              for (int i2 = 0; i2 < B; i2++) acc[i2] = i2 == j ? acc[i2] + sc : acc[i2];   // (acc stays in registers)
            }
          } else if (pf.off == kCmNotStaged) {
            cm_batch_scores<true, B>(fd.tab + (size_t)(counts ? GP_T0 : 0) * kpad + k0 + j0, kpad, fam, fd.dim, fd.vcap, v, tg - j0, acc);
          } else {
            cm_batch_scores<false, B>(tile + pf.off + j0, TS, fam, fd.dim, fd.vcap, v, B, acc);
          }
        }
        float tv[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
          const float s = (acc[j] + tile[TS + j0 + j]) + tile[j0 + j];   // the prior's lo first: the last add rounds the total once
          tv[j] = j0 + j < tg ? s : -INFINITY;
        }
        cmerge::row_push(rp, tv);
      }
    }
    const double L = cmerge::row_logp(rp, norm[c]);
    if (ch.logp != nullptr && has) ch.logp[rel] = (float)L;
    cmerge::w_push(w, lwc + L);
  }
  if (!has) return;
  if (part != nullptr) {
    double *p = part + 2 * ((size_t)blockIdx.y * nrows + rel);
    p[0] = w.M;
    p[1] = w.S;
  } else if (mix != nullptr) {
    mix[rel] = cmerge::w_finish(w);
  }
}

__global__ __launch_bounds__(256) void k_chains_marginal_finish(const double *__restrict__ part, uint32_t nslices,
                                                                uint64_t nrows, float *__restrict__ mix) {
  const uint64_t rel = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (rel >= nrows) return;
  cmerge::WPart w = cmerge::w_empty();
  for (uint32_t s = 0; s < nslices; s++) {
    const double *p = part + 2 * ((size_t)s * nrows + rel);
    w = cmerge::w_merge(w, cmerge::WPart{p[0], p[1]});
  }
  mix[rel] = cmerge::w_finish(w);
}

int launch_chains_marginal_prep(hipStream_t stream, const MargChain *chains_dev, uint32_t nchains, uint32_t K,
                                const double *logw, double *lw, double *norm) {
  hipLaunchKernelGGL(k_chains_marginal_prep, dim3(nchains), dim3(256), 0, stream, chains_dev, nchains, K, logw, lw, norm);
  return launch_status("k_chains_marginal_prep");
}

int launch_chains_marginal(hipStream_t stream, const MargChain *chains_dev, const MargFeat *plan_dev, uint32_t nsel,
                           const CmPlan &plan, uint32_t nchains, uint32_t nslices, uint32_t K, uint32_t kpad, uint64_t row0,
                           uint64_t nrows, const double *lw, const double *norm, float *mix, double *part) {
  if (nchains == 0 || nslices == 0 || nslices > kMaxGridYZ || K == 0 || plan.TG == 0 || plan.TS < plan.TG ||
      plan.lds_floats * sizeof(float) > 64u * 1024u || nrows == 0 || nrows >= (1ull << 32) || (nslices > 1 && mix && !part))
    return fail(MSC_EHIP, "launch_chains_marginal: a shape no route sends");
  const uint32_t per_slice = (nchains + nslices - 1) / nslices;
  const dim3 grid((unsigned)((nrows + 255) / 256), nslices);
  double *p = nslices > 1 && mix != nullptr ? part : nullptr;
#define MSC_CM_LAUNCH(LARGE, B)                                                                                              \
  hipLaunchKernelGGL((k_chains_marginal<LARGE, B>), grid, dim3(256), plan.lds_floats * sizeof(float), stream, chains_dev, plan_dev, \
                     nsel, nchains, per_slice, K, kpad, plan.TG, plan.TS, row0, nrows, lw, norm, mix, p)
  if (plan.large && plan.wide) MSC_CM_LAUNCH(true, kCmBatchWide);
  else if (plan.large) MSC_CM_LAUNCH(true, kCmBatch);
  else if (plan.wide) MSC_CM_LAUNCH(false, kCmBatchWide);
  else MSC_CM_LAUNCH(false, kCmBatch);
#undef MSC_CM_LAUNCH
  if (p != nullptr)
    hipLaunchKernelGGL(k_chains_marginal_finish, dim3(grid.x), dim3(256), 0, stream, p, nslices, nrows, mix);
  return launch_status("k_chains_marginal");
}

}  // namespace msc
