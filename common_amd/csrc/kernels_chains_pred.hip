// kernels_chains_pred.hip -- msc_chains_sample_predictive: posterior predictive draws from the model average of an
// ensemble.  A row draws a chain with probability ~ w_c p(row's observed entries | state_c), a group of that chain
// ~ CRP term x likelihood of the observed entries, and its values from that group's predictive.  The chains' terms
// Lf[c][r] and normalised log weights lw_c are msc_chains_score_marginal's own (k_chains_marginal_prep, k_chains_marginal,
// run by the host into a scratch of the handle); what is here comes after them, one lane a row throughout:
//
//   k_chains_pick          walks the chains in ascending order three times (maximum, sum, running sum: chains_pick.hpp
//                          pick_index) over lw_c + Lf[c][r] -- coalesced reads of Lf's rows -- and writes the row's chain,
//                          or -1 for a row no chain of finite weight can hold.
//   k_chains_draw          the group draw against the CHOSEN chain's tables.  Neighbouring lanes hold different chains,
//                          so nothing is staged: a lane reads its chain's score tables from global memory through the
//                          chain's descriptors (MargChain::feats), batches of 8 or 32 groups at a time -- per feature
//                          the row's value and the table's address are formed once a batch.  A total is what
//                          k_chains_marginal forms for (chain, row, group): the features' scores added in ascending
//                          feature order, then the CRP term's lo, then its hi.  Pass one keeps (max, sum) of the K totals
//                          in double, pass two walks the running sum up to u2 * sum and stops at the batch that crosses it.
//                          What is the same in every chain -- a feature's family, dim, bound column, mask and the rows
//                          of its exact count table -- is read from member 0's descriptors with scalar loads.
//                          <LARGE, B>: LARGE holds the large-count forms of gp / bnb (seq_feature_score) and is launched
//                          only when a count column reaches past the exact table, as k_chains_marginal<true, .> is; B is
//                          the batch (<true, 8>, <false, 8>, <false, 32>).  The batch moves no bit: a total is summed per group, the groups are pushed in
//                          ascending order.
//   k_chains_values<HEAVY> the value draws of k_pred_sample, split the same way: <false> the copies of observed entries
//                          and the one-uniform draws (bb, dd), <true> the rejection families (gp, bnb, nich).  The
//                          group's predictive parameters are evaluated from the chain's raw tables and hp by
//                          pred_params.hpp's formulas -- the ones k_pred_prepare stores -- and the draws read the same
//                          Philox streams: the entries are msc_sample_predictive's, bit for bit.
// A row's results depend on the row alone; no atomics.
#include "chains_pick.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "pred_params.hpp"
#include "pred_samplers.hpp"
#include "score_block.hpp"
#include "seq_score.hpp"

namespace msc {

// groups a lane sums in registers at a time.  What a feature costs a lane apart from its table reads -- the descriptor's
// fields, the row's value, the chain's table address, each a load that waits for the one before -- is paid once a batch:
// kCpBatchWide from kCpWideFrom groups on, kCpBatch below (route_calls.hpp chains_draw_batch chooses; a batch reads
// whole, also past the last group).  Both divide the tables' row stride (kpad), so a batch never reads past a table row.
static_assert(kGroupTile % kCpBatch == 0 && kGroupTile % kCpBatchWide == 0, "a batch never reads past a table row");

__global__ __launch_bounds__(256) void k_chains_pick(const double *__restrict__ lw, const float *__restrict__ Lf, uint64_t ld,
                                                     uint32_t nchains, uint64_t nrows, uint64_t row_id0, uint64_t seed,
                                                     uint64_t sweep, int32_t *__restrict__ chain) {
  const uint64_t rel = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (rel >= nrows) return;
  double u1, u2;
  cpick::pick_uniforms(seed, row_id0 + rel, sweep, u1, u2);
  const float *mine = Lf + rel;
  chain[rel] = cpick::pick_index(nchains, u1, [=](uint32_t c) { return lw[c] + (double)mine[(size_t)c * ld]; });
}

// tv[j] = the total of (the lane's chain, row, group k0 + j), j < B; groups from K on are -inf.
// fl: the lane's chain's descriptors; f0: member 0's (uniform)
template <bool LARGE, int B>
MSC_DEV void cp_batch_totals(const FeatDesc *__restrict__ fl, const FeatDesc *__restrict__ f0, uint32_t nfeat,
                             const uint32_t *__restrict__ cnt, const float *__restrict__ crp, float e_hi, float e_lo,
                             uint32_t K, uint32_t kpad, uint64_t row, uint32_t k0, float (&tv)[B]) {
  float acc[B];
#pragma unroll
  for (int j = 0; j < B; j++) acc[j] = 0.f;
  for (uint32_t f = 0; f < nfeat; f++) {
    const FeatDesc &u = f0[f];
    const int fam = u.family;
    if (fam == MSC_NOOP || u.col == nullptr || load_masked<false>(u, row, true)) continue;   // (a masked entry adds nothing)
    const uint32_t v = load_raw_value<false>(u, 0, row, true);
    const float *tab = fl[f].tab + k0;
    if (fam == MSC_NICH) {
      const float x = __uint_as_float(v);
#pragma unroll
      for (int j = 0; j < B; j++)
        acc[j] += nich_eval(x, tab[(size_t)NICH_MU_HI * kpad + j], tab[(size_t)NICH_MU_LO * kpad + j],
                            tab[(size_t)NICH_C0 * kpad + j], tab[(size_t)NICH_C1LN2 * kpad + j],
                            tab[(size_t)NICH_C1 * kpad + j], tab[(size_t)NICH_C2 * kpad + j]);
      continue;
    }
    uint32_t r;
    if (fam == MSC_BB) {
      r = v != 0 ? 1u : 0u;
    } else if (fam == MSC_DD) {
      r = (int)v < 0 ? 0u : ((int)v >= (int)u.dim ? u.dim - 1u : v);
    } else {                                                 // gp, bnb
      if (LARGE && v >= u.vcap) {
        const double rowc = fam == MSC_GP ? gp_row_const(v) : 0.0;
#pragma unroll 1
        for (int j = 0; j < B; j++) {                 // (one copy of the large-count forms: they are long and rare)
          if (k0 + j >= K) break;
          const float sc = seq_feature_score(fl[f], v, k0 + j, kpad, rowc);
#pragma unroll
          for (int i2 = 0; i2 < B; i2++) acc[i2] = i2 == j ? acc[i2] + sc : acc[i2];   // (acc stays in registers)
        }
        continue;
      }
      r = (uint32_t)GP_T0 + (v < u.vcap ? v : u.vcap - 1u);
    }
    tab += (size_t)r * kpad;
#pragma unroll
    for (int j = 0; j < B; j++) acc[j] += tab[j];
  }
#pragma unroll
  for (int j = 0; j < B; j++) {
    const uint32_t k = k0 + j;                               // (< kpad: the tables' rows and the CRP table reach that far)
    const bool used = cnt[k] != 0u;
    const float hi = used ? crp[k] : e_hi, lo = used ? crp[crp_lo_cnt(kpad) + k] : e_lo;
    const float s = (acc[j] + lo) + hi;                      // the prior's lo first: the last add rounds the total once
    tv[j] = k < K ? s : -INFINITY;
  }
}

template <bool LARGE, int B>
__global__ __launch_bounds__(256) void k_chains_draw(const MargChain *__restrict__ chains, uint32_t nfeat, uint32_t K,
                                                     uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                                     uint64_t seed, uint64_t sweep, int32_t *__restrict__ chain,
                                                     int32_t *__restrict__ z) {
  const uint64_t rel = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (rel >= nrows) return;
  const int32_t c = chain[rel];
  if (c < 0) {
    z[rel] = -1;
    return;
  }
  const FeatDesc *f0 = chains[0].feats;
  const FeatDesc *fl = chains[c].feats;
  const uint32_t *cnt = chains[c].cnt;
  const float *crp = chains[c].crp;
  const float e_hi = crp[2 * (size_t)kpad], e_lo = crp[2 * (size_t)kpad + 2];
  const uint64_t row = row0 + rel;
  double u1, u2;
  cpick::pick_uniforms(seed, row_id0 + rel, sweep, u1, u2);
  float tv[B];
  cpick::Online on = cpick::online_start();
  for (uint32_t k0 = 0; k0 < K; k0 += B) {
    cp_batch_totals<LARGE, B>(fl, f0, nfeat, cnt, crp, e_hi, e_lo, K, kpad, row, k0, tv);
#pragma unroll
    for (int j = 0; j < B; j++) cpick::online_push(on, (double)tv[j]);
  }
  if (cpick::neg_inf(on.M) || !(on.S > 0.0)) {               // no group of the chain holds the row: skipped
    chain[rel] = -1;
    z[rel] = -1;
    return;
  }
  const double target = u2 * on.S;
  cpick::Running run = cpick::running_start();
  for (uint32_t k0 = 0; k0 < K && run.hit < 0; k0 += B) {
    cp_batch_totals<LARGE, B>(fl, f0, nfeat, cnt, crp, e_hi, e_lo, K, kpad, row, k0, tv);
#pragma unroll
    for (int j = 0; j < B; j++) cpick::running_push(run, (int32_t)(k0 + j), cpick::term((double)tv[j], on.M), target);
  }
  z[rel] = cpick::running_result(run);
}

MSC_DEV bool cp_heavy(int family) { return family == MSC_GP || family == MSC_BNB || family == MSC_NICH; }

// outs: one pointer a state feature (null: not drawn), entry `at + rel` is the row's
template <bool HEAVY>
__global__ __launch_bounds__(256) void k_chains_values(const MargChain *__restrict__ chains, void *const *__restrict__ outs,
                                                       uint32_t nfeat, uint32_t kpad, uint64_t row0, uint64_t nrows,
                                                       uint64_t row_id0, uint64_t at, const int32_t *__restrict__ chain,
                                                       const int32_t *__restrict__ z, uint32_t masked_only, uint64_t seed,
                                                       uint64_t sweep) {
  const uint64_t rel = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (rel >= nrows) return;
  const int32_t c = chain[rel], g = z[rel];
  if (c < 0 || g < 0) return;
  const FeatDesc *f0 = chains[0].feats;
  const FeatDesc *fl = chains[c].feats;
  const uint64_t vrow = row0 + rel, grow = row_id0 + rel, o = at + rel;
  const uint32_t k = (uint32_t)g;
  for (uint32_t f = 0; f < nfeat; f++) {
    void *out = outs[f];
    if (out == nullptr) continue;
    const FeatDesc &u = f0[f];
    const int fam = u.family;
    if (masked_only && !(u.mask != nullptr && u.mask[vrow] != 0)) {
      if (HEAVY) continue;
      switch (fam) {                                         // observed: the view's value, as the model reads it
        case MSC_BB: static_cast<uint8_t *>(out)[o] = static_cast<const uint8_t *>(u.col)[vrow] != 0; break;
        case MSC_NICH: static_cast<float *>(out)[o] = static_cast<const float *>(u.col)[vrow]; break;
        default: static_cast<uint32_t *>(out)[o] = static_cast<const uint32_t *>(u.col)[vrow]; break;
      }
      continue;
    }
    if (cp_heavy(fam) != HEAVY) continue;
    const float *hp = fl[f].hp;
    const uint32_t *ru = fl[f].raw_u32;
    pred::Stream s(seed, grow, sweep, f);
    if (!HEAVY) {
      if (fam == MSC_DD) {
        double total = 0.0;
        for (uint32_t i = 0; i < u.dim; i++) total += predpar::dd_weight(hp, ru, kpad, k, i);
        const double t = s.u24() * total;
        int32_t v = (int32_t)u.dim - 1;
        double cum = 0.0;
        for (uint32_t j = 0; j + 1 < u.dim; j++) {
          cum += predpar::dd_weight(hp, ru, kpad, k, j);
          if (t < cum) { v = (int32_t)j; break; }
        }
        static_cast<int32_t *>(out)[o] = v;
      } else {
        static_cast<uint8_t *>(out)[o] = s.u24() >= predpar::bb_p0(hp, ru, kpad, k) ? 1 : 0;   // bb
      }
      continue;
    }
    switch (fam) {
      case MSC_GP: {
        const predpar::Gp p = predpar::gp(hp, ru, kpad, k);
        static_cast<uint32_t *>(out)[o] = pred::poisson(s, pred::gamma1(s, p.shape) * p.scale);
        break;
      }
      case MSC_BNB: {
        const predpar::Bnb p = predpar::bnb(hp, ru, kpad, k);
        const double q = fmax(pred::beta(s, p.a, p.b), 1e-300);        // (a Beta draw that underflowed: no 1/0)
        const double rate = pred::gamma1(s, p.r) * (1.0 - q) / q;      // failures before the r-th success
        static_cast<uint32_t *>(out)[o] = pred::poisson(s, rate);
        break;
      }
      default: {
        const predpar::Nich p = predpar::nich(hp, ru, fl[f].raw_f32, kpad, k);
        static_cast<float *>(out)[o] = (float)(p.mu + p.scale * pred::student_t(s, p.nu));
        break;
      }
    }
  }
}

int launch_chains_pick(hipStream_t stream, const double *lw, const float *Lf, uint64_t ld, uint32_t nchains, uint64_t nrows,
                       uint64_t row_id0, uint64_t seed, uint64_t sweep, int32_t *chain) {
  if (nchains == 0 || nrows == 0 || nrows >= (1ull << 32) || ld < nrows)
    return fail(MSC_EHIP, "launch_chains_pick: a shape no route sends");
  hipLaunchKernelGGL(k_chains_pick, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, lw, Lf, ld, nchains, nrows,
                     row_id0, seed, sweep, chain);
  return launch_status("k_chains_pick");
}

int launch_chains_draw(hipStream_t stream, const MargChain *chains_dev, bool large, int batch, uint32_t nfeat, uint32_t K,
                       uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t seed, uint64_t sweep,
                       int32_t *chain, int32_t *z) {
  const bool wide = batch == kCpBatchWide;
  if (K == 0 || kpad < K || kpad % kCpBatchWide != 0 || nrows == 0 || nrows >= (1ull << 32) || (!wide && batch != kCpBatch) ||
      (wide && large))
    return fail(MSC_EHIP, "launch_chains_draw: a shape no route sends");
  const dim3 grid((unsigned)((nrows + 255) / 256));
#define MSC_CP_LAUNCH(LARGE, B)                                                                                            \
  hipLaunchKernelGGL((k_chains_draw<LARGE, B>), grid, dim3(256), 0, stream, chains_dev, nfeat, K, kpad, row0, nrows, row_id0, \
                     seed, sweep, chain, z)
  if (large) MSC_CP_LAUNCH(true, kCpBatch);          // (the large-count forms beside a wide batch spill)
  else if (wide) MSC_CP_LAUNCH(false, kCpBatchWide);
  else MSC_CP_LAUNCH(false, kCpBatch);
#undef MSC_CP_LAUNCH
  return launch_status("k_chains_draw");
}

int launch_chains_values(hipStream_t stream, const MargChain *chains_dev, void *const *outs_dev, bool light, bool heavy,
                         uint32_t nfeat, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t at,
                         const int32_t *chain, const int32_t *z, bool masked_only, uint64_t seed, uint64_t sweep) {
  if (nrows == 0 || nrows >= (1ull << 32)) return fail(MSC_EHIP, "launch_chains_values: a shape no route sends");
  const dim3 grid((unsigned)((nrows + 255) / 256));
  if (light)
    hipLaunchKernelGGL(k_chains_values<false>, grid, dim3(256), 0, stream, chains_dev, outs_dev, nfeat, kpad, row0, nrows,
                       row_id0, at, chain, z, masked_only ? 1u : 0u, seed, sweep);
  if (heavy)
    hipLaunchKernelGGL(k_chains_values<true>, grid, dim3(256), 0, stream, chains_dev, outs_dev, nfeat, kpad, row0, nrows,
                       row_id0, at, chain, z, masked_only ? 1u : 0u, seed, sweep);
  return launch_status("k_chains_values");
}

}  // namespace msc
