// kernels_chains_sm.hip -- split-merge proposals for every chain of an ensemble in one launch (msc_chains_split_merge,
// include/microscopes_hip.h).  The move is msc_split_merge's, step for step (kernels_splitmerge.hip,
// splitmerge_math.hpp: the same streams, the same arithmetic), in the shape of k_sweep_seq_chains:
//   k_sm_chains   a grid of workgroups, workgroup c carries chain c (an SmChain entry of a device table) through proposals
//                 [p0, p1) of the call, whole proposals only, and keeps every table of the chain's state current itself.
// One proposal, the phases separated by __syncthreads.  Row r belongs to thread r % 256 in EVERY phase, so a row's label
// (ell, the handle's scratch) and its z entry are read and written by one thread only and need no barrier of their own.
//   anchors   the lowest empty slot and the number of empty slots from the chain's count table (all threads), sm::anchors
//             and the kind (thread 0).  Void: the log row, the counters, the outputs' rows, and theta as msc_split_merge
//             leaves it (the last pass's draw from two empty slots); nothing of the chain's state is written.
//   coins     ell[r] = -1 outside S, 0 / 1 at the anchors, the coin of k_sm_coins elsewhere
//   passes t = 0 .. launch_iters:
//     stats   the pair slots' suff-stats from ell, feature after feature: a thread sums its rows r = t, t + 256, ... in
//             that order into registers, the lanes of a wave combine by shuffles (offset 32, 16, ... 1), thread 0 adds the
//             waves' sums in wave order.  THAT IS THE ORDER OF EVERY DOUBLE SUM (nich sum x and sum x^2, gp sum ln
//             Gamma(v + 1)): fixed by the row count alone, so a call repeats its bits.  The integer sums take the same
//             route (dd: atomics on the pair's own table; any order gives the same integers).  Thread 0 stores the sums in
//             the pair state's additive tables and runs commit_group on the slots.
//     draws   one thread a (feature, slot): blk_draw_slot; the last thread the K = 2 stick: blk_stick_slot for slot 0,
//             slot 1 the last slot -- the bits k_blocked_sticks gives at K = 2 (blocked_draw.hpp)
//     labels  blk_tile_scores<MODE_GLOBAL> of the row, sm::two_way, the label dart; the final pass draws for a split and
//             takes [z = z_j] for a merge, and sums log q over the free rows in double in the order above
//   decide    the stats once more under the final labels, slot 2 = slot 0 + slot 1 in the additive tables;
//             score_data_group of every (feature, slot) rounded to float (what k_score_data stores), added in feature
//             order in double by thread 0; sm::log_accept, the dart, the log row, the counters
//   apply     (accepted) z of the label-1 rows; the two groups' additive sums taken from the pair slots -- a split gives
//             g_i slot 0's and the empty slot slot 1's, a merge gives g_i the union's and zeroes g_j -- then what seq_move
//             does for a row, for the whole group: commit_group, the counts, the two groups' CRP terms and the empty-slot
//             terms, and prepare_group of every (feature, slice)
#include "blocked_draw.hpp"
#include "blocked_score.hpp"
#include "commit_ops.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "splitmerge_math.hpp"

namespace msc {

constexpr uint32_t kSmcWaves = kSmChainsThreads / 64;

struct SmcShared {
  SmProp prop;
  uint32_t lowest, nempty, accepted, pad;
  unsigned long long wi[2][kSmcWaves][4];   // the waves' integer sums of a feature (two features in flight)
  double wd[2][kSmcWaves][4];               // ... and their double sums
  double wq[kSmcWaves];                     // the waves' log q
  float sd[3 * kSeqMaxFeat];                // score_data [feature][slot]
};

MSC_DEV void smc_split(double v, float &hi, float &lo) {      // (kernels_seq.hip seq_split: -inf has no lo part)
  hi = (float)v;
  lo = __builtin_isinf(hi) ? 0.f : (float)(v - (double)hi);
}

template <typename T>
MSC_DEV T smc_wave_sum(T v) {                                  // lane 0 holds the wave's sum: offsets 32, 16, ... 1
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The two pair slots' suff-stats of one feature from the labels (fd null: the pair's group counts), stored in the pair
// state's additive tables and committed; with_union: slot 2 = slot 0 + slot 1 as well.  -> whether half `par` of sh.wi /
// sh.wd was used: thread 0 may still read it when the call returns, so the next call that uses a half must take the other
// one (a noop feature and a dd feature use none).  The caller ends the phase with a barrier (smc_all_stats).
MSC_DEV bool smc_stats(SmcShared &sh, uint32_t par, const FeatDesc *fd, long long *pcnt_acc, uint32_t *pcnt_u32, uint32_t pk,
                       uint64_t nrows, const int32_t *ell, bool with_union) {
#pragma clang fp contract(off)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const int fam = fd != nullptr ? fd->family : -1;
  if (fd != nullptr && (fd->col == nullptr || (fam != MSC_BB && fam != MSC_GP && fam != MSC_BNB && fam != MSC_DD && fam != MSC_NICH)))
    return false;                                              // (uniform: noop has no tables)
  if (fam == MSC_DD) {
    const uint32_t dim = fd->dim;
    for (uint32_t i = t; i < dim; i += kSmChainsThreads) fd->acc_i64[(size_t)i * pk] = fd->acc_i64[(size_t)i * pk + 1] = 0;
    __syncthreads();
    const int32_t *col = static_cast<const int32_t *>(fd->col);
    for (uint64_t r = t; r < nrows; r += kSmChainsThreads) {
      const int32_t lab = ell[r];
      if (lab < 0 || (fd->mask != nullptr && fd->mask[r] != 0)) continue;
      const int32_t v = col[r];
      if (v >= 0 && (uint32_t)v < dim)
        atomicAdd(reinterpret_cast<unsigned long long *>(&fd->acc_i64[(size_t)v * pk + (uint32_t)lab]), 1ull);
    }
    __syncthreads();
    if (with_union)
      for (uint32_t i = t; i < dim; i += kSmChainsThreads)
        fd->acc_i64[(size_t)i * pk + 2] = fd->acc_i64[(size_t)i * pk] + fd->acc_i64[(size_t)i * pk + 1];
    __syncthreads();
    if (t < (with_union ? 3u : 2u)) commit_group(*fd, t, pk);
    __syncthreads();
    return false;
  }
  unsigned long long a[2] = {0ull, 0ull}, b[2] = {0ull, 0ull};
  double d[2] = {0.0, 0.0}, e[2] = {0.0, 0.0};
  for (uint64_t r = t; r < nrows; r += kSmChainsThreads) {
    const int32_t lab = ell[r];
    if (lab < 0) continue;
    const uint32_t s = lab != 0 ? 1u : 0u;
    if (fd == nullptr) {
      if (s) a[1]++; else a[0]++;
      continue;
    }
    if (fd->mask != nullptr && fd->mask[r] != 0) continue;      // masked value: not part of the group
    switch (fam) {
      case MSC_BB:
        if (static_cast<const uint8_t *>(fd->col)[r] != 0) { if (s) a[1]++; else a[0]++; }
        else { if (s) b[1]++; else b[0]++; }
        break;
      case MSC_GP: {
        const uint32_t v = static_cast<const uint32_t *>(fd->col)[r];
        const double lf = log_factorial(v);
        if (s) a[1]++, b[1] += v, d[1] += lf; else a[0]++, b[0] += v, d[0] += lf;
      } break;
      case MSC_BNB: {
        const uint32_t v = static_cast<const uint32_t *>(fd->col)[r];
        if (s) a[1]++, b[1] += v; else a[0]++, b[0] += v;
      } break;
      default: {                                               // nich
        const double x = static_cast<const float *>(fd->col)[r];
        const double xx = x * x;
        if (s) a[1]++, d[1] += x, e[1] += xx; else a[0]++, d[0] += x, e[0] += xx;
      } break;
    }
  }
#pragma unroll
  for (int s = 0; s < 2; s++) {
    a[s] = smc_wave_sum(a[s]);
    b[s] = smc_wave_sum(b[s]);
    d[s] = smc_wave_sum(d[s]);
    e[s] = smc_wave_sum(e[s]);
  }
  if (lane == 0) {
    sh.wi[par][wave][0] = a[0], sh.wi[par][wave][1] = a[1], sh.wi[par][wave][2] = b[0], sh.wi[par][wave][3] = b[1];
    sh.wd[par][wave][0] = d[0], sh.wd[par][wave][1] = d[1], sh.wd[par][wave][2] = e[0], sh.wd[par][wave][3] = e[1];
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long A[3] = {0, 0, 0}, B[3] = {0, 0, 0};
    double D[3] = {0.0, 0.0, 0.0}, E[3] = {0.0, 0.0, 0.0};
    for (uint32_t w = 0; w < kSmcWaves; w++)
      for (int s = 0; s < 2; s++) {
        A[s] += sh.wi[par][w][s];
        B[s] += sh.wi[par][w][2 + s];
        D[s] += sh.wd[par][w][s];
        E[s] += sh.wd[par][w][2 + s];
      }
    A[2] = A[0] + A[1], B[2] = B[0] + B[1], D[2] = D[0] + D[1], E[2] = E[0] + E[1];
    const uint32_t ns = with_union ? 3u : 2u;
    for (uint32_t s = 0; s < ns; s++) {
      if (fd == nullptr) {
        pcnt_acc[s] = (long long)A[s];
        pcnt_u32[s] = (uint32_t)A[s];
        continue;
      }
      fd->acc_i64[s] = (long long)A[s];
      if (fam != MSC_NICH) fd->acc_i64[pk + s] = (long long)B[s];
      if (fam == MSC_GP) fd->acc_f64[s] = D[s];
      if (fam == MSC_NICH) fd->acc_f64[s] = D[s], fd->acc_f64[pk + s] = E[s];
      commit_group(*fd, s, pk);
    }
  }
  // (no barrier here: the next call that uses wi / wd writes their other half -- one barrier, the one above, then lies
  // between this read and the next write of this half -- and the caller ends the phase with one)
  return true;
}

// all features' stats and the pair's counts; every table of the pair slots written on return
MSC_DEV void smc_all_stats(SmcShared &sh, const FeatDesc *pfeats, int nfeat, long long *pcnt_acc, uint32_t *pcnt_u32, uint32_t pk,
                           uint64_t nrows, const int32_t *ell, bool with_union) {
  uint32_t par = 0;                                            // the half the next user of wi / wd takes
  for (int f = -1; f < nfeat; f++)
    if (smc_stats(sh, par, f < 0 ? nullptr : &pfeats[f], pcnt_acc, pcnt_u32, pk, nrows, ell, with_union)) par ^= 1u;
  __syncthreads();
}

// group g of the chain's feature d takes pair slot `slot` of the pair's feature s (slot < 0: empties); fields follow
MSC_DEV void smc_install(const FeatDesc &d, const FeatDesc &s, uint32_t kpad, uint32_t pk, uint32_t g, int slot) {
  uint32_t ni = 0, nf = 0;
  switch (d.family) {
    case MSC_BB:
    case MSC_BNB: ni = 2; break;
    case MSC_GP: ni = 2, nf = 1; break;
    case MSC_DD: ni = d.dim; break;
    case MSC_NICH: ni = 1, nf = 2; break;
    default: return;
  }
  for (uint32_t r = 0; r < ni; r++) d.acc_i64[(size_t)r * kpad + g] = slot < 0 ? 0ll : s.acc_i64[(size_t)r * pk + (uint32_t)slot];
  for (uint32_t r = 0; r < nf; r++) d.acc_f64[(size_t)r * kpad + g] = slot < 0 ? 0.0 : s.acc_f64[(size_t)r * pk + (uint32_t)slot];
  commit_group(d, g, kpad);
}

// The pair slots' parameters and the K = 2 stick from the pair state's fields, under the pass's key.  (msc_split_merge
// hands launch_blocked_draw this key ^ blocked::kKey as its seed, and the launcher's own ^ kKey takes it off again: the
// draws run under the pass's key itself, as splitmerge_math.hpp states.)
MSC_DEV void smc_draws(const BlkFeat *pblk, int nfeat, uint32_t pk, uint64_t key, uint64_t sw, const uint32_t *pcnt_u32,
                       float alpha, float *ptab) {
  const uint32_t t = threadIdx.x, nt = kSmChainsThreads;
  for (uint32_t i = t; i < 2u * (uint32_t)nfeat; i += nt) {
    const BlkFeat &bf = pblk[i >> 1];
    if (bf.nslices != 0) blk_draw_slot(bf, i & 1u, pk, key, sw, ptab);
  }
  if (t == nt - 1) {
    double lv0, l10, lv1, l11;
    blk_stick_slot((double)pcnt_u32[0], (double)pcnt_u32[1], (double)alpha, key, 0u, sw, false, &lv0, &l10);
    blk_stick_slot((double)pcnt_u32[1], 0.0, (double)alpha, key, 1u, sw, true, &lv1, &l11);
    ptab[0] = blocked::fin(lv0 + 0.0);
    ptab[1] = blocked::fin(lv1 + l10);
  }
}

__global__ __launch_bounds__(kSmChainsThreads) void k_sm_chains(const SmChain *__restrict__ chains, int nfeat, uint32_t K,
                                                                uint32_t kpad, uint32_t pk, uint64_t nrows, uint64_t row_id0,
                                                                uint32_t p0, uint32_t p1, uint32_t launch_iters,
                                                                uint64_t sweep) {
  __shared__ SmcShared sh;
  const SmChain &c = chains[blockIdx.x];
  const FeatDesc *feats = c.feats, *pfeats = c.pair_feats;
  const BlkFeat *pblk = c.pair_blk;
  float *ptab = c.pair_tab, *crp = c.crp;
  long long *cnt_acc = c.cnt_acc, *pcnt_acc = c.pair_cnt_acc;
  uint32_t *cnt_u32 = c.cnt_u32, *pcnt_u32 = c.pair_cnt_u32;
  int32_t *z = c.z, *ell = c.ell;
  const uint64_t seed = c.seed;
  const float alpha = c.alpha;
  const uint32_t t = threadIdx.x, nt = kSmChainsThreads, lane = t & 63u, wave = t >> 6;

  for (uint32_t pi = p0; pi < p1; pi++) {
    const uint64_t sw = sweep + pi;
    int32_t *proposed = c.proposed != nullptr ? c.proposed + (size_t)pi * nrows : nullptr;
    int32_t *trace = c.trace != nullptr ? c.trace + (size_t)pi * nrows : nullptr;
    double *log_row = c.log != nullptr ? c.log + (size_t)pi * 8 : nullptr;
    // ---- anchors ----
    if (t == 0) sh.lowest = K, sh.nempty = 0;
    __syncthreads();
    {
      uint32_t mine = K, empties = 0;
      for (uint32_t k = t; k < K; k += nt)
        if (cnt_u32[k] == 0) {
          if (mine == K) mine = k;
          empties++;
        }
      if (mine < K) atomicMin(&sh.lowest, mine);
      if (empties) atomicAdd(&sh.nempty, empties);
    }
    __syncthreads();
    if (t == 0) {
      SmProp p;
      p.gi = p.gj = p.target = -1;
      p.kind = sm::kVoid;
      p.i = p.j = 0;
      p.accepted = 0;
      p.pad = 0;
      if (nrows >= 2) {
        sm::anchors(sm::stream_key(seed, sm::kStreamProposal), sw, nrows, &p.i, &p.j);
        const int32_t gi = z[p.i], gj = z[p.j];
        if (gi >= 0 && (uint32_t)gi < K && gj >= 0 && (uint32_t)gj < K) {
          p.gi = gi;
          p.gj = gj;
          if (gi != gj) {
            p.kind = sm::kMerge;
            p.target = gi;
          } else if (sh.lowest < K) {
            p.kind = sm::kSplit;
            p.target = (int32_t)sh.lowest;
          }
        }
      }
      sh.prop = p;
    }
    __syncthreads();
    const SmProp p = sh.prop;
    if (p.kind == sm::kVoid) {                          // (uniform)
      // theta of a void proposal is what msc_split_merge leaves: the last pass's draw from two empty slots (the prior)
      for (uint64_t r = t; r < nrows; r += nt) ell[r] = -1;
      smc_all_stats(sh, pfeats, nfeat, pcnt_acc, pcnt_u32, pk, nrows, ell, false);
      smc_draws(pblk, nfeat, pk, sm::stream_key(seed, sm::kStreamPass0 + launch_iters), sw, pcnt_u32, alpha, ptab);
      if (proposed != nullptr)
        for (uint64_t r = t; r < nrows; r += nt) proposed[r] = -1;
      if (trace != nullptr)
        for (uint64_t r = t; r < nrows; r += nt) trace[r] = z[r];
      if (t == 0) {
        if (log_row != nullptr) {
          log_row[0] = (double)p.i, log_row[1] = (double)p.j, log_row[2] = (double)p.kind;
          log_row[3] = log_row[4] = log_row[5] = log_row[6] = log_row[7] = 0.0;
        }
        if (c.counters != nullptr) c.counters[4] += 1ull;
      }
      continue;
    }
    // ---- coins ----
    {
      const uint64_t key = sm::stream_key(seed, sm::kStreamCoin);
      for (uint64_t r = t; r < nrows; r += nt) {
        const int32_t zr = z[r];
        int32_t lab = -1;
        if (zr == p.gi || zr == p.gj) lab = r == p.i ? 0 : r == p.j ? 1 : sm::uniform01(key, sw, row_id0 + r) >= 0.5f ? 1 : 0;
        ell[r] = lab;
      }
    }
    // ---- passes ----
    double logq = 0.0;
    for (uint32_t pass = 0; pass <= launch_iters; pass++) {
      const bool final = pass == launch_iters;
      smc_all_stats(sh, pfeats, nfeat, pcnt_acc, pcnt_u32, pk, nrows, ell, false);
      const uint64_t key = sm::stream_key(seed, sm::kStreamPass0 + pass);
      smc_draws(pblk, nfeat, pk, key, sw, pcnt_u32, alpha, ptab);
      __syncthreads();
      double lq = 0.0;
      for (uint64_t r = t; r < nrows; r += nt) {
        int32_t lab = ell[r];
        if (lab < 0) continue;
        float s[kBlkTile];
        blk_tile_scores<MODE_GLOBAL>(pblk, nfeat, ptab, pk, 0, nullptr, 0, r, kBlkMasked, s);
        float lp0, lp1, pr0;
        sm::two_way(s[0], s[1], &lp0, &lp1, &pr0);
        const bool free_row = r != p.i && r != p.j;
        if (final && p.kind == sm::kMerge) lab = z[r] == p.gj ? 1 : 0;
        else if (!free_row) lab = r == p.j ? 1 : 0;
        else lab = sm::uniform01(key, sw, row_id0 + r) < pr0 ? 0 : 1;
        ell[r] = lab;
        if (final && free_row) lq += (double)(lab ? lp1 : lp0);
      }
      if (final) {
        lq = smc_wave_sum(lq);
        if (lane == 0) sh.wq[wave] = lq;
        __syncthreads();
        for (uint32_t w = 0; w < kSmcWaves; w++) logq += sh.wq[w];
      }
    }
    if (proposed != nullptr)
      for (uint64_t r = t; r < nrows; r += nt) proposed[r] = ell[r];
    // ---- decide ----
    smc_all_stats(sh, pfeats, nfeat, pcnt_acc, pcnt_u32, pk, nrows, ell, true);
    for (uint32_t i = t; i < 3u * (uint32_t)nfeat; i += nt) sh.sd[i] = (float)score_data_group(pfeats[i / 3u], i % 3u, pk);
    __syncthreads();
    if (t == 0) {
      double tot[3] = {0.0, 0.0, 0.0};
      for (uint32_t slot = 0; slot < 3; slot++)
        for (uint32_t f = 0; f < (uint32_t)nfeat; f++) tot[slot] += (double)sh.sd[f * 3u + slot];
      const double n0 = (double)pcnt_u32[0], n1 = (double)pcnt_u32[1];
      const double logA = sm::log_accept(p.kind, log((double)alpha), n0, n1, tot[0], tot[1], tot[2], logq);
      const double u = (double)sm::uniform01(sm::stream_key(seed, sm::kStreamProposal), sw, sm::kDartAccept);
      const uint32_t accepted = log(u) < logA ? 1u : 0u;
      sh.accepted = accepted;
      if (log_row != nullptr) {
        log_row[0] = (double)p.i, log_row[1] = (double)p.j, log_row[2] = (double)p.kind, log_row[3] = n0, log_row[4] = n1;
        log_row[5] = logq, log_row[6] = logA, log_row[7] = (double)accepted;
      }
      if (c.counters != nullptr) {
        c.counters[2 * p.kind] += 1ull;
        c.counters[2 * p.kind + 1] += accepted;
      }
    }
    __syncthreads();
    // ---- apply ----
    if (sh.accepted) {                                  // (uniform)
      const bool split = p.kind == sm::kSplit;
      const uint32_t ga = (uint32_t)p.gi, gb = split ? (uint32_t)p.target : (uint32_t)p.gj;
      for (uint64_t r = t; r < nrows; r += nt)
        if (ell[r] == 1) z[r] = p.target;
      for (uint32_t f = t; f < (uint32_t)nfeat; f += nt) {
        smc_install(feats[f], pfeats[f], kpad, pk, ga, split ? 0 : 2);
        smc_install(feats[f], pfeats[f], kpad, pk, gb, split ? 1 : -1);
      }
      if (t == nt - 1) {
        const long long n0 = pcnt_acc[0], n1 = pcnt_acc[1];
        const long long cs[2] = {split ? n0 : n0 + n1, split ? n1 : 0ll};
        const uint32_t gs[2] = {ga, gb};
        for (int i = 0; i < 2; i++) {
          const long long cn = cs[i];
          const uint32_t g = gs[i];
          cnt_acc[g] = cn;
          cnt_u32[g] = (uint32_t)cn;
          smc_split(cn ? log((double)cn) : -(double)INFINITY, crp[g], crp[crp_lo_cnt(kpad) + g]);
          smc_split(cn > 1 ? log((double)cn - 1.0) : -(double)INFINITY, crp[kpad + g], crp[crp_lo_cntm1(kpad) + g]);
        }
        uint32_t ne = sh.nempty;                        // a split's label-1 block holds its anchor, a merged group none
        if (split && n1 > 0) ne--;
        if (!split) ne++;
        smc_split(ne > 0 ? log((double)alpha / (double)ne) : -(double)INFINITY, crp[2 * (size_t)kpad], crp[2 * (size_t)kpad + 2]);
        smc_split(log((double)alpha / ((double)ne + 1.0)), crp[2 * (size_t)kpad + 1], crp[2 * (size_t)kpad + 3]);
      }
      __syncthreads();                                  // (the groups' fields are written; every slice prepares from them)
      const uint32_t per = nfeat > 0 ? nt / (uint32_t)nfeat : 1u;
      const uint32_t S = per > 64u ? 64u : (per > 0u ? per : 1u);
      for (uint32_t i = t; i < (uint32_t)nfeat * S; i += nt) {
        prepare_group(feats[i / S], ga, kpad, i % S, S);
        prepare_group(feats[i / S], gb, kpad, i % S, S);
      }
    }
    if (trace != nullptr)
      for (uint64_t r = t; r < nrows; r += nt) trace[r] = z[r];
    __syncthreads();
  }
}

int launch_sm_chains(hipStream_t stream, const SmChain *chains_dev, uint32_t nchains, int nfeat, uint32_t K, uint32_t kpad,
                     uint32_t pair_kpad, uint64_t nrows, uint64_t row_id0, uint32_t p0, uint32_t p1, uint32_t launch_iters,
                     uint64_t sweep) {
  if (nfeat < 0 || nfeat > kSeqMaxFeat || K == 0 || nchains == 0 || pair_kpad < (uint32_t)kBlkTile) return -2;
  hipLaunchKernelGGL(k_sm_chains, dim3(nchains), dim3(kSmChainsThreads), 0, stream, chains_dev, nfeat, K, kpad, pair_kpad,
                     nrows, row_id0, p0, p1, launch_iters, sweep);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
