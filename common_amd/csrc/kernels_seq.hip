// kernels_seq.hip -- the sequential collapsed Gibbs sweep (msc_sweep_sequential, include/microscopes_hip.h; SURVEY 3.2, the
// reference's chain, entity_state.hpp:57-89): row i + 1 is scored against the tables row i has just changed.
//   k_sweep_seq   ONE workgroup carries the chain.  Per row visit, phases separated by __syncthreads:
//                   read   every thread reads the order entry, the row's old group and its count; threads f < nfeat
//                          stage feature f's value (and whether it is masked) in LDS
//                   leave  feature f's additive sums and fields (thread f, as k_entity_op's block f), the group count and
//                          its CRP terms (the last thread); then prepare_group of every (feature, table slice) for that group
//                   score  sum over the features of score_value (threads over groups, and over feature slices when K is
//                          below the block), into LDS; then log pseudocount + the slices in a fixed order
//                   draw   block max -> exp -> block scan of the per-thread sums (thread t owns a run of consecutive
//                          groups) -> every thread counts its CDF steps below the dart (util::sample_discrete_log: the
//                          draw is the number of steps below it)
//                   join   as leave, for the drawn group; the row's slot in z is written there
//                 Only the two groups that changed, and the empty-slot terms, have their CRP terms rewritten; the count of
//                 empty slots lives in LDS for the launch.  The score tables are read from global memory (L2 at these
//                 sizes).  A launch takes the visits that fit a time budget (route_calls.hpp seq_visit_us); the state carries over in
//                 global memory.
//   k_sweep_seq_chains   a grid of such workgroups, one independent chain each (msc_chains_sweep): what differs per chain
//                 is a SeqChain entry of a device table; also a thinned trace and the occupied-slot count per sample.
//                 Two nullable outputs per chain (msc_chains_visit): the visit's log predictive m + log(total) - log(n +
//                 alpha) of the draw's own block max and sum, by order position, and its running sum in double.
//   k_sweep_seq_chains_tempered   the same grid with chain c at its own temperature beta[c] (msc_chains_sweep_tempered):
//                 a slot's score is log pseudocount + beta * (the features' sum), each slice partial going on by one fused
//                 multiply-add in the place of the add (temper_math.hpp); beta == 0 reads no feature table.  A second
//                 instantiation of the workgroup's function: the two kernels above keep their code.
//   k_chains_clone   copies the additive tables and the z row of a source chain onto a destination, for a table of pairs
//                 (msc_chains_clone): words as they are, so a clone holds its ancestor's bits.
#include "commit_ops.hpp"
#include "device_error.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "score_block.hpp"
#include "seq_score.hpp"
#include "temper_math.hpp"

namespace msc {

MSC_DEV void seq_split(double v, float &hi, float &lo) {      // (kernels_score.hip crp_split: -inf has no lo part)
  hi = (float)v;
  lo = __builtin_isinf(hi) ? 0.f : (float)(v - (double)hi);
}

// feature f of one row joins (sign > 0) or leaves (sign < 0) group g: the additive sums and the reference's fields
// (k_entity_op's feature blocks); false when a leave finds the counter it would take a unit from empty
MSC_DEV bool seq_feature_op(const FeatDesc &fd, uint32_t v, uint32_t g, uint32_t kpad, int sign) {
  const long long sgn = sign;
  bool has = true;
  if (sign < 0) switch (fd.family) {
    case MSC_BB: has = fd.acc_i64[(v != 0 ? 0 : kpad) + g] > 0; break;
    case MSC_GP:
    case MSC_BNB:
    case MSC_NICH: has = fd.acc_i64[g] > 0; break;
    case MSC_DD: has = !((int)v >= 0 && (int)v < (int)fd.dim) || fd.acc_i64[(size_t)v * kpad + g] > 0; break;
    default: break;
  }
  if (!has) return false;
  switch (fd.family) {
    case MSC_BB: fd.acc_i64[(v != 0 ? 0 : kpad) + g] += sgn; break;
    case MSC_GP:
      fd.acc_i64[g] += sgn;
      fd.acc_i64[kpad + g] += sgn * (long long)v;
      fd.acc_f64[g] += (double)sign * log_factorial(v);
      break;
    case MSC_BNB:
      fd.acc_i64[g] += sgn;
      fd.acc_i64[kpad + g] += sgn * (long long)v;
      break;
    case MSC_DD:
      if ((int)v >= 0 && (int)v < (int)fd.dim) fd.acc_i64[(size_t)v * kpad + g] += sgn;
      break;
    case MSC_NICH: {
      const double x = __uint_as_float(v);
      fd.acc_i64[g] += sgn;
      fd.acc_f64[g] += (double)sign * x;
      fd.acc_f64[kpad + g] += (double)sign * x * x;
    } break;
    default: return true;
  }
  commit_group(fd, g, kpad);
  return true;
}

MSC_DEV float seq_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
MSC_DEV float seq_wave_scan(float v, int lane) {     // inclusive prefix sum over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(v, (unsigned)o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// shared state of the chain's workgroup
struct SeqShared {
  float sc[kSeqMaxGroups];        // score partials [slice][K], then every slot's score (slice 0's place)
  uint32_t val[kSeqMaxFeat];      // the visited row's value of every feature (raw 32 bits)
  uint8_t skip[kSeqMaxFeat];      // masked for that feature (no part in the sums or the score)
  float wmax[kSeqThreads / 64], wsum[kSeqThreads / 64];   // per-wave max / sum of the draw
  uint32_t nempty;                // empty slots among [0, K)
  uint32_t n;                     // rows seated: the sum of the group counts
  uint32_t below;                 // CDF steps below the dart
};

// leave (sign < 0) / join (sign > 0) of the staged row: every table of group g current afterwards
MSC_DEV void seq_move(SeqShared &sh, const FeatDesc *__restrict__ feats, int nfeat, uint32_t K, uint32_t kpad, uint32_t g,
                      int sign, long long *cnt_acc, uint32_t *cnt_u32, float alpha, float *crp, int32_t *zslot) {
  const uint32_t t = threadIdx.x, nt = kSeqThreads;
  for (uint32_t f = t; f < (uint32_t)nfeat; f += nt)
    if (!sh.skip[f] && !seq_feature_op(feats[f], sh.val[f], g, kpad, sign)) report_device_error(MSC_DEVERR_SEQ_SWEEP, g);
  if (t == nt - 1) {
    const long long c = cnt_acc[g] + sign;
    cnt_acc[g] = c;
    cnt_u32[g] = (uint32_t)c;
    seq_split(c ? log((double)c) : -(double)INFINITY, crp[g], crp[crp_lo_cnt(kpad) + g]);
    seq_split(c > 1 ? log((double)c - 1.0) : -(double)INFINITY, crp[kpad + g], crp[crp_lo_cntm1(kpad) + g]);
    uint32_t ne = sh.nempty;
    if (sign < 0 && c == 0) ne++;
    if (sign > 0 && c == 1) ne--;
    sh.nempty = ne;
    sh.n += (uint32_t)sign;
    seq_split(ne > 0 ? log((double)alpha / (double)ne) : -(double)INFINITY, crp[2 * (size_t)kpad], crp[2 * (size_t)kpad + 2]);
    seq_split(log((double)alpha / ((double)ne + 1.0)), crp[2 * (size_t)kpad + 1], crp[2 * (size_t)kpad + 3]);
    if (zslot != nullptr) *zslot = (int32_t)g;
  }
  __syncthreads();                                     // (the group's fields are written; every slice prepares from them)
  const uint32_t per = nfeat > 0 ? nt / (uint32_t)nfeat : 1u;   // slices of one (feature, group)'s table rows
  const uint32_t S = per > 64u ? 64u : (per > 0u ? per : 1u);
  for (uint32_t i = t; i < (uint32_t)nfeat * S; i += nt)
    if (!sh.skip[i / S]) prepare_group(feats[i / S], g, kpad, i % S, S);     // (a masked / noop feature's group is as it was)
  __syncthreads();
}

// MSC_SEQ_PHASES (an experiment build, Makefile VARIANT / EXTRA; tools/bench_sequential.py --phases): thread 0 stamps
// s_memtime after the barrier that closes each phase and adds the cycles per phase -- read, leave, score (sums, prior,
// max), draw (exp, scan, count), join -- and the visits into g_seq_phase; msc_seq_phase_cycles reads and clears it
#ifdef MSC_SEQ_PHASES
static __device__ unsigned long long g_seq_phase[6];
#define SEQ_STAMP(i)                                                   \
  do {                                                                 \
    if (t == 0) {                                                      \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
      ph_acc[i] += now_ - ph_last;                                     \
      ph_last = now_;                                                  \
    }                                                                  \
  } while (0)
#else
#define SEQ_STAMP(i) do {} while (0)
#endif

// The chain's workgroup, whichever kernel launched it: both kernels below are this function and nothing else, so a chain
// of k_sweep_seq_chains performs exactly the arithmetic of a k_sweep_seq launch with the same arguments.
// Visits [v0, v1) of the call's nsweeps x nrows: visit v is sweep v / nrows, position v % nrows of the order.
// Scoring: K >= the block, thread t sums every feature for groups t, t + 256, ...; fewer groups, the block is nq = 256 / K
// slices of K threads and slice q sums features q, q + nq, ... (partials summed in slice order: the same bits every run)
// trace (nullable): after sweep s of the call, when (s + 1) % trace_every == 0, z of the row range goes to sample
// (s + 1) / trace_every - 1; occupied (nullable): K - the empty slots at the same moments.
// logw, visit_logp (nullable): the visit at position pos has the log predictive of its row given the tables at that
// moment, inc = m + log(total) - log(n + alpha) in double (m, total: the draw's block max and sum; n: the rows seated, the
// row itself not among them; -inf when total == 0 or m == -inf).  visit_logp[pos] = (float)inc; *logw += inc, visit by
// visit in visit order by thread 0, in a register between the launch's first and last visit: the same adds however the
// visits are cut into launches.  Neither changes a draw: with both null the visit is as it was.
// kTempered (k_sweep_seq_chains_tempered; beta finite and >= 0, else unused): the slices' partials go on as
// temper::tempered_add(beta, partial, sk); at beta == 0 the score phase reads no feature table and adds no partial -- the
// slot's score is the CRP term's hi + lo -- while read, leave and join are as ever.  With kTempered false no line differs.
template <bool kTempered>
MSC_DEV void seq_visits(SeqShared &sh, const FeatDesc *__restrict__ feats, int nfeat, uint32_t K, uint32_t kpad,
                        uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z, const uint32_t *__restrict__ order,
                        uint64_t v0, uint64_t v1, uint64_t seed, uint64_t sweep, long long *cnt_acc, uint32_t *cnt_u32,
                        float alpha, float *crp, int32_t *trace, uint32_t trace_every, uint32_t *occupied, double *logw,
                        float *visit_logp, float beta) {
  const bool prior_only = kTempered && beta == 0.f;        // (-0.0f too)
  const uint32_t t = threadIdx.x, nt = kSeqThreads, lane = t & 63u, wave = t >> 6, nw = kSeqThreads / 64;
  if (t == 0) sh.nempty = sh.n = 0;
  __syncthreads();
  uint32_t mine = 0, mine_n = 0;
  for (uint32_t k = t; k < K; k += nt) {
    const uint32_t c = cnt_u32[k];
    mine += c == 0u;
    mine_n += c;
  }
  atomicAdd(&sh.nempty, mine);
  atomicAdd(&sh.n, mine_n);
  __syncthreads();
  const bool want_inc = logw != nullptr || visit_logp != nullptr;
  double lw = t == 0 && logw != nullptr ? *logw : 0.0;
  const float *lo0 = crp + crp_lo_cnt(kpad);
  const uint32_t nq = K < nt ? nt / K : 1u, q = t / K, kq = t - q * K;     // (scoring slices, K < the block)
  const uint32_t chunk = (K + nt - 1) / nt, kb = t * chunk;                  // the draw: thread t owns [kb, kb + chunk)
#ifdef MSC_SEQ_PHASES
  unsigned long long ph_acc[5] = {0, 0, 0, 0, 0}, ph_last = __builtin_amdgcn_s_memtime();
#endif
  for (uint64_t v = v0; v < v1; v++) {
    const uint64_t s = v / nrows, pos = v - s * nrows;
    // ---- read ----
    const uint32_t off = order != nullptr ? order[pos] : (uint32_t)pos;
    if (off >= nrows) {                                // (uniform: the whole block skips the visit)
      if (t == 0) report_device_error(MSC_DEVERR_SEQ_SWEEP, off);
    } else {
      const uint64_t row = row0 + off;
      const int32_t old = z[off];
      bool leave = old >= 0 && (uint32_t)old < K;
      if (leave && cnt_acc[old] <= 0) {               // a leave from an empty group: reported, the row only joins
        if (t == 0) report_device_error(MSC_DEVERR_SEQ_SWEEP, (uint32_t)old);
        leave = false;
      }
      for (uint32_t f = t; f < (uint32_t)nfeat; f += nt) {
        const FeatDesc &fd = feats[f];
        const bool skip = fd.family == MSC_NOOP || fd.col == nullptr || load_masked(fd, row, true);
        sh.skip[f] = skip;
        sh.val[f] = skip ? 0u : load_raw_value<false>(fd, 0, row, true);
      }
      __syncthreads();
      SEQ_STAMP(0);
      // leave (phase 0, when the row has a group), then score, draw and join (phase 1): one copy of seq_move's code
      uint32_t g = (uint32_t)old;
#pragma unroll 1
      for (int ph = leave ? 0 : 1; ph < 2; ph++) {
        if (ph == 1) {
          SEQ_STAMP(1);
          // ---- score: feature sums ----
          if (prior_only) {                              // (beta == 0: no feature table is read, sh.sc holds no partial)
          } else if (nq > 1) {
            if (q < nq) {
              float acc = 0.f;
              for (uint32_t f = q; f < (uint32_t)nfeat; f += nq) {
                if (sh.skip[f]) continue;
                const FeatDesc &fd = feats[f];
                const uint32_t x = sh.val[f];
                acc += seq_feature_score(fd, x, kq, kpad, fd.family == MSC_GP && x >= fd.vcap ? gp_row_const(x) : 0.0);
              }
              sh.sc[q * K + kq] = acc;
            }
          } else {
            for (uint32_t k = t; k < K; k += nt) {
              float acc = 0.f;
              for (int f = 0; f < nfeat; f++) {
                if (sh.skip[f]) continue;
                const FeatDesc &fd = feats[f];
                const uint32_t x = sh.val[f];
                acc += seq_feature_score(fd, x, k, kpad, fd.family == MSC_GP && x >= fd.vcap ? gp_row_const(x) : 0.0);
              }
              sh.sc[k] = acc;
            }
          }
          if (t == 0) sh.below = 0;
          __syncthreads();
          // ---- score: + log pseudocount (hi, the slices, lo), the block max ----
          const float e_hi = crp[2 * (size_t)kpad], e_lo = crp[2 * (size_t)kpad + 2];
          float m = -INFINITY;
          for (uint32_t k = kb; k < kb + chunk && k < K; k++) {
            const bool used = cnt_u32[k] != 0u;
            float sk = used ? crp[k] : e_hi;
            if (!kTempered) {
              for (uint32_t j = 0; j < nq; j++) sk += sh.sc[j * K + k];
            } else if (!prior_only) {
              for (uint32_t j = 0; j < nq; j++) sk = temper::tempered_add(beta, sh.sc[j * K + k], sk);
            }
            sk += used ? lo0[k] : e_lo;
            sh.sc[k] = sk;
            m = fmaxf(m, sk);
          }
          m = seq_wave_max(m);
          if (lane == 0) sh.wmax[wave] = m;
          __syncthreads();
          SEQ_STAMP(2);
          // ---- draw ----
          m = sh.wmax[0];
          for (uint32_t w = 1; w < nw; w++) m = fmaxf(m, sh.wmax[w]);
          float part = 0.f;
          for (uint32_t k = kb; k < kb + chunk && k < K; k++)
            part += __builtin_amdgcn_exp2f((sh.sc[k] - m) * 1.44269504088896340736f);   // exp(-inf) = 0
          const float incl = seq_wave_scan(part, (int)lane);
          float c = __shfl_up(incl, 1u, 64);             // the exclusive prefix of the scan itself: the CDF never steps back
          if (lane == 0) c = 0.f;
          if (lane == 63) sh.wsum[wave] = incl;
          __syncthreads();
          float total = 0.f;
          for (uint32_t w = 0; w < nw; w++) {
            const float ws = sh.wsum[w];
            if (w < wave) c += ws;
            total += ws;
          }
          if (want_inc && t == 0) {
            const double inc = total == 0.f || m == -INFINITY
                                   ? -(double)INFINITY
                                   : (double)m + log((double)total) - log((double)sh.n + (double)alpha);
            lw += inc;
            if (visit_logp != nullptr) visit_logp[pos] = (float)inc;
          }
          const float dart = philox_uniform01(seed, sweep + s, row_id0 + off) * total;
          uint32_t cnt = 0;
          for (uint32_t k = kb; k < kb + chunk && k < K; k++) {
            c += __builtin_amdgcn_exp2f((sh.sc[k] - m) * 1.44269504088896340736f);
            cnt += c < dart ? 1u : 0u;
          }
          if (cnt) atomicAdd(&sh.below, cnt);
          __syncthreads();
          SEQ_STAMP(3);
          g = sh.below < K ? sh.below : K - 1;
        }
        // ---- leave / join ----
        seq_move(sh, feats, nfeat, K, kpad, g, ph == 0 ? -1 : 1, cnt_acc, cnt_u32, alpha, crp, ph == 0 ? nullptr : z + off);
      }
      SEQ_STAMP(4);
    }
    if ((trace != nullptr || occupied != nullptr) && pos + 1 == nrows && (s + 1) % trace_every == 0) {
      const uint64_t j = (s + 1) / trace_every - 1;      // the row range's assignment after sweep s
      if (trace != nullptr)
        for (uint64_t i = t; i < nrows; i += nt) trace[j * nrows + i] = z[i];
      if (occupied != nullptr && t == 0) occupied[j] = K - sh.nempty;
      __syncthreads();
    }
  }
  if (t == 0 && logw != nullptr) *logw = lw;
#ifdef MSC_SEQ_PHASES
  if (t == 0) {
    for (int i = 0; i < 5; i++) atomicAdd(&g_seq_phase[i], ph_acc[i]);
    atomicAdd(&g_seq_phase[5], (unsigned long long)(v1 - v0));
  }
#endif
}

// visits [v0, v1) of the call's nsweeps x nrows: visit v is sweep v / nrows, position v % nrows of the order.
__global__ __launch_bounds__(kSeqThreads) void k_sweep_seq(const FeatDesc *__restrict__ feats, int nfeat, uint32_t K,
                                                           uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                                           int32_t *z, const uint32_t *__restrict__ order, uint64_t v0,
                                                           uint64_t v1, uint64_t seed, uint64_t sweep, long long *cnt_acc,
                                                           uint32_t *cnt_u32, float alpha, float *crp, int32_t *trace) {
  __shared__ SeqShared sh;
  seq_visits<false>(sh, feats, nfeat, K, kpad, row0, nrows, row_id0, z, order, v0, v1, seed, sweep, cnt_acc, cnt_u32, alpha,
                    crp, trace, 1u, nullptr, nullptr, nullptr, 1.f);
}

// the same visits of gridDim.x independent chains (msc_chains_sweep): workgroup c carries chain c, whose state, z, order,
// key and outputs come from chains[c]; the fields are read once, into what k_sweep_seq has as arguments
__global__ __launch_bounds__(kSeqThreads) void k_sweep_seq_chains(const SeqChain *__restrict__ chains, int nfeat, uint32_t K,
                                                                  uint32_t kpad, uint64_t row0, uint64_t nrows,
                                                                  uint64_t row_id0, uint64_t v0, uint64_t v1, uint64_t sweep,
                                                                  uint32_t trace_every) {
  __shared__ SeqShared sh;
  const SeqChain &c = chains[blockIdx.x];
  const FeatDesc *feats = c.feats;
  int32_t *z = c.z, *trace = c.trace;
  long long *cnt_acc = c.cnt_acc;
  uint32_t *cnt_u32 = c.cnt_u32, *occupied = c.occupied;
  float *crp = c.crp;
  const uint32_t *order = c.order;
  const float alpha = c.alpha;
  const uint64_t seed = c.seed;
  double *logw = c.logw;
  float *visit_logp = c.visit_logp;
  seq_visits<false>(sh, feats, nfeat, K, kpad, row0, nrows, row_id0, z, order, v0, v1, seed, sweep, cnt_acc, cnt_u32, alpha,
                    crp, trace, trace_every, occupied, logw, visit_logp, 1.f);
}

// k_sweep_seq_chains with chain c at the temperature beta[c], read here once per launch (msc_chains_sweep_tempered; the
// entries' logw and visit_logp are not read: a tempered visit has no weight).  A beta that is none -- NaN, negative,
// infinite -- is reported with the chain as its detail and the chain's workgroup makes no visit: it writes no sample and
// changes neither z nor a table; the other chains run as usual.
__global__ __launch_bounds__(kSeqThreads) void k_sweep_seq_chains_tempered(const SeqChain *__restrict__ chains,
                                                                           const float *__restrict__ beta_dev, int nfeat,
                                                                           uint32_t K, uint32_t kpad, uint64_t row0,
                                                                           uint64_t nrows, uint64_t row_id0, uint64_t v0,
                                                                           uint64_t v1, uint64_t sweep, uint32_t trace_every) {
  __shared__ SeqShared sh;
  const float beta = beta_dev[blockIdx.x];
  if (!temper::beta_ok(beta)) {                          // (uniform: the whole block leaves)
    if (threadIdx.x == 0) report_device_error(MSC_DEVERR_TEMPER_BETA, blockIdx.x);
    return;
  }
  const SeqChain &c = chains[blockIdx.x];
  const FeatDesc *feats = c.feats;
  int32_t *z = c.z, *trace = c.trace;
  long long *cnt_acc = c.cnt_acc;
  uint32_t *cnt_u32 = c.cnt_u32, *occupied = c.occupied;
  float *crp = c.crp;
  const uint32_t *order = c.order;
  const float alpha = c.alpha;
  const uint64_t seed = c.seed;
  seq_visits<true>(sh, feats, nfeat, K, kpad, row0, nrows, row_id0, z, order, v0, v1, seed, sweep, cnt_acc, cnt_u32, alpha,
                   crp, trace, trace_every, occupied, nullptr, nullptr, beta);
}

int launch_sweep_seq(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t K, uint32_t kpad, uint64_t row0,
                     uint64_t nrows, uint64_t row_id0, int32_t *z, const uint32_t *order, uint64_t v0, uint64_t v1,
                     uint64_t seed, uint64_t sweep, long long *cnt_acc, uint32_t *cnt_u32, float alpha, float *crp,
                     int32_t *trace) {
  if (nfeat < 0 || nfeat > kSeqMaxFeat || K == 0 || K > kSeqMaxGroups) return -2;
  hipLaunchKernelGGL(k_sweep_seq, dim3(1), dim3(kSeqThreads), 0, stream, feats_dev, nfeat, K, kpad, row0, nrows, row_id0,
                     z, order, v0, v1, seed, sweep, cnt_acc, cnt_u32, alpha, crp, trace);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sweep_seq_chains(hipStream_t stream, const SeqChain *chains_dev, uint32_t nchains, int nfeat, uint32_t K,
                            uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t v0, uint64_t v1,
                            uint64_t sweep, uint32_t trace_every) {
  if (nfeat < 0 || nfeat > kSeqMaxFeat || K == 0 || K > kSeqMaxGroups || nchains == 0 || trace_every == 0) return -2;
  hipLaunchKernelGGL(k_sweep_seq_chains, dim3(nchains), dim3(kSeqThreads), 0, stream, chains_dev, nfeat, K, kpad, row0,
                     nrows, row_id0, v0, v1, sweep, trace_every);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sweep_seq_chains_tempered(hipStream_t stream, const SeqChain *chains_dev, const float *beta_dev, uint32_t nchains,
                                     int nfeat, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                     uint64_t v0, uint64_t v1, uint64_t sweep, uint32_t trace_every) {
  if (nfeat < 0 || nfeat > kSeqMaxFeat || K == 0 || K > kSeqMaxGroups || nchains == 0 || trace_every == 0 ||
      beta_dev == nullptr)
    return -2;
  hipLaunchKernelGGL(k_sweep_seq_chains_tempered, dim3(nchains), dim3(kSeqThreads), 0, stream, chains_dev, beta_dev, nfeat, K,
                     kpad, row0, nrows, row_id0, v0, v1, sweep, trace_every);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// nwords 32-bit words from src to dst by the blocks of grid row y: 16 bytes a lane where both ends are aligned to it
MSC_DEV void clone_words(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, size_t nwords) {
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
    const size_t nvec = nwords / 4;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (size_t i = i0; i < nvec; i += step) d4[i] = s4[i];
    for (size_t i = nvec * 4 + i0; i < nwords; i += step) dst[i] = src[i];
  } else {
    for (size_t i = i0; i < nwords; i += step) dst[i] = src[i];
  }
}

// pair blockIdx.y of the table: the source's additive tables (int64 sums, the group counts leading; float64 sums) and z
// row onto the destination's.  A pair's source is no pair's destination (msc_chains_clone checks), so no block reads
// what another writes.
__global__ __launch_bounds__(256) void k_chains_clone(const ClonePair *__restrict__ pairs, size_t n_i64, size_t n_f64,
                                                      size_t nrows) {
  const ClonePair p = pairs[blockIdx.y];
  clone_words(reinterpret_cast<const uint32_t *>(p.src_i64), reinterpret_cast<uint32_t *>(p.dst_i64), 2 * n_i64);
  clone_words(reinterpret_cast<const uint32_t *>(p.src_f64), reinterpret_cast<uint32_t *>(p.dst_f64), 2 * n_f64);
  clone_words(reinterpret_cast<const uint32_t *>(p.src_z), reinterpret_cast<uint32_t *>(p.dst_z), nrows);
}

int launch_chains_clone(hipStream_t stream, const ClonePair *pairs_dev, uint32_t npairs, size_t n_i64, size_t n_f64,
                        size_t nrows) {
  const size_t words = std::max(std::max(2 * n_i64, 2 * n_f64), nrows);
  const uint32_t chunks = (uint32_t)std::min<size_t>(64, std::max<size_t>(1, (words / 4 + 255) / 256));
  for (uint32_t p0 = 0; p0 < npairs; p0 += 65535u)      // (a grid's y extent; one launch up to 65535 pairs)
    hipLaunchKernelGGL(k_chains_clone, dim3(chunks, std::min(npairs - p0, 65535u)), dim3(256), 0, stream, pairs_dev + p0,
                       n_i64, n_f64, nrows);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

MSC_DEFINE_BIND_ERROR_WORD(bind_error_word_seq)

#ifdef MSC_SEQ_PHASES
// cycles per phase (read, leave, score, draw, join) and visits since the last call; synchronises the device
extern "C" int msc_seq_phase_cycles(unsigned long long *out6) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_seq_phase), 6 * sizeof(unsigned long long)) != hipSuccess) return -1;
  const unsigned long long zero[6] = {0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_seq_phase), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace msc
