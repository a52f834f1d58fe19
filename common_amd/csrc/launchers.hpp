// launchers.hpp -- host entry points of the kernel translation units.  They launch what the routes chose (route.hpp,
// route_calls.hpp: the only places that choose); nothing is chosen here.
#pragma once
#include <algorithm>

#include "msc_internal.hpp"
#include "route_calls.hpp"

namespace msc {

// A function attribute (dynamic LDS beyond 64 KiB) is per device: `seen` is the launcher's own bit set of devices that
// have it.  True the first time the current device asks.
inline bool first_use_on_device(unsigned long long &seen) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;
  const unsigned long long bit = 1ull << dev;
  if (seen & bit) return false;
  seen |= bit;
  return true;
}

struct UnpackFeat {
  void *dst;
  uint8_t *dst_mask;     // may be null
  uint32_t offset;       // byte offset of the feature in the packed record
  uint32_t mask_offset;  // element offset of the feature in the mask record
  int32_t src_type, dst_type;
  uint32_t count;
  uint32_t pad;
};

// kernels_single.hip
struct MailboxHeader {
  int32_t family, dim, op, status;
  float score;
  uint32_t hp_off, ss_off, value_off;
};
int launch_value_op(hipStream_t stream, void *mailbox_dev, uint32_t dim, int family);

// every kernel translation unit that can report a device-side error (device_error.hpp): point its copy of the pointer at
// the device's pinned word; called once per device by msc_context_create
int bind_error_word_score(uint32_t *word_dev);
int bind_error_word_sweep(uint32_t *word_dev);
int bind_error_word_state(uint32_t *word_dev);
int bind_error_word_seq(uint32_t *word_dev);
int bind_error_word_query(uint32_t *word_dev);

// kernels_score.hip
int launch_prepare(hipStream_t stream, const FeatDesc *feats_dev, uint32_t nfeat, uint32_t kpad, uint32_t value_slices);
int launch_dm_prepare(hipStream_t stream, const FeatDesc *feats_dev, int f, uint32_t dim, uint32_t kpad, uint32_t value_slices);
int launch_crp_prepare(hipStream_t stream, const uint32_t *cnt, uint32_t K, uint32_t kpad, float alpha,
                       float *crp);
int launch_entity_op(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t K, uint32_t kpad, uint64_t row,
                     uint32_t group, int sign, long long *cnt_acc, uint32_t *cnt_u32, float alpha, float *crp, int32_t *z_slot);
int launch_set_i32(hipStream_t stream, int32_t *dst, int32_t value);
constexpr int kLooRows = 4, kLooThreads = 1024;      // k_loo_own_lds: rows a thread, threads a workgroup (staged = true)
int launch_loo_own(hipStream_t stream, bool heavy, bool staged, const FeatDesc *feats_dev, int nfeat, uint32_t K, uint32_t kpad, uint64_t row0,
                   uint64_t nrows, const int32_t *z, const float *crp, float *own);
int launch_gp_large_fix(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, int f, uint32_t K,
                        uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z, float *out, uint64_t ld);
// k_score_nich1 launch shapes: a wave visits `visits` blocks of q consecutive rows (index 0 = the default)
struct Nich1Shape { int q, visits; };
constexpr int kNich1NumShapes = 8;
extern const Nich1Shape kNich1Shapes[kNich1NumShapes];
// what k_score_tail_rows needs to score a partly filled last tile (<= kTailMaxGroups groups; tile_plan.hpp plan_layout: the plan's first
// phase is lookup features only, the second plain nich features).  ok = false: the plan is not for it.
struct TailPlan {
  bool ok = false;            // (route.hpp narrow_tail_fits: the plan, the tile and the LDS the staged tables need)
  bool exact = true;          // the tile kernels' bits (two sums per group: score passes, where the row count picks the kernel);
                              // false: one sum per group, faster (sweeps: the choice of kernel follows the bound view's row count, not the call's)
  bool masked_nich = false;   // the first phase holds masked nich columns (the kernel's instantiation that evaluates them)
  bool dm = false;            // ... or dm features with their tables staged whole (the instantiation that looks them up)
  uint32_t max_rows = 0;      // the largest lookup table (rows a value may select)
  uint32_t pack_rows = 0;     // all lookup tables together
  float *pack = nullptr;      // scratch of pack_rows x 64 floats (the tail groups' tables, k_tail_pack), owned by the state
};
// the narrow kernel alone: groups [k0, K) of every row (k0 < K <= k0 + kTailMaxGroups, tp.ok)
int launch_score_tail(hipStream_t stream, int num_cus, const TailPlan &tp, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K,
                      uint32_t kpad, uint32_t k0, uint64_t row0, uint64_t nrows, const int32_t *z, const float *own, const float *crp,
                      float *out, uint64_t ld);
// two runs of 8-byte words that a fused sweep kernel zeroes on its way (the additive tables, which the accumulate
// pass that follows in a sweep step wants empty); all null / 0 when nothing follows
struct ZeroSpans {
  unsigned long long *a = nullptr;
  size_t na = 0;
  unsigned long long *b = nullptr;
  size_t nb = 0;
};
// (kernels_score.hip: the lane <-> row kernel with the draw in it; K <= 64, tp.ok)
int launch_sweep_rows(hipStream_t stream, int num_cus, const TailPlan &tp, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K,
                      uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z, const float *own, const float *crp,
                      const uint64_t *rng, ZeroSpans zero);
int launch_score_pair_tail(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K, uint32_t kpad,
                           uint64_t row0, uint64_t nrows, const int32_t *z, const float *own, const float *crp, float *tail, uint64_t ld);
int launch_score(hipStream_t stream, int num_cus, ScorePath path, const TailPlan &narrow_tail, const ScoreShape &shape, const FeatDesc *feats_dev, int nfeat, int nsplit,
                 uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z,
                 const float *own, const float *crp, float *out, uint64_t ld);

// which kernel INSTANTIATION the library chose for the most recent scoring pass (slot 0) / fused assignment pass (slot 1)
// / z-matrix kernel (slot 2) / row predictive pass (slot 3: the kernel that reduced the rows),
// spelled as rocprofv3 spells it ("k_score_tile_roles<false, false, false>"): bench.py and tools/ key the committed
// counter summaries by it (msc_last_kernel, include/microscopes_hip.h).  Process-wide, set by the launchers.
void note_kernel(int slot, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *last_kernel(int slot);
inline const char *tf(bool b) { return b ? "true" : "false"; }
// what the routed launchers return: 0, or MSC_EHIP with the launch's HIP error (or the shape no route sends) reported
inline int launch_status(const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(MSC_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

// kernels_sweep.hip (launchers launch what route.hpp route_sweep chose: a shape it never sends is MSC_EHIP, reported)
int launch_sweep_nich1(hipStream_t stream, int num_cus, bool transposed, const FeatDesc *feats_dev, uint32_t K,
                       uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z,
                       const float *own, const float *crp, const uint64_t *rng_dev, ZeroSpans zero);
#ifndef MSC_NICH_PACK_WAVES
#define MSC_NICH_PACK_WAVES 8
#endif
constexpr int kNichPackWaves = MSC_NICH_PACK_WAVES;   // waves a workgroup of the nich-only kernels (8: two a SIMD and 256 registers each -- no LDS ties them to sixteen)
#ifndef MSC_NICH_PACK_NC
#define MSC_NICH_PACK_NC 4
#endif
constexpr int kNichPackNC = MSC_NICH_PACK_NC;          // groups of the lane a block part of the nich-only kernels takes (256 registers a wave there)
int launch_sweep_mixed(hipStream_t stream, int num_cus, bool has_dm, ScorePath path, const ScoreShape &shape, const FeatDesc *feats_dev, int nfeat, int nsplit,
                       uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z,
                       const float *own, const float *crp, const uint64_t *rng, ZeroSpans zero);
int launch_sweep_roles_tail(hipStream_t stream, int num_cus, ScorePath path, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K,
                            uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z, const float *own,
                            const float *crp, const uint64_t *rng, ZeroSpans zero, const float *tail);
int sweep_niw1_max_groups(uint32_t dim);
// single nich feature beyond 1024 groups (lane <-> row, groups as scalar operands); `table`: device scratch of
// sweep_nich1_rows_table_floats(kpad) floats, rewritten by every call
size_t sweep_nich1_rows_table_floats(uint32_t kpad);
uint32_t sweep_nich1_rows_max_groups();
int launch_sweep_nich1_rows(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, uint32_t K, uint32_t kpad,
                            uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z, const float *crp,
                            const uint64_t *rng, ZeroSpans zero, float *table);
int launch_sweep_niw1(hipStream_t stream, int num_cus, uint32_t dim, const FeatDesc *feats_dev, uint32_t K, uint32_t kpad,
                      uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z, const float *crp, const uint64_t *rng,
                      ZeroSpans zero);
int launch_narrow(hipStream_t stream, int num_cus, int lanes_per_row, uint32_t table_rows, bool sweep, const FeatDesc *feats_dev,
                  int nfeat, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z, const float *own,
                  const float *crp, float *out, uint64_t ld, uint64_t row_id0, int32_t *z_out, const uint64_t *rng,
                  ZeroSpans zero);
int launch_sample_rows(hipStream_t stream, int num_cus, const float *scores, uint64_t ld, uint32_t K,
                       uint64_t nrows, uint64_t row_id0, int32_t *z, const uint64_t *rng_dev);
int launch_rng_set(hipStream_t stream, uint64_t *rng_dev, uint64_t seed, uint64_t sweep);
int launch_rng_bump(hipStream_t stream, uint64_t *rng_dev);

// kernels_seq.hip: visits [v0, v1) of the sequential sweep (msc_sweep_sequential), one workgroup; -2: shape not covered
// (kSeqMaxGroups, kSeqMaxFeat: route_calls.hpp route_sequential)
constexpr int kSeqThreads = 256;           // the workgroup: one wave a SIMD, room for prepare_group and the score paths
int launch_sweep_seq(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t K, uint32_t kpad, uint64_t row0,
                     uint64_t nrows, uint64_t row_id0, int32_t *z, const uint32_t *order, uint64_t v0, uint64_t v1,
                     uint64_t seed, uint64_t sweep, long long *cnt_acc, uint32_t *cnt_u32, float alpha, float *crp,
                     int32_t *trace);
// ... and of nchains independent chains, one workgroup each (msc_chains_sweep): what differs per chain
struct SeqChain {
  const FeatDesc *feats;   // the chain's state: descriptors, counts (additive, u32), CRP terms
  long long *cnt_acc;
  uint32_t *cnt_u32;
  float *crp;
  int32_t *z;              // int32 [nrows] of the row range
  const uint32_t *order;   // uint32 [nrows] or null (ascending)
  int32_t *trace;          // int32 [ntrace][nrows] or null
  uint32_t *occupied;      // uint32 [ntrace] or null
  double *logw;            // one double or null: the visits' log predictives are added to it (msc_chains_visit)
  float *visit_logp;       // float [nrows] by order position or null: each visit's log predictive
  uint64_t seed;           // the chain's Philox key
  float alpha;
  uint32_t pad;
};
// trace_every >= 1: sample (s + 1) / trace_every - 1 is written after sweep s of the call when (s + 1) % trace_every == 0
int launch_sweep_seq_chains(hipStream_t stream, const SeqChain *chains_dev, uint32_t nchains, int nfeat, uint32_t K,
                            uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t v0, uint64_t v1,
                            uint64_t sweep, uint32_t trace_every);
// ... with chain c at the temperature beta_dev[c] (msc_chains_sweep_tempered): float [nchains] on the device, read by the
// kernel once per launch; the entries' logw and visit_logp are not read
int launch_sweep_seq_chains_tempered(hipStream_t stream, const SeqChain *chains_dev, const float *beta_dev, uint32_t nchains,
                                     int nfeat, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                     uint64_t v0, uint64_t v1, uint64_t sweep, uint32_t trace_every);
// msc_chains_clone: pair p's source tables (red_i64[n_i64], red_f64[n_f64]) and z row [nrows] onto its destination's, one
// launch for all pairs (grid: chunks x pairs); no source may be a destination
struct ClonePair {
  const long long *src_i64;
  long long *dst_i64;
  const double *src_f64;
  double *dst_f64;
  const int32_t *src_z;
  int32_t *dst_z;
};
int launch_chains_clone(hipStream_t stream, const ClonePair *pairs_dev, uint32_t npairs, size_t n_i64, size_t n_f64,
                        size_t nrows);

// kernels_blocked.hip: the blocked Gibbs sampler (msc_blocked_*; route_calls.hpp route_blocked chooses the assign kernel)
int launch_blocked_draw(hipStream_t stream, const BlkFeat *fs_dev, uint32_t nfeat, uint32_t K, uint32_t kpad,
                        const uint32_t *cnt, float alpha, uint64_t seed, uint64_t sweep, double *work, float *tab);
int launch_blocked_assign(hipStream_t stream, BlockedKernel kernel, uint32_t block, const BlkFeat *fs_dev, int nfeat,
                          const float *tab, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                          int32_t *z, uint64_t seed, uint64_t sweep);
int launch_blocked_top_slot(hipStream_t stream, const uint32_t *cnt, uint32_t K, uint32_t *out);

// kernels_blocked_niw.hip: the same sampler for a state of one niw feature of dim <= 32 (BlockedKernel::niw1).  The draw:
// the stick weights, then every slot's mean[K][dim], whiten[K][dim (dim + 1) / 2] and, from the same doubles, the operand
// streams w64 / mu64 of the assign kernel (msc_internal.hpp niw_w_index / niw_b_index)
int launch_blocked_draw_niw(hipStream_t stream, const BlkFeat *fs_dev, uint32_t K, uint32_t kpad, const uint32_t *cnt,
                            float alpha, uint64_t seed, uint64_t sweep, double *work, float *tab, double *mean,
                            double *whiten, double *w64, double *mu64);
int launch_blocked_assign_niw(hipStream_t stream, uint32_t dim, const BlkFeat *fs_dev, const float *tab, const double *w64,
                              const double *mu64, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                              int32_t *z, uint64_t seed, uint64_t sweep);

// kernels_splitmerge.hip: the split-merge move (msc_split_merge; route_calls.hpp route_splitmerge chooses the assign kernel).
// seed is the caller's: the launchers form the streams' keys (splitmerge_math.hpp).  `zero`: the pair state's additive
// tables, emptied on the way for the accumulate pass that follows.
int launch_sm_begin(hipStream_t stream, const int32_t *z, uint64_t nrows, uint64_t row_id0, const uint32_t *cnt, uint32_t K,
                    uint64_t seed, uint64_t sweep, SmProp *prop, int32_t *ell, ZeroSpans zero);
uint32_t sm_assign_blocks(uint64_t nrows, uint32_t block);   // workgroups (= partials) of an assign pass
int launch_sm_assign(hipStream_t stream, BlockedKernel kernel, uint32_t block, bool final, uint32_t pass, const BlkFeat *fs_dev,
                     int nfeat, const float *tab, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                     const int32_t *z, int32_t *ell, const SmProp *prop, uint64_t seed, uint64_t sweep, double *part,
                     ZeroSpans zero);
int launch_sm_merge_slots(hipStream_t stream, long long *i64, uint32_t rows_i, double *f64, uint32_t rows_f, uint32_t kpad);
int launch_sm_decide(hipStream_t stream, SmProp *prop, const double *part, uint32_t nparts, const float *sd, uint32_t nfeat,
                     const uint32_t *pair_cnt, float alpha, uint64_t seed, uint64_t sweep, double *log_row,
                     unsigned long long *counters);
int launch_sm_relabel(hipStream_t stream, uint64_t nrows, int32_t *z, const int32_t *ell, const SmProp *prop,
                      const uint32_t *pair_cnt, uint32_t *cnt);

// kernels_chains_sm.hip: the same move for every chain of an ensemble in one launch (msc_chains_split_merge), workgroup c
// on chain c: proposals [p0, p1) of the call, whole proposals only.  What differs per chain:
constexpr int kSmChainsThreads = 256;      // the workgroup: one wave a SIMD, as the sequential chain's
struct SmChain {
  const FeatDesc *feats;       // the chain's state: descriptors, counts (additive, u32), CRP terms
  long long *cnt_acc;
  uint32_t *cnt_u32;
  float *crp;
  int32_t *z;                  // int32 [nrows]
  const FeatDesc *pair_feats;  // the chain's pair state (blocked.cpp sm_setup): descriptors, parameter-table features,
  const BlkFeat *pair_blk;     // the parameter table theta (msc_split_merge_tables' layout), the pair's counts
  float *pair_tab;
  long long *pair_cnt_acc;
  uint32_t *pair_cnt_u32;
  int32_t *ell;                // int32 [nrows]: the pair labels (the handle's scratch)
  double *log;                 // double [nproposals][8] or null
  int32_t *trace;              // int32 [nproposals][nrows] or null
  int32_t *proposed;           // int32 [nproposals][nrows] or null
  unsigned long long *counters;   // [5] or null
  uint64_t seed;               // the chain's seed (the streams' keys: splitmerge_math.hpp)
  float alpha;
  uint32_t pad;
};
// -2: shape not covered (more than kSeqMaxFeat features)
int launch_sm_chains(hipStream_t stream, const SmChain *chains_dev, uint32_t nchains, int nfeat, uint32_t K, uint32_t kpad,
                     uint32_t pair_kpad, uint64_t nrows, uint64_t row_id0, uint32_t p0, uint32_t p1, uint32_t launch_iters,
                     uint64_t sweep);

// kernels_niw.hip
int launch_niw_prepare(hipStream_t stream, const FeatDesc *feats_dev, uint32_t f, uint32_t dim, uint32_t K,
                       uint32_t kpad);
int launch_niw_score_data(hipStream_t stream, const FeatDesc *feats_dev, uint32_t f, uint32_t K,
                          uint32_t kpad, float *out);
int launch_niw_score(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, uint32_t f, uint32_t dim, uint32_t K,
                     uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z, bool accum, bool f32_fast,
                     double *qown /* [nrows] scratch, leave-one-out only */, float *out, uint64_t ld);
int launch_niw_accumulate(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, uint32_t f, uint32_t K,
                          uint64_t row0, uint64_t nrows, const int32_t *z, int sign, uint32_t *scratch_dev, uint32_t dim);
int launch_niw_commit(hipStream_t stream, const FeatDesc *feats_dev, uint32_t f, uint32_t dim, uint32_t K,
                      uint32_t kpad, int to_raw);

// kernels_state.hip
int launch_accumulate(hipStream_t stream, int num_cus, const FeatDesc *feats_dev,
                      const FeatDesc *feats_host, int nfeat, uint32_t K, uint32_t kpad, uint64_t row0,
                      uint64_t nrows, const int32_t *z, int sign, long long *cnt_acc);
int launch_commit(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t kpad,
                  const long long *cnt_acc, uint32_t *cnt_u32);
int launch_commit_prepare(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t K, uint32_t kpad,
                          const long long *cnt_acc, uint32_t *cnt_u32, float alpha, float *crp, uint64_t *rng_bump,
                          uint32_t value_slices);
int launch_pack64(hipStream_t stream, bool unpack, long long *i64, size_t ni, double *f64, size_t nf, double *pack);
int launch_zero64(hipStream_t stream, void *a, size_t na, void *b, size_t nb);   // 8-byte words
int launch_stream_fill(hipStream_t stream, int num_cus, void *buf, size_t nbytes);   // the score kernels' store pattern, zeros
int launch_lift(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t kpad,
                long long *cnt_acc, const uint32_t *cnt_u32, int lift_cnt);
int launch_score_data(hipStream_t stream, const FeatDesc *feats_dev, int nfeat, uint32_t K,
                      uint32_t kpad, float *out);
int launch_relation_blocks(hipStream_t stream, uint32_t ndim, const uint64_t *shape, const int32_t *const *z_dev,
                           const uint32_t *ngroups, const uint32_t *positions_dev, uint64_t ncells, int32_t *out_dev);
int launch_relation_slice_scores(hipStream_t stream, const float *scores, uint64_t ld, uint32_t ndim, const uint64_t *shape,
                                 uint32_t dim, const uint32_t *seg_dev, const uint32_t *ids_dev, const int32_t *off_dev,
                                 uint32_t ncand, uint32_t cand_stride, uint64_t nent, float *out_dev, uint64_t ld_out);
int launch_dm_stats(hipStream_t stream, const uint32_t *col, uint64_t n, uint32_t dim, uint32_t *colmax_dev,
                    uint32_t *rowtot_dev);
int launch_col_max_u32(hipStream_t stream, const uint32_t *col, uint64_t n, uint32_t *out_dev);
int launch_mask_sentinel(hipStream_t stream, const void *col, const uint8_t *mask, uint64_t n, bool bytes, uint32_t sentinel, void *out);
int launch_pack_bits(hipStream_t stream, const void *const *cols, int m, uint32_t radix, uint64_t n, void *out);
int launch_pack_nich_x(hipStream_t stream, const float *const *cols_dev, uint32_t n2, uint32_t n2p, uint64_t n, float *out);
int launch_pack_look_idx(hipStream_t stream, const LookIdxSrc *src_dev, uint32_t nsrc, uint32_t l4, uint64_t n, uint32_t *out);
int launch_fuse_tables(hipStream_t stream, const FeatDesc *feats_dev, int nsplit, int nblocks, uint32_t kpad);
// kernels_hp.hip (msc_hp_grid_*): score + reduce of njobs feature grids (partials [nblk][npoints] per job, then out), the CRP
// grid, and the draw of njobs grids (every job of the draw is scored into `scores` at its out_off)
int launch_hp_grid_score(hipStream_t stream, const HpJob *jobs_dev, uint32_t njobs, uint32_t max_points, uint32_t K,
                         uint32_t kpad, const uint32_t *cnt, const uint8_t *slots, uint32_t nblk, double *part,
                         double *out);
int launch_crp_grid_score(hipStream_t stream, const HpJob *job_dev, uint32_t npoints, const uint32_t *cnt, uint32_t K,
                          double *out);
int launch_hp_grid_draw(hipStream_t stream, const HpJob *jobs_dev, uint32_t njobs, const double *scores, uint64_t seed,
                        uint64_t sweep, uint32_t *chosen);
// kernels_slice.hip (msc_hp_slice / msc_theta_slice): one workgroup per target; the theta kernel writes per (job, block of
// 256 slots) the evaluations and the first slot left unchanged for a non-finite target (theta_slice_blocks(K) blocks a job)
int launch_hp_slice(hipStream_t stream, const SliceTarget *targets_dev, uint32_t ntargets, const SliceCoord *coords_dev,
                    uint32_t K, uint32_t kpad, const uint32_t *cnt, const uint8_t *slots, uint64_t key, uint64_t sweep,
                    float *values, uint32_t *evals, uint32_t *status);
// the ensemble's step (msc_chains_hp_slice): targets_dev [nchains][ntargets], chains_dev [nchains], coords_dev [n] shared,
// values / evals / status [nchains][n]; then the rebuild of every chain's score tables (prepare_group, value_slices
// threads per (feature, group) as launch_prepare) and CRP table from chains_dev[c].alpha as the step left it
constexpr uint32_t kMaxGridYZ = 65535;
int launch_hp_slice_chains(hipStream_t stream, const SliceTarget *targets_dev, uint32_t ntargets, HpChain *chains_dev,
                           uint32_t nchains, const SliceCoord *coords_dev, uint32_t n, uint32_t K, uint32_t kpad,
                           uint64_t sweep, float *values, uint32_t *evals, uint32_t *status);
int launch_chains_prepare(hipStream_t stream, const HpChain *chains_dev, uint32_t nchains, uint32_t nfeat, uint32_t K,
                          uint32_t kpad, uint32_t value_slices);
inline uint32_t theta_slice_blocks(uint32_t K) { return (K + 255) / 256; }
int launch_theta_slice(hipStream_t stream, const ThetaJob *jobs_dev, uint32_t njobs, uint32_t K, uint32_t kpad,
                       const uint32_t *cnt, const uint8_t *slots, uint64_t key, uint64_t sweep,
                       unsigned long long *evals_part, uint32_t *bad_part);
int launch_unpack(hipStream_t stream, const uint8_t *records, const uint8_t *mask, uint64_t nrows,
                  uint32_t rowsize, uint32_t maskrowsize, const void *feats_dev, uint32_t nfeat);
// kernels_joint.hip (msc_score_joint / msc_chains_score_joint / msc_chains_keep_best): one workgroup per state or chain
// writes the row of nfeatures + 3 doubles; coords: the n hyper-prior entries on the HOST (they travel as kernel
// arguments, kJointCoords a launch); keep_best: one workgroup per chain
int launch_score_joint(hipStream_t stream, const FeatDesc *feats_dev, uint32_t nfeat, uint32_t K, uint32_t kpad,
                       const uint32_t *cnt, const uint8_t *slots, float alpha, const JointCoord *coords, uint32_t n,
                       double *out);
int launch_chains_score_joint(hipStream_t stream, const JointChain *chains_dev, uint32_t nchains, uint32_t nfeat, uint32_t K,
                              uint32_t kpad, const JointCoord *coords, uint32_t n);
int launch_chains_keep_best(hipStream_t stream, uint32_t nchains, const double *joint, uint64_t ld_joint, const int32_t *z,
                            uint64_t ld_z, uint64_t nrows, int64_t iter, double *best, int32_t *best_z, uint64_t ld_best,
                            int64_t *best_iter);
// kernels_temper.hip (msc_chains_exchange / msc_chains_anneal_weights; the arithmetic: temper_math.hpp): joint is the
// chains' rows as msc_chains_score_joint wrote them.  exchange: one thread a ladder of nrungs chains; anneal_weights: one
// thread a chain; err_word_dev: the device address of the context's error word pair (a broken ladder is reported there)
int launch_chains_exchange(hipStream_t stream, uint32_t nchains, uint32_t nfeat, const double *joint, uint64_t ld_joint,
                           uint32_t nrungs, float *beta, int32_t *rung, uint64_t parity, uint64_t seed, uint64_t sweep,
                           uint32_t *proposed, uint32_t *accepted, uint32_t *err_word_dev);
int launch_chains_anneal_weights(hipStream_t stream, uint32_t nchains, uint32_t nfeat, const double *joint, uint64_t ld_joint,
                                 const float *beta_from, const float *beta_to, double *logw);

// kernels_pred.hip
int launch_pred_prepare(hipStream_t stream, const PredFeat *pfs_dev, const std::vector<PredFeat> &pfs, uint32_t K,
                        uint32_t kpad);
int launch_pred_sample(hipStream_t stream, const PredFeat *pfs_dev, const std::vector<PredFeat> &pfs, uint32_t K,
                       uint64_t row0, uint64_t nrows, uint64_t row_id0, const int32_t *z, int32_t *z_out,
                       bool masked_only, uint64_t seed, uint64_t sweep);

// kernels_marginal.hip (msc_score_marginal; route_calls.hpp route_marginal chooses): norm = {log(n + alpha), log(n - 1 + alpha)} on the
// device; z null = no leave-one-out; map / logresp null = not wanted
int launch_marginal_norm(hipStream_t stream, const uint32_t *cnt, uint32_t K, float alpha, double *norm);
int launch_marginal_nich1(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, uint32_t K, uint32_t kpad, uint64_t row0,
                          uint64_t nrows, const int32_t *z, const float *crp, const double *norm, float *logp, int32_t *map,
                          float *logresp);
int launch_marginal_tile(hipStream_t stream, int num_cus, const FeatDesc *feats_dev, int nfeat, int nsplit, uint32_t K,
                         uint32_t kpad, uint64_t row0, uint64_t nrows, const int32_t *z, const float *own, const float *crp,
                         const double *norm, float *logp, int32_t *map, float *logresp);
int launch_row_lse(hipStream_t stream, int num_cus, const float *scores, uint64_t ld, uint32_t K, uint64_t nrows,
                   const int32_t *z, const double *norm, float *logp, int32_t *map, float *logresp);

// kernels_chains_marginal.hip (msc_chains_score_marginal): what differs per chain (per selected feature: MargFeat, and
// the call's tile plan CmPlan, both of route_calls.hpp plan_chains_marginal)
struct MargChain {
  const FeatDesc *feats;   // the chain's state: descriptors, group counts, CRP terms
  const uint32_t *cnt;
  const float *crp;
  float *logp;             // float [nrows] or null: the chain's row of chain_logp
  float alpha;
  uint32_t pad;
};
// lw / norm: double [nchains] each, written by the first launch and read by the second
int launch_chains_marginal_prep(hipStream_t stream, const MargChain *chains_dev, uint32_t nchains, uint32_t K,
                                const double *logw, double *lw, double *norm);
// mix nullable; part: double [nslices][nrows][2], needed when nslices > 1 and mix is wanted
int launch_chains_marginal(hipStream_t stream, const MargChain *chains_dev, const MargFeat *plan_dev, uint32_t nsel,
                           const CmPlan &plan, uint32_t nchains, uint32_t nslices, uint32_t K, uint32_t kpad, uint64_t row0,
                           uint64_t nrows, const double *lw, const double *norm, float *mix, double *part);

// kernels_chains_pred.hip (msc_chains_sample_predictive), after the two launches above have left lw and the chains' rows
// Lf (float [nchains][ld], through MargChain::logp): the chain of every row (-1: skipped), its group in that chain, its
// values.  chain / z: int32 [nrows]; outs_dev: one pointer a state feature (null: not drawn), a row's entry at `at` + its
// offset from row0; large: the instantiation with the large-count forms of gp / bnb (CmPlan::large); batch: the groups a
// lane sums at a time (route_calls.hpp chains_draw_batch)
int launch_chains_pick(hipStream_t stream, const double *lw, const float *Lf, uint64_t ld, uint32_t nchains, uint64_t nrows,
                       uint64_t row_id0, uint64_t seed, uint64_t sweep, int32_t *chain);
int launch_chains_draw(hipStream_t stream, const MargChain *chains_dev, bool large, int batch, uint32_t nfeat, uint32_t K,
                       uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t seed, uint64_t sweep,
                       int32_t *chain, int32_t *z);
int launch_chains_values(hipStream_t stream, const MargChain *chains_dev, void *const *outs_dev, bool light, bool heavy,
                         uint32_t nfeat, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, uint64_t at,
                         const int32_t *chain, const int32_t *z, bool masked_only, uint64_t seed, uint64_t sweep);

// kernels_query.hip (msc_zmatrix_*): counts live as upper-triangle tiles of kZmTile x kZmTile u32 (zm_tile_base); the
// batch is [rows rounded up to kZmTile][kZmBatchWords] u32, four 8-bit or two 16-bit labels a word; `bad` holds a flag
// per batch slot (kZmBatchMax of them) and then the number of flagged slots
constexpr uint32_t kZmTile = 64;
constexpr uint32_t kZmBatchWords = 256;
constexpr uint32_t kZmBatchMax = 4 * kZmBatchWords;
constexpr uint32_t kZmMaxRows = 1u << 18;
constexpr uint32_t kZmMaxLabels = 1u << 16;
inline uint32_t zm_batch_cap(bool wide) { return (wide ? 2u : 4u) * kZmBatchWords; }
int launch_zm_stage(hipStream_t stream, const int32_t *z, uint64_t ld, uint32_t nsamples, const uint32_t *rows,
                    uint32_t m, uint32_t nlabels, bool wide, uint32_t slot0, uint32_t *bad, uint32_t *batch);
int launch_zm_count(hipStream_t stream, const uint32_t *batch, uint32_t nt, bool wide, uint32_t staged,
                    const uint32_t *bad, uint32_t *counts);
int launch_zm_finish(hipStream_t stream, const uint32_t *counts, uint32_t nt, uint32_t m, const uint32_t *order,
                     bool norm, float S, void *out, uint64_t ld);

// kernels_partition.hip (msc_zmatrix_partition_*): candidates are gathered to lab[candidate][64 nt] (the selected rows'
// labels, 0 in the padding) a chunk of zm_partition_chunk(nt) at a time (a multiple of kZmPartBatch; the label buffer
// stays within 32 MiB up to m = 131072).  packed: every count is below kZmPartPackedMax (the kernel file's head says why
// that matters); the sums kernel takes kZmPartBatch candidates a workgroup then, half as many otherwise.
// launch_zm_partition_loss: tmode = the one candidate is the all-in-one partition and *T_io receives T (and *valid V);
// otherwise *T_io is read.  -2: a shape the launcher does not take
constexpr int kZmPartBatch = 64;
constexpr uint64_t kZmPartPackedMax = 1ull << 20;
uint32_t zm_partition_chunk(uint32_t nt);
int launch_zm_partition_gather(hipStream_t stream, const int32_t *cand, uint64_t ld, uint32_t ncand, const uint32_t *rows,
                               uint32_t m, uint32_t nt, int32_t *lab);
int launch_zm_partition_sums(hipStream_t stream, const uint32_t *counts, uint32_t nt, uint32_t m, bool packed,
                             const int32_t *lab, uint32_t ncand, uint64_t *w_out, uint32_t *size_out);
int launch_zm_partition_loss(hipStream_t stream, const uint32_t *counts, const uint64_t *w, const uint32_t *size,
                             uint32_t m, uint32_t ncand, bool tmode, uint64_t *T_io, int64_t *binder, double *vi,
                             uint64_t *valid);

// kernels_refine.hip (msc_zmatrix_partition_refine): greedy row moves over a dense [m][ldd] u32 copy of the counts (ldd =
// m rounded up to 4), a workgroup per start.  ids: [nstarts][ldd] 16-bit cluster ids of the positions; st: a start's
// running totals.  init turns gathered labels (launch_zm_partition_gather's lab, row stride mpad) into ids and reports
// MSC_DEVERR_REFINE_CLUSTERS for a start with more than max_clusters labels; one sweep launch is one sweep of every
// start that is still active (narrow: nsamples x m < 2^32, so 32-bit bins hold every s_k); finish writes the outputs
// (each nullable).  -2: a shape beyond the caps
constexpr uint32_t kZmRefineMaxRows = 1u << 15;
constexpr uint32_t kZmRefineMaxClusters = 1u << 10;
int bind_error_word_refine(uint32_t *word_dev);
int launch_zm_refine_init(hipStream_t stream, const int32_t *lab, uint32_t mpad, uint32_t m, uint32_t max_clusters,
                          uint32_t nstarts, uint16_t *ids, uint64_t ldi, RefineStart *st);
int launch_zm_refine_sweep(hipStream_t stream, const uint32_t *dense, uint64_t ldd, uint32_t m, uint32_t max_clusters,
                           const uint32_t *order, bool narrow, uint32_t nstarts, uint16_t *ids, RefineStart *st);
int launch_zm_refine_finish(hipStream_t stream, const uint16_t *ids, uint64_t ldi, uint32_t m, uint32_t max_clusters,
                            uint32_t nstarts, const RefineStart *st, const int64_t *binder0, int32_t *labels,
                            int64_t *binder, uint32_t *sweeps, uint64_t *moves);

// kernels_linkage.hip (msc_linkage_single): Prim's chain over the dense n x n matrix z (row stride ld), one workgroup
// of linkage::shape_for(n) (linkage_host.hpp); edges[3 i ..] = (x, y, distance) of step i.  -2: n outside [2, 65536]
int launch_linkage_prim(hipStream_t stream, const float *z, uint64_t ld, uint32_t n, double *edges);

// kernels_distance.hip (msc_partition_distances): partitions are canonicalised a chunk of kPdChunk at a time into 16-bit
// ids [chunk][ldi] (ldi = m rounded up to 4) and cluster counts k (kPdBad: more than kPdMaxClusters, reported as
// MSC_DEVERR_DISTANCE_CLUSTERS); the pair kernel then takes a block of a chunk of a against a chunk of b.  A pair's
// contingency table lives where route_pd_table (route_calls.hpp) says -- the one place that picks: in LDS while K_a K_b cells fit, else in
// the workgroup's slice of a global workspace of kPdSlices x kPdSliceCells u32 (zeroed when allocated; the kernel leaves
// it zero).  launch_pd_pairs(route) computes the pairs of the block that take `route` and leaves the others alone; the
// LDS launch also writes -1 / NaN for the pairs of a kPdBad partition.  -2: a shape the launcher does not take
constexpr uint32_t kPdMaxRows = kZmRefineMaxRows;
constexpr uint32_t kPdMaxClusters = kZmRefineMaxClusters;
constexpr uint32_t kPdBad = 0xFFFFFFFFu;
constexpr uint32_t kPdChunk = 256;
constexpr uint32_t kPdTile = 8;                              // b's a work item of the pair kernel takes
constexpr uint32_t kPdSliceCells = kPdMaxClusters * kPdMaxClusters;
constexpr uint32_t kPdSlices = 128;
struct PdPairArgs {
  const uint16_t *ids_a, *ids_b;   // [na][ldi], [nb][ldi]
  uint64_t ldi;
  const uint32_t *k_a, *k_b;       // cluster counts of the block's partitions
  uint32_t m, na, nb;              // rows; partitions of the block
  uint32_t a0, b0;                 // the block's first partitions in their sets
  uint64_t ldo;                    // row stride of the outputs: the whole nb
  uint32_t mirror;                 // b is a: pairs with b0 + j < a0 + i are left out, the others are written twice
  const double *log2tab;           // [m + 1]
  uint32_t *table;                 // the global workspace (null on the LDS route)
  int64_t *pairs_ab;               // [.][ldo], nullable
  double *nlogn_ab;
};
int bind_error_word_distance(uint32_t *word_dev);
int launch_pd_log2(hipStream_t stream, double *tab, uint32_t n);
int launch_pd_canon(hipStream_t stream, const int32_t *lab, uint64_t ld, uint32_t m, uint32_t nparts, const double *log2tab,
                    uint32_t part0, uint16_t *ids, uint64_t ldi, uint32_t *k, int64_t *pairs, double *nlogn,
                    uint32_t *nclusters);
int launch_pd_pairs(hipStream_t stream, int num_cus, PdRoute route, const PdPairArgs &p);

// kernels_refine_vi.hip (msc_partition_refine_vi): greedy row moves under the exact expected VI, a workgroup per start.
// launch_vi_canon turns samples (cap = kViMaxClusters; count receives the cluster counts L) or starts (cap =
// max_clusters; st receives the running totals) into 16-bit ids [n][ldi] and reports MSC_DEVERR_VI_CLUSTERS for one with
// more clusters than cap; launch_vi_rows makes off[S + 1] (the running sum of L) and row[m][S] = off[s] + id_s[a];
// launch_vi_count fills the zeroed u16 cells [nstarts][off[S] kcap] of the starts; one launch_vi_sweep is one sweep of
// every start that is still active; launch_vi_finish writes the outputs (each nullable).  -2: a shape beyond the caps
constexpr uint32_t kViMaxRows = kZmRefineMaxRows;
constexpr uint32_t kViMaxClusters = kZmRefineMaxClusters;
constexpr uint32_t kViMaxSamples = 1u << 16;
constexpr uint32_t kViCellPad = 32;                          // ids a block of cells; kcap: max_clusters rounded up to it
struct ViSweepArgs {
  const uint32_t *row;             // [m][S]
  uint32_t S, m, max_clusters, kcap;
  const uint32_t *order;           // nullable
  const int64_t *G;                // [m]: G(n) = F(n + 1) - F(n) of msc_vi_table
  uint16_t *ids;                   // [nstarts][ldi]
  uint64_t ldi;
  uint16_t *cells;                 // [nstarts][cells_per_start]
  uint64_t cells_per_start;
  RefineStart *st;
};
// (the sweep kernel's instantiation: route_calls.hpp route_vi_refine)
int bind_error_word_refine_vi(uint32_t *word_dev);
int launch_vi_canon(hipStream_t stream, const int32_t *lab, uint64_t ld, uint32_t m, uint32_t cap, uint32_t nparts,
                    uint32_t part0, uint16_t *ids, uint64_t ldi, uint32_t *count, RefineStart *st);
int launch_vi_rows(hipStream_t stream, const uint16_t *ids, uint64_t ldi, const uint32_t *L, uint32_t S, uint32_t m,
                   uint32_t *off, uint32_t *row);
int launch_vi_count(hipStream_t stream, int num_cus, const ViSweepArgs &p, uint32_t nstarts);
int launch_vi_sweep(hipStream_t stream, const ViSweepArgs &p, uint32_t nstarts);
int launch_vi_finish(hipStream_t stream, const uint16_t *ids, uint64_t ldi, uint32_t m, uint32_t max_clusters,
                     uint32_t nstarts, const RefineStart *st, int32_t *labels, int64_t *decrease, uint32_t *sweeps,
                     uint64_t *moves);

}  // namespace msc
