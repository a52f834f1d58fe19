// route_calls.hpp -- what every other call chooses: the blocked sweep and split-merge, the sequential sweep and the chain
// ensembles, the row predictive density of a state and of an ensemble, the partition summaries.  The rule of route.hpp
// holds here too: pure functions of a state's facts (RouteFacts), the environment's switches and plain numbers; host
// only, no object of the library.  The units fill the facts (abi.cpp route_facts_now) and launch what a route returns;
// tests/cxx/test_route_calls.cpp builds this header with the host compiler and holds every function to its rule.
#pragma once

#include <string>

#include "blocked_niw.hpp"
#include "blocked_post.hpp"
#include "route.hpp"

namespace msc {

// ---- the blocked Gibbs sampler and the split-merge move (kernels_blocked.hip, kernels_splitmerge.hip) ------------------
// Which assign kernel a state takes, and whether the sampler takes it at all.  By the state alone: every kernel adds a
// row's terms in the same order (blk_tile_scores), so a sub-range draws what the whole draws whichever is chosen.
//   nich1   a single nich column: the row's value in a register, no LDS
//   staged  up to 256 features: the workgroup's row values staged in LDS once, [feature][row] -- 256 rows a workgroup up
//           to 32 features, 128 up to 64, 64 beyond (32 KiB at most, 64 KiB from 129 features on)
//   global  more features than that: the values re-read from the columns for every eight slots
// The split-merge move takes the same families and shapes (every kernel adds a row's terms in the same order, so the
// choice never changes a bit); its staged kernel holds one feature fewer.  who: the caller, as the message names it.
//   niw1    the blocked sweep alone (niw_alone): a state whose ONLY feature is one niw column of dim <= 32 -- kernels of
//           its own (kernels_blocked_niw.hip: the parameter draw leaves matrices, the assign pass runs on the f64 matrix
//           pipe, 256 rows a workgroup).  A niw feature beside others, and any niw state in split-merge, is refused.
enum class BlockedKernel { nich1, staged, global, niw1 };
struct BlockedRoute { int rc = MSC_OK; std::string why; BlockedKernel kernel = BlockedKernel::global; uint32_t block = 256; };
constexpr uint32_t kBlockedStagedMax = 256;             // (at most 32 KiB of LDS a workgroup: several a compute unit)
constexpr uint32_t kSplitMergeStagedMax = 255;          // (the codes and the waves' sums within 64 KiB of LDS a workgroup)
inline BlockedRoute route_blocked(const RouteFacts &rf, const char *who, uint32_t staged_max, bool niw_alone = false) {
  BlockedRoute r;
  const auto refuse = [&](const char *what) { r.rc = MSC_EUNSUPPORTED, r.why = std::string(who) + what; return r; };
  if (niw_alone && rf.nfeat == 1 && rf.feats.size() == 1 && rf.feats[0].family == MSC_NIW) {
    // (kNiwMaxDim = 32, two 16-blocks: k_blocked_assign_niw<1>, <2>)
    if (rf.feats[0].dim > blocked::kNiwMaxDim) return refuse(" takes a niw feature of dimension at most 32");
    r.kernel = BlockedKernel::niw1;
    return r;
  }
  for (const RouteFeat &h : rf.feats)
    if (h.family == MSC_NIW || h.family == MSC_DM || h.family == MSC_BBNC)
      return refuse(" takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
  if (rf.nfeat >= blocked::kStickTag) return refuse(" takes fewer than 32767 features");
  if (rf.nfeat == 1 && rf.feats[0].family == MSC_NICH) r.kernel = BlockedKernel::nich1;
  else if (rf.nfeat <= staged_max) {
    r.kernel = BlockedKernel::staged;
    r.block = rf.nfeat <= 32 ? 256 : rf.nfeat <= 64 ? 128 : 64;
  }
  return r;
}
inline BlockedRoute route_sweep_blocked(const RouteFacts &rf) { return route_blocked(rf, "the blocked sweep", kBlockedStagedMax, true); }
inline BlockedRoute route_splitmerge(const RouteFacts &rf) { return route_blocked(rf, "split-merge", kSplitMergeStagedMax); }

// ---- the sequential sweep and the ensembles of such chains (kernels_seq.hip, kernels_chains_sm.hip) ---------------------
constexpr uint32_t kSeqMaxGroups = 8192;   // the groups' scores sit in LDS (32 KiB)
constexpr int kSeqMaxFeat = 256;           // features whose row values the workgroup stages
constexpr double kSeqLaunchUs = 20000.0;   // what one launch may take (estimated)
constexpr uint64_t kSeqMaxVisitsPerLaunch = 10000;

// whether the sequential kernel takes a state: ok, or the status and why not
struct SeqRoute { int rc = MSC_OK; const char *why = ""; };
inline SeqRoute route_sequential(const RouteFacts &rf) {
  const auto refuse = [](const char *why) { return SeqRoute{MSC_EUNSUPPORTED, why}; };
  // niw, dm: prepare kernels of their own (msc_entity_op sends them down the general path); bbnc: a slot that empties
  // mid-sweep would be offered with a stale p (free slots' p is drawn between sweeps, mixture_state refresh_free_slots)
  for (const RouteFeat &h : rf.feats)
    if (h.family == MSC_NIW || h.family == MSC_DM || h.family == MSC_BBNC)
      return refuse("the sequential sweep takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
  if (rf.nfeat > (uint32_t)kSeqMaxFeat) return refuse("the sequential sweep takes at most 256 features");
  if (rf.K > kSeqMaxGroups) return refuse("the sequential sweep takes at most 8192 groups");
  return SeqRoute();
}

// An upper estimate of one row visit, in microseconds: a fixed part (barriers, the draw, a nich prepare) plus the table
// entries a leave and a join rebuild and the (group, feature) scores; fitted to the visits of profiles/sequential.txt (one
// nich column to the C3 mix, K = 16 to 1024): launches measured there at 11.9 ms on average, 26.3 ms the longest
inline double seq_visit_us(const RouteFacts &rf) {
  double rows = 0.0;                              // table entries prepare_group writes per (feature, group)
  for (const RouteFeat &h : rf.feats) {
    switch (h.family) {
      case MSC_BB: rows += 4; break;
      case MSC_GP:
      case MSC_BNB: rows += 2.0 * h.vcap + 4; break;
      case MSC_DD: rows += 2.0 * h.dim + 2; break;
      case MSC_NICH: rows += 14; break;
      default: break;
    }
  }
  return 16.0 + 0.02 * 2.0 * rows + 0.007 * (double)rf.K * (double)rf.nfeat;
}

// Whole units (row visits, proposals) of every chain that one launch takes: what one chain may take in kSeqLaunchUs at
// unit_us a unit, kSeqMaxVisitsPerLaunch at most, divided by the rounds the grid runs in -- at these kernels' register
// counts one workgroup is resident per CU.  At least one: the least a launch can take.  With one chain the grid runs in
// one round, so this is max(1, min(kSeqMaxVisitsPerLaunch, kSeqLaunchUs / unit_us)) cut to an integer for every
// unit_us > 0: the budget of msc_sweep_sequential.
inline uint64_t units_per_launch(uint32_t nchains, int num_cus, double unit_us) {
  const uint64_t cus = (uint64_t)std::max(1, num_cus), rounds = std::max<uint64_t>(1, ((uint64_t)nchains + cus - 1) / cus);
  const double one = std::max(1.0, std::min((double)kSeqMaxVisitsPerLaunch, kSeqLaunchUs / unit_us));
  return std::max<uint64_t>(1, (uint64_t)one / rounds);
}

// ---- the row predictive density of a state (kernels_marginal.hip) ---------------------------------------------------
// Which kernels reduce a state's rows.  By the state and view_rows alone (THE SHARD RULE of route_sweep; no argument
// carries the call's rows): the fused kernels and the score kernels add a row's terms in different orders, so a call
// over a sub-range must take what the whole call takes.
//   nich1    a single nich feature (masked or not) up to 1024 groups: k_marginal_nich1, the own-group values computed inside
//   tile     scalar features within the tables (no niw, no dm, no count beyond a table), K <= 256, a view of at least
//            kTailMinRows rows (fewer rows do not fill the chip with 128-row workgroups: the score pass has shapes for
//            them), on plans whose SCORE pass is the plain tile kernel too (tile_path == MSC_PATH_TILE): k_loo_own, then
//            k_marginal_tile over the fused plan.  A plan with kernels of its own (role-split, nich-only, lookups-only)
//            goes the generic way: its score pass plus k_row_lse beats the plain tile form (C3, 10^6 x 256: DESIGN.md 6g)
//            until a fused form of those kernels exists.  MSC_MARGINAL_TILE=1 / 0 sends every such plan / none to the tile
//            kernel (how the two were measured against each other).
//   generic  everything else: run_score (leave-one-out + prior) into the scratch chunk, then k_row_lse over it
enum class MarginalKind { nich1, tile, generic };
inline MarginalKind route_marginal(const RouteFacts &rf, const Switches &sw) {
  if (!sweep_plain(rf)) return MarginalKind::generic;
  if (rf.nich1) return rf.K <= 1024 ? MarginalKind::nich1 : MarginalKind::generic;
  if (!rf.has_dm && rf.K <= 256 && rf.view_rows >= kTailMinRows) {
    const int forced = sw.marginal_tile;
    if (forced >= 0 ? forced != 0 : rf.plan.tile_path == MSC_PATH_TILE) return MarginalKind::tile;
  }
  return MarginalKind::generic;
}

// The row chunk of the materialised paths (SweepKind::generic, MarginalKind::generic): rows of ld = K rounded up to 64
// floats, not of the padded table width (at K = 300 the chunk is 320 wide, not 512 -- neither the score kernels nor the
// readers touch a row beyond K), up to 4 GiB of scores a chunk (288 GB of HBM: the scratch is not what runs out).  Fewer
// and larger launches beat keeping the chunk cache-resident (single nich, 1M rows x 300 groups, 32 / 64 / 128 / 256 /
// 512 MiB: 1.88 / 1.55 / 1.28 / 1.13 / 1.05 ms), a state with niw features wants >= 4 waves per SIMD on its MFMA kernel,
// and the leave-one-out pass takes its staged kernel only when the rows fill the chip -- C3's columns at K = 512, 1M rows:
// 5.39 ms a sweep step with 256 MiB chunks (eight of them), 4.95 with 1 GiB, 4.63 with the whole 2 GiB at once.
struct ScoreChunk { uint64_t ld, chunk; };
inline ScoreChunk score_chunk(uint32_t K, uint32_t kpad, uint64_t nrows) {
  const uint64_t ld = std::min<uint64_t>(kpad, ((uint64_t)K + 63) & ~63ull);
  return ScoreChunk{ld, std::max<uint64_t>(1, std::min<uint64_t>((4096ull << 20) / (ld * sizeof(float)), nrows))};
}

// ---- the row predictive density over an ensemble and its predictive draws (kernels_chains_marginal.hip, _pred.hip) ------
// How the chains are cut over the grid's second dimension.  By the ensemble and view_rows alone (THE SHARD RULE of
// route_marginal): the slices' parts are merged in slice order, so a call over a sub-range must cut as the whole call does.
// A view of fewer than four workgroups of 256 rows a compute unit (what its LDS holds) is filled up with slices, at most
// one a chain.  (The launcher gives a slice ceil(nchains / slices) chains: every slice but the last full, the last not empty.)
inline uint32_t route_chains_marginal(uint32_t nchains, uint64_t view_rows, int num_cus) {
  const uint32_t n = nchains;
  const uint64_t blocks = std::max<uint64_t>(1, (view_rows + 255) / 256);
  const uint64_t want = 4ull * (uint64_t)std::max(1, num_cus);
  if (blocks >= want || n == 0) return 1;
  const uint32_t slices = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, 1024), (want + blocks - 1) / blocks);
  const uint32_t per = (n + slices - 1) / slices;
  return (n + per - 1) / per;
}

// The tile plan of a call: which selected features' tables are staged, where, and how many groups a tile holds.  From the
// features alone (their families, dims and the bound column's vcap) and K: every member of an ensemble has the same, and
// neither the rows nor the number of chains enters -- a row's bits depend on the tile size.
struct MargFeat {
  uint32_t f;              // the feature's index in the state
  uint32_t off;            // first float of its block in the LDS tile; kCmNotStaged: its tables are read from global memory
  uint32_t rows;           // table rows of the block (cm_table_rows: bb 2, dd dim, gp / bnb vcap, nich 6, noop 0)
  uint32_t pad;
};
struct CmPlan {
  uint32_t TG = 0;          // groups a tile
  uint32_t TS = 0;          // floats between two table rows of a tile: TG | 1
  uint32_t lds_floats = 0;  // the launch's dynamic LDS
  bool wide = false;        // tiles of whole batches of 32 groups: the wide-batch instantiation
  bool large = false;       // a selected gp / bnb column may hold counts beyond the exact table: the instantiation with the large-count forms
};
constexpr uint32_t kCmTileFloats = 10240;   // 40 KiB of LDS a workgroup: four workgroups of 256 rows a CU
constexpr uint32_t kCmMinTile = 32;         // a feature is staged only while a tile of this many groups still fits
// groups a lane sums in registers before it pushes them: what a feature costs a lane apart from its table reads -- its
// plan entry, the descriptor's fields, the row's value -- is paid once a batch, so tiles of whole wide batches take
// kCmBatchWide; narrower tiles (few groups, or tables too tall for 32 groups of them) take kCmBatch
constexpr int kCmBatch = 8, kCmBatchWide = 32;
constexpr uint32_t kCmNotStaged = 0xffffffffu;  // MargFeat::off of a feature whose tables stay in global memory
// out[nsel]: the plan of the selected features sel[nsel] (ascending state indices); feats: the state's (RouteFacts::feats)
inline CmPlan plan_chains_marginal(const RouteFeat *feats, const uint32_t *sel, uint32_t nsel, uint32_t K, MargFeat *out) {
  // features are staged in order while a tile of kCmMinTile groups of them fits; the others read global memory
  const uint32_t min_ts = (std::min<uint32_t>(K, kCmMinTile)) | 1u;
  CmPlan p;
  uint32_t rows = 2;
  for (uint32_t i = 0; i < nsel; i++) {
    const RouteFeat &d = feats[sel[i]];
    const uint32_t r = cm_table_rows(d.family, d.dim, d.vcap);
    if (is_count_family(d.family) && d.vcap >= kGpMaxTable) p.large = true;   // (vcap = min(column max + 1, the cap))
    MargFeat &m = out[i];
    m.f = sel[i];
    m.rows = r;
    m.pad = 0;
    if (r == 0 || (uint64_t)(rows + r) * min_ts + kCmBatchWide > kCmTileFloats) {
      m.off = kCmNotStaged;
      if (r == 0) m.off = 0;                                // (noop: nothing to stage, nothing to read)
      continue;
    }
    m.off = rows;                                           // (in rows for now)
    rows += r;
  }
  uint32_t tg = std::min<uint32_t>(K, (kCmTileFloats - kCmBatchWide) / rows - 1u);
  p.wide = tg >= (uint32_t)kCmBatchWide;
  const uint32_t batch = p.wide ? kCmBatchWide : kCmBatch;
  if (tg > batch) tg -= tg % batch;                         // whole batches
  p.TG = std::max<uint32_t>(tg, 1u);
  p.TS = p.TG | 1u;
  p.lds_floats = rows * p.TS + kCmBatchWide;                // (a batch's reads past the tile's groups stay inside)
  for (uint32_t i = 0; i < nsel; i++)
    if (out[i].off != kCmNotStaged) out[i].off *= p.TS;
  return p;
}

// groups a lane of k_chains_draw sums in registers at a time: kCpBatchWide from kCpWideFrom groups on, kCpBatch below and
// with the large-count forms (beside a wide batch they spill)
constexpr int kCpBatch = 8, kCpBatchWide = 32;
constexpr uint32_t kCpWideFrom = 64;
inline int chains_draw_batch(uint32_t K, bool large) { return !large && K >= kCpWideFrom ? kCpBatchWide : kCpBatch; }

// The rows of msc_chains_sample_predictive go through the handle's scratch -- the chains' rows Lf [nchains][chunk] floats,
// then the rows' chain and group -- a chunk at a time: at most kPredScratchBytes of Lf and kPredChunkRows rows.  A row
// depends on the row alone, so the cut moves no bit.  A power of two from 4096 on: the buffers a growing scratch retires
// stay with the handle, and add up to less than the last one.
constexpr uint64_t kPredScratchBytes = 256ull << 20;
constexpr uint64_t kPredChunkRows = 1ull << 18;
inline uint64_t pred_chunk(uint32_t nchains, uint64_t nrows) {
  uint64_t chunk = 4096;
  while (chunk < nrows && chunk < kPredChunkRows && 2 * chunk * nchains * sizeof(float) <= kPredScratchBytes) chunk *= 2;
  return chunk;
}

// ---- the partition summaries (kernels_distance.hip, kernels_refine_vi.hip) --------------------------------------------
// where a pair's contingency table of ka x kb cells lives: in LDS while the cells fit, else in the workgroup's slice of
// the global workspace.  The one place that picks; kernels_distance.hip asks it on the device too.
constexpr uint32_t kPdLdsCells = 15u * 1024u;                // 60 KiB of the 64 a workgroup declares; the rest holds the partial sums
enum class PdRoute { lds, global };
MSC_HOST_DEVICE inline PdRoute route_pd_table(uint32_t ka, uint32_t kb) {
  return (uint64_t)ka * kb <= kPdLdsCells ? PdRoute::lds : PdRoute::global;
}
// the one place that picks the VI sweep kernel's instantiation: the 64-id slots a thread keeps sums for in one pass over
// the samples, 1, 2, 4 or 8 (sixteen would not fit the 128 registers of a thread of sixteen waves: past 512 ids in use
// the kernel makes two passes)
inline int route_vi_refine(uint32_t kcap) {
  int nk = 1;
  while (nk < 8 && (uint32_t)nk * 64u < kcap) nk *= 2;
  return nk;
}

}  // namespace msc
