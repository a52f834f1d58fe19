// route.hpp -- which kernels a score pass and a sweep take: the routes and the rules they share, as pure functions of a
// state's facts (RouteFacts), the environment's switches (Switches) and the call's rows.  Host only: no HIP header, no
// object of the library -- abi.cpp fills the facts where a state is planned or bound and launches what a route returns;
// tests/cxx/test_route.cpp builds this header with the host compiler and holds the routes to their rules, THE SHARD RULE
// among them.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "feat_desc.hpp"

namespace msc {

// What the library reads from the environment, all of it here (INTEGRATION.md "Environment" says what each switch does):
// read afresh by every call that plans, routes or allocates, so that a test may set a switch between two calls
// (abi_internal.hpp read_switches).
struct Switches {
  bool tail_forced = false, no_narrow_tail = false, no_bb_fuse = false, sweep_graph = false;
  uint64_t tail_min_rows = 0;                           // (tail_forced)
  int loo_lds = -1, sweep_nich1 = 0, alloc_candidates = 12;
  int marginal_tile = -1;                               // MSC_MARGINAL_TILE: 1 / 0 = the fused tile kernel for every plan it takes / for none

  float alloc_accept_gbps = 6650.f;
};

// What the routes read of a state.  Everything but view_rows is fixed once the state is planned and its view bound
// (abi.cpp upload_desc builds it there); view_rows -- the bound view's rows, or those of the whole a sharded driver
// announced -- is refreshed by the call that routes.
struct RouteFeat {
  int family = 0;
  uint32_t dim = 0, vcap = 0;
  bool beyond_table = false;      // gp / bnb: the bound column (or the stated bound) holds counts beyond the exact table; dm: row totals
};
struct RouteFacts {
  uint32_t K = 0, kpad = 0;
  int num_cus = 256;
  bool nich1 = false, has_dm = false;
  uint32_t n_niw = 0, nfeat = 0;
  TilePlan plan;
  std::vector<RouteFeat> feats;
  uint64_t view_rows = 0;
  // the two limits that live with their kernels (kernels_sweep.hip): sweep_niw1_max_groups(dim) of feature 0,
  // sweep_nich1_rows_max_groups()
  int niw1_max_groups = 0;
  uint32_t nich1_rows_max_groups = 0;
};

// What a pass over `nrows` rows costs, in microseconds, on either kind of kernel -- only to choose between them.  The
// prices follow the PLAN (tile_plan.hpp plan_prices; measured on one MI355X, 1M rows: tools/scans/c3_pieces.py --spec=...,
// tail_threshold.py, small_n.py, n_scan.py) -- with C3's prices for every plan (round 3) a state of lookup features only took the
// lane <-> row kernel up to 128 groups and ran 32 bool columns at 0.58 ms (K = 128) and 0.87 (K = 64) where the tile pass
// takes 0.34:
//   tile kernels: one workgroup of 128 rows per CU and round; a round costs ~6 us + 0.45 a staged lookup feature + 0.012 a
//   staged table row + 1.5 a nich feature (the role-split kernels overlap the two halves: half the nich share; the
//   nich-only kernels 1.3 a feature); C3: 50 us a round of a scoring pass, 55 of a fused sweep; at most 128 groups on the
//   role-split / nich-only kernels (PAIR mode, 256 rows a workgroup): kPairTileShare of that;
//   lane <-> row kernel: a launch of g groups takes ~2 us + g (0.5 + 0.03 a lookup feature + 0.057 a nich feature) per round
//   of 1024 rows a CU (two workgroups of 512); C3: 2 + 2.5 g (round 3 priced it 30 + 1.7 g: the same at 32-48 groups).
// (struct PlanCost: feat_desc.hpp -- the state keeps its plan's)
inline double tile_rounds_us(uint64_t workgroups, int num_cus, bool sweep, const PlanCost &pc = PlanCost()) {
  return (sweep ? pc.sweep_round_us : pc.tile_round_us) * (double)((workgroups + (uint64_t)num_cus - 1) / (uint64_t)num_cus);
}
inline double tail_rows_us(uint32_t groups, bool exact, uint64_t nrows, int num_cus, const PlanCost &pc = PlanCost()) {
  const uint32_t widest = exact ? 32u : 64u, nblk = (groups + widest - 1) / widest;      // (as launch_score_tail cuts them)
  const uint32_t per = ((groups + nblk - 1) / nblk + 15u) / 16u * 16u;
  // (a round of 1024 rows a CU that is not full costs less than a whole one -- the workgroups are 512 rows, most CUs get
  // none -- but not in proportion: sixteen dd columns, two exact launches: 0.066 ms at 262k rows, 0.050 at 100k, ~0.04 at 70k)
  const double frac = (double)nrows / (1024.0 * num_cus);
  const double rounds = frac >= 1.0 ? frac : std::max(0.6, 0.4 + 0.6 * frac);      // (100k rows, 0.38 of a round: 0.75 of its price)
  return (double)nblk * (pc.tail_fixed_us + pc.tail_group_us * per) * rounds;
}

// Can k_score_tail_rows take this plan's partly filled last tile?  A plan it takes (plan_layout), at most kTailMaxGroups
// groups there, and the largest staged table beside the second phase's block (64 floats a nich feature) in 64 KiB of LDS.
inline bool narrow_tail_fits(const RouteFacts &rf) {
  const size_t nich_bytes = (size_t)(rf.plan.fuse_nfeat - rf.plan.fuse_split) * 64 * sizeof(float);
  return rf.plan.tile_narrow_tail_ok && rf.K - (rf.kpad - kGroupTile) <= kTailMaxGroups &&
         nich_bytes + (size_t)std::max<uint32_t>(1u, rf.plan.tail_max_rows) * kTailStride * sizeof(float) <= 64u * 1024u;
}

// PAIR mode of the role-split / nich-only / lookups-only kernels: one k-tile of at most 128 groups
inline bool pair_path(ScorePath path, uint32_t K) {
  return (path == MSC_PATH_TILE_ROLES || path == MSC_PATH_NICH_PACK || path == MSC_PATH_LOOKUPS) && K <= 128;
}

// K <= 64 and nothing but scalar families whose tables all fit 64 KiB of LDS at 4 L groups per row: the narrow tiling
// (kernels_sweep.hip k_narrow).  Returns L = lanes per row (4 / 8 / 16) or 0, and the table rows to stage.
inline int narrow_lanes(const RouteFacts &rf, const Switches &sw, uint32_t *table_rows) {
  // (32 lanes per row for K <= 128 was measured and loses to the 256-group tiling: 8 bb at K = 100, 0.52 against 0.20 ms)
  if (rf.K > 64) return 0;
  // Views of many rows leave it to the lane <-> row kernel (round 3's; by view_rows: route_sweep's shard rule).  At a million rows that kernel is 1.3-2.7x the faster one (tools/scans/k_monotone.sh:
  // sixteen dd32 columns at K = 32 0.34 -> 0.13 ms, 8 bb + 8 nich at K = 64 0.48 -> 0.26, sixteen nich at K = 32 0.30 -> 0.18);
  // this tiling is for the small problems it was made for (C1: 10k rows, 8 us a pass): views below kNarrowMaxRows rows.
  if (rf.view_rows >= kNarrowMaxRows && rf.plan.tile_narrow_tail_ok && !sw.tail_forced) return 0;
  const int L = rf.K <= 16 ? 4 : rf.K <= 32 ? 8 : 16;
  uint32_t rows = 0;
  for (uint32_t f = 0; f < rf.nfeat; f++) {
    const RouteFeat &h = rf.feats[f];
    switch (h.family) {
      case MSC_BB: case MSC_BBNC: rows += 2; break;
      case MSC_NICH: rows += 6; break;                                      // (NICH_ROWS)
      case MSC_DD: rows += h.dim; break;
      case MSC_GP: case MSC_BNB:
        if (h.beyond_table) return 0;
        rows += h.vcap;
        break;
      case MSC_NOOP: break;
      default: return 0;                                                    // niw, dm: their own kernels
    }
  }
  if ((size_t)rows * L * 16 > 64u * 1024u) return 0;
  // ... and only where it is the cheaper tiling for THIS plan (by the plan alone: the narrow kernel adds the features in
  // the caller's order, the tile kernels in the plan's).
  // Per million rows, us, at 16 lanes a row (tools/scans/grid_scan.py at 100k rows, k_monotone.sh): a bb column 30 (the tile
  // plan fuses four of them into one lookup, this tiling cannot), dd / gp 50, nich 60, half of it at 8 lanes and no less at
  // 4; against the tile kernels' rounds at the plan's price (PlanCost; up to 128 groups the role-split /
  // nich-only kernels run in PAIR mode).  32 bool columns at K = 64, 1M rows: 0.86 ms here, 0.30 on the tile kernel; 64 at
  // K = 8, 100k rows: 0.10 against 0.04.
  {
    double us = 0;
    for (uint32_t f = 0; f < rf.nfeat; f++) {
      const int fam = rf.feats[f].family;
      us += fam == MSC_BB || fam == MSC_BBNC ? 30.0 : fam == MSC_NICH ? 60.0 : fam == MSC_NOOP ? 0.0 : 50.0;
    }
    us *= std::max(L, 8) / 16.0;
    const double tile = rf.plan.plan_cost.tile_round_us * (1.0e6 / 128.0 / rf.num_cus) * (pair_path(rf.plan.tile_path, rf.K) ? kPairTileShare : 1.0);
    if (us > 1.25 * tile) return 0;
  }
  *table_rows = rows;
  return L;
}

// Which kernels score `nrows` rows: k_narrow when `lanes` is set (narrow_lanes: by view_rows), else the scalar
// features' pass on `path` as `shape` says -- by the call's rows: every shape gives the tile kernels' bits --, then niw's.
// (path MSC_PATH_NICH1: shape.nich1 is the caller's to set -- abi.cpp nich1_shape_for reads the context's placement lists)
struct ScoreRoute { int lanes = 0; uint32_t table_rows = 0; ScorePath path = MSC_PATH_TILE; ScoreShape shape; };
inline ScoreRoute route_score(const RouteFacts &rf, const Switches &sw, uint64_t nrows) {
  ScoreRoute r;
  r.lanes = narrow_lanes(rf, sw, &r.table_rows);
  r.path = rf.nich1 ? MSC_PATH_NICH1 : rf.has_dm ? MSC_PATH_TILE_DM : rf.plan.tile_path;
  if (r.lanes || r.path == MSC_PATH_NICH1) return r;
  // few rows: the chunks -- serial chains, feature after feature -- spread over the chip in ONE round at 4 or 2 rows a
  // wave (4 only while the 64-row workgroups fit one round: 20000 rows made 313 of them, 0.113 ms, where 157 of 128 take one)
  const int cus = rf.num_cus;
  const uint32_t ktiles = rf.kpad / kGroupTile, last_groups = rf.K - (ktiles - 1) * kGroupTile;
  const uint64_t round = (uint64_t)cus / ktiles;
  const bool small4 = r.path != MSC_PATH_TILE_DM && (nrows + 63) / 64 <= round, small2 = small4 && (nrows + 31) / 32 <= round;
  r.shape.wave_rows = small2 ? 2 : small4 ? 4 : 8;
  r.shape.pair = !small4 && pair_path(r.path, rf.K);
  // a LAST tile of 65 .. 128 groups beyond full ones on the role-split kernels: PAIR mode at that tile (round 5), ~0.62 of a
  // full tile's price where the lane <-> row kernel takes two or three launches
  // else the last tile on the lane <-> row kernel when the plan allows and the rows are many (few -- a per-entity call's one
  // -- are better off with lanes as groups): whichever the cost model above prices lower for these rows
  if (ktiles > 1 && r.path == MSC_PATH_TILE_ROLES && !small4 && last_groups > 64 && last_groups <= 128) r.shape.last = LastTile::pair;
  if (r.shape.last == LastTile::pair || !narrow_tail_fits(rf)) return r;
  const PlanCost &pc = rf.plan.plan_cost;
  const uint64_t c128 = (nrows + 127) / 128;
  const double tile_us = (r.shape.pair ? kPairTileShare : 1.0) *
                         (tile_rounds_us(c128 * ktiles, cus, false, pc) - (ktiles > 1 ? tile_rounds_us(c128 * (ktiles - 1), cus, false, pc) : 0.0));
  const bool many_rows = sw.tail_forced ? nrows >= sw.tail_min_rows
                                        : nrows >= kTailMinRows && tail_rows_us(last_groups, true, nrows, cus, pc) < tile_us;
  if (many_rows) r.shape.last = LastTile::rows;
  return r;
}

// score + sample in one kernel; niw and gp-beyond-table features and wide K need the materialised path
// one niw feature of small dimension on few groups: the fused k_sweep_niw1
inline bool sweep_is_niw1(const RouteFacts &rf) {
  return rf.nfeat == 1 && rf.feats[0].family == MSC_NIW && (int)rf.K <= rf.niw1_max_groups;
}

// the lane <-> row kernel fills the chip from ~260k rows on; with fewer the tile kernels' rounds of 128-row chunks can be
// shorter.  Decided on the view's row count, so every row range of it takes the same kernels.
// (priced with the cost model above: the lane <-> row launches -- plus, beyond 64 groups, the trip through
// 128 floats per row and the row sampler -- against the rounds of the fused tile sweep kernel; for a tail beyond a full
// tile, against one more tile pass, the materialised matrix and the sampler)
// PAIR mode of the role-split sweep kernel (at most 128 groups; kernels_sweep.hip): its draw associates a row's entries
// differently from the other tile kernels'
inline bool sweep_pair_mode(const RouteFacts &rf) {
  return rf.view_rows >= kTailMinRows && pair_path(rf.plan.tile_path, rf.K);
}
inline bool sweep_rows_pays(const RouteFacts &rf, const Switches &sw, uint32_t groups) {
  const uint64_t rows = rf.view_rows;
  if (sw.tail_forced) return rows >= sw.tail_min_rows;
  if (rows < kTailMinRows) return false;
  const int cus = rf.num_cus;
  const uint64_t c128 = (rows + 127) / 128;
  const bool tail = groups < rf.K;                        // the groups beyond a full first tile
  const double sample_us = [&](uint64_t floats_per_row) { return 30.0 + (double)rows * floats_per_row * 4.0 / 2.0e6; }(tail ? rf.K : 128);
  double rows_us = tail_rows_us(groups, false, rows, cus, rf.plan.plan_cost), tile_us;
  if (tail) {
    rows_us *= 1.15;                                      // (the tile kernel's instantiation that reads the tail is that much slower)
    tile_us = tile_rounds_us(c128, cus, false, rf.plan.plan_cost) + sample_us;                // one more tile pass, then the sampler over K floats a row
  } else {
    if (groups > 64) rows_us += sample_us;
    // (a fused sweep round = the scoring round -- its PAIR share up to 128 groups -- + the draws, which do not shrink with the
    // plan or the mode: ~2.5 us a round; 8 bb columns at K = 64: 0.18 ms in PAIR mode, 0.10 on the lane <-> row kernel)
    PlanCost pc = rf.plan.plan_cost;
    pc.sweep_round_us = pc.tile_round_us * (sweep_pair_mode(rf) ? kPairTileShare : 1.0) + 2.5;
    tile_us = tile_rounds_us(c128, cus, true, pc);
  }
  return rows_us < tile_us;
}

// no niw feature and no count beyond the tables: what the fused sweep kernels score
inline bool sweep_plain(const RouteFacts &rf) {
  for (uint32_t f = 0; f < rf.nfeat; f++) if (rf.feats[f].beyond_table) return false;
  return rf.n_niw == 0;
}

inline bool sweep_is_fused(const RouteFacts &rf) {
  if (sweep_is_niw1(rf)) return true;
  if (!sweep_plain(rf)) return false;
  return rf.nich1 ? rf.K <= rf.nich1_rows_max_groups : rf.K <= 256;
}

// How a sweep assigns a state's rows: the kind sweep_assign_impl switches on, and what that kind needs -- every kernel the
// sweep launches, decided here (the launchers take it as it is).
// THE SHARD RULE: some kernels add a row's terms in a different order from others, so the choice depends only on the plan
// and on view_rows (the bound view's, or the whole's a sharded driver announced), never on the call's rows: that is what
// makes a shard draw the same bits as the whole.  (A launch shape that draws the same bits at every row count may follow
// the call's rows; the test that holds it so is named where it is chosen.)  Recomputed on every call (the bound view, the hint and the switches read
// here change between calls).  tests/cxx/test_route.cpp holds the rule over a grid of plans, K and view_rows.
// (rows: K <= 64, the lane <-> row kernel draws its own row; rows_sampler: up to 128 groups, its scores into 128 floats a
// row, then the row sampler; roles_tail: 256 < K <= 384, the groups beyond the tile from the narrow kernel -- or, 65 .. 128
// of them on a role-split plan, the role-split kernel in PAIR mode (tail_pair) -- into tail_ld floats a row, then the fused
// kernel over the tile draws over both; generic: chunks scored into scratch, then sampled)
enum class SweepKind { niw1, nich1, nich1_rows, narrow, rows, rows_sampler, mixed, roles_tail, generic };
struct SweepRoute {
  SweepKind kind = SweepKind::generic;
  int lanes = 0; uint32_t table_rows = 0;   // narrow (narrow_lanes)
  bool transposed = false;                  // nich1: k_sweep_nich1_t
  ScoreShape shape;                         // mixed: PAIR mode of the tile kernels (sweep_pair_mode), rows a wave
  uint64_t tail_ld = 0;                     // roles_tail
  bool tail_pair = false;                   // roles_tail
};
inline SweepRoute route_sweep(const RouteFacts &rf, const Switches &sw, uint64_t nrows) {
  const uint64_t cus = (uint64_t)rf.num_cus;
  const TilePlan &p = rf.plan;
  SweepRoute r;
  if (sweep_is_niw1(rf)) {
    r.kind = SweepKind::niw1;
  } else if (sweep_is_fused(rf)) {
    if (rf.nich1) {
      r.kind = rf.K > 1024 ? SweepKind::nich1_rows : SweepKind::nich1;
      // enough rows for a 32-row chunk per wave over most of the chip: the transposed draw (k_sweep_nich1_t; measured ahead
      // from ~16 k rows on at K = 256 and at K = 1024 alike -- 4 k rows: 15 vs 11 us, 16 k: 15 vs 18, 64 k: 19 vs 30,
      // 512 k: 74 vs 120).  The two kernels draw different bits: by view_rows.
      r.transposed = sw.sweep_nich1 == 2 || (sw.sweep_nich1 != 1 && rf.view_rows >= cus * 64);
    } else if ((r.lanes = narrow_lanes(rf, sw, &r.table_rows)) != 0) {
      r.kind = SweepKind::narrow;
    } else if (narrow_tail_fits(rf) && rf.K <= kTailMaxGroups && sweep_rows_pays(rf, sw, rf.K)) {
      r.kind = rf.K <= 64 ? SweepKind::rows : SweepKind::rows_sampler;
    } else {
      r.kind = SweepKind::mixed;
      r.shape.pair = sweep_pair_mode(rf);
      // Few rows: R = 2 or 4 rows a wave (not 8) spread the chunks over the chip in one round.  k_sweep_tile<R, 16> then
      // takes the place of a plan's own non-PAIR kernel: by view_rows.  R follows the call's rows: the same bits at every R
      // (test_gpu_shard_views.py _kernels).
      const bool small = (nrows + 63) / 64 <= cus, view_small = (rf.view_rows + 63) / 64 <= cus;
      const int R = small ? ((nrows + 31) / 32 > cus ? 4 : 2) : view_small ? 4 : 8;
      if (!rf.has_dm && (view_small || p.tile_path == MSC_PATH_TILE)) r.shape.wave_rows = R;
    }
  } else if (!rf.nich1 && !rf.has_dm && p.tile_path != MSC_PATH_TILE && p.tile_narrow_tail_ok && rf.K > 256 &&
             rf.K <= (uint32_t)kGroupTile + kTailMaxGroups && sweep_rows_pays(rf, sw, rf.K - kGroupTile) && sweep_plain(rf)) {
    r.tail_ld = rf.K <= (uint32_t)kGroupTile + 64 ? 64 : 128;
    // (65 .. 128 groups beyond the tile on a role-split plan: ONE pass of the role-split kernel in PAIR mode at tile 1
    // instead of three launches of the lane <-> row kernel -- round 5)
    r.tail_pair = p.tile_path == MSC_PATH_TILE_ROLES && r.tail_ld == 128;
    if (r.tail_pair || narrow_tail_fits(rf)) r.kind = SweepKind::roles_tail;
  }
  return r;
}

}  // namespace msc
