// feat_desc.hpp -- the plain-old-data descriptors shared with the gfx950 kernels, the results of the tile planner and the
// constants the planner (tile_plan.hpp) and the routes (route.hpp) go by.  Host only: no HIP header, nothing else of the
// library -- tests/cxx/test_tile_plan.cpp and test_route.cpp build it with the host compiler (msc_internal.hpp includes
// it for everything else).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/microscopes_hip.h"

// (a function the kernels call too: the attributes where the compiler knows them, nothing in a host-only build)
#ifdef __HIPCC__
#define MSC_HOST_DEVICE __host__ __device__
#else
#define MSC_HOST_DEVICE
#endif

namespace msc {

constexpr int kGroupTile = 256;    // groups per k-tile: lane <-> 4 consecutive groups
constexpr int kGrpRows = 128;   // table rows the LDS slot of the tile kernels holds (128 KiB): one feature group
constexpr unsigned kGpMaxTable = 1024;   // gp counts below this are exact table entries

// ---- device-visible feature descriptor -------------------------------------
// One per state feature; lives in a small device array rebuilt when the (view,
// cols) binding changes.  All tables are struct-of-arrays with row stride kpad
// (ngroups rounded up to kGroupTile) so that lane l of a wave reads groups
// 4l..4l+3 of a k-tile with one 16-byte load.
//
// Derived score tables (float, filled by the prepare kernels from the raw tables):
//   bb / bbnc rows {s0, s1}                  log p(v=0), log p(v=1)
//   gp   rows {nse_hi, nse_lo, T[0..vcap)}   -stirlerr(a) as hi/lo, then the exact table log p(v) (family_math.hpp)
//   dd   rows {T[0..dim)}                    log p(v = i)
//   nich rows {mu_hi, mu_lo, c0, c1ln2, c1, c2}
//   niw  rows {c0, c1, A_loo, B_loo, C_loo, logdet_hi, logdet_lo} + the matrices below (kernels_niw.hip)
// Raw tables (the reference's own fields, u32 / f32):
//   bb   u32 {heads, tails}          bbnc: + f32 {p}
//   gp   u32 {count, sum}            f32 {log_prod}
//   dd   u32 {count_sum, counts[dim]}
//   nich u32 {count}                 f32 {mean, count_times_variance}
//   niw  u32 {count}                 f32 group-major {sum_x[d]} then {sum_xxT[d*d]} (see niw_* offsets)
//   bnb  u32 {count, sum}
//   dm   u32 {counts[dim]}           f32 {ratio}
// Additive tables (the all-reduce payload):
//   bb   i64 {heads, tails}
//   gp   i64 {count, sum}            f64 {log_prod}
//   dd   i64 {counts[dim]}
//   nich i64 {count}                 f64 {sum_x, sum_xx}
//   niw  i64 {count}                 f64 group-major {sum_x[d]}, {sum_xxT[d*d]}
//   bnb  i64 {count, sum}
//   dm   i64 {counts[dim]}           f64 {ratio}
// nich blocks (family_math.hpp): up to kNichBlock plain nich features of the plan's second phase that share c1
#ifndef MSC_NICH_BLOCK
#define MSC_NICH_BLOCK 4
#endif
constexpr int kNichBlock = MSC_NICH_BLOCK;
constexpr float kNichFarA = 32768.0f;                    // |a| beyond this: the row is "far" (see NichPlanInfo::xlim)
struct NichPlanInfo {                                    // per feature of the plan's second phase (FeatDesc::nich_info)
  float xlim;                                            // |x| <= xlim: no group's |a| = |s x - s mu| exceeds kNichFarA
  uint32_t blk_ok;                                       // at a block's FIRST feature: c1 ln2 is bit-equal over the block
};

// The role-split kernels' nich waves (score_block.hpp nich_phase_packed) read the second phase from three arrays made
// for them -- the plan's own descriptors are 300 bytes a feature and every number in them is a scalar load that waits for
// the one before (round 4: the nich waves issued 0.53 of their time, the rest were such chains):
//   * NichPos[n2p]: per POSITION i of the second phase (plan index - split; padded to a multiple of four) its block
//     (first position, length), the end of its LDS segment (the order of the sums follows the segments in every kernel),
//     and what the head kernel found (xlim, blk_ok: NichPlanInfo's two, copied here);
//   * the pack: (1 + kNichPackRows n2) rows of kpad floats -- row 0 the features' summed c0 (summed in plan order from 0,
//     as nich_c0_sum does), then per position mu_hi, mu_lo, c2, c1 ln2, c1 -- written by the head kernel at the head of
//     every scoring / sweep call from the tables as they stand: ONE buffer, scalar offsets;
//   * the x matrix: float [view rows][n2p], position-major inside a row -- a row's values of the second phase in one
//     64-byte stretch (abi.cpp nich_x_matrix: built when the view is bound, cached on the view).
// what a round of the tile kernels / a launch of the lane <-> row kernel costs for a plan, in microseconds (route.hpp
// tile_rounds_us / tail_rows_us; tile_plan.hpp plan_prices computes it): only to choose between the kernels
struct PlanCost {
  double tile_round_us = 50.0, sweep_round_us = 55.0;    // (C3's, until a plan says otherwise)
  double tail_fixed_us = 30.0, tail_group_us = 1.7;
};
// which scoring kernel a state takes (route.hpp decides from its feature list; a state's tile plan is one of TILE,
// TILE_ROLES, NICH_PACK and LOOKUPS, TilePlan::tile_path)
// (TILE_ROLES: a tile state whose first phase is lookup runs only and whose second phase is not empty -- with enough
// rows its workgroups split the phases between their waves, k_score_tile_roles)
enum ScorePath { MSC_PATH_NICH1 = 0, MSC_PATH_TILE = 1, MSC_PATH_TILE_DM = 2, MSC_PATH_TILE_ROLES = 3, MSC_PATH_NICH_PACK = 4, MSC_PATH_LOOKUPS = 5 };
struct NichPos {                                         // (32-bit fields: a scalar load fetches no less)
  float xlim;
  uint32_t blk_ok;
  uint32_t blk;                                          // the position's block: first position | length << 16
  uint32_t seg_end;
};
constexpr uint32_t kNichPackRows = 5;                    // mu_hi, mu_lo, c2, c1 ln2, c1
struct FeatDesc {
  // -- what the tile kernels' lookup runs read per feature: one 32-byte block, one scalar load (score_block.hpp) --
  const void *col;         // bound dataview column (device), null until bound
  uint32_t grp_off;        // tile kernels, group plan (tile_plan.hpp plan_layout): first row of this feature's table block
                           // inside the LDS slot
  uint32_t run_clamp;      // lookup kinds: the largest table row a value may select (dd: dim - 1, gp / bnb: staged rows - 1)
  uint32_t kind;           // MSC_KIND_*: which inner loop of the tile kernel scores this feature
  uint32_t run_end;        // lookup kinds: one past the last feature of the run of lookup features this one
                           // belongs to (within its group); generic: its own index
  uint32_t grp_rows;       // rows of the block staged in LDS (entries beyond are read from global)
  uint32_t grp_end;        // one past the last feature of this feature's group
  // ----------------------------------------------------------------------------------------------------------------
  int32_t family;
  uint32_t dim;
  int32_t col_type;        // msc_primitive_type of the bound column (value type of the family)
  uint32_t pad0;
  const uint8_t *mask;     // optional per-element mask column
  const float *hp;         // device copy of the hp block
  float *tab;              // derived score table rows
  uint32_t *raw_u32;
  float *raw_f32;
  long long *acc_i64;
  double *acc_f64;
  float *niw_w;            // niw, dim <= 32 only (the f32 MFMA kernel): [K][32][32] whitening matrix (row-major), scaled
  float *niw_b;            // niw, dim <= 32 only: [K][2][32] posterior mean, hi | lo floats
  double *niw_w64;         // niw: W_k = L^-1 sqrt(kn/(kn+1)) as the operand stream of the f64 MFMA kernel,
                           //      [K][niw_w_stream(dim)] (niw_w_index; kernels_niw.hip)
  double *niw_mu64;        // niw: W_k mu_k in the accumulator layout of that kernel, [K][niw_b_stream(dim)] (niw_b_index)
  double *niw_c64;         // niw only: [K][8] {c0, c1, A_loo, B_loo, C_loo}
  double aux;              // dd: sum of the alphas
  uint32_t vcap;           // gp, bnb: rows of the exact table (min(column max + 1, kGpMaxTable))
  uint32_t dm_rows;        // dm: rows of all its (hi, lo) count tables together (host: bind_dm_column), 0 otherwise
  const uint32_t *dm_meta;    // dm: [dim+1][2] per stage (device): {first table row, entries in the table};
                              //     count v of a stage occupies table rows first + 2v (hi) and first + 2v + 1 (lo)
  const uint32_t *dm_tot;     // dm: row totals of the bound column (device, owned by the view)
  // (the group plan's fields are the struct's head; 32-bit on purpose: the kernels read them with scalar loads, a
  // 16-bit field costs a vector load and a full wait)
  double *loo64;              // nich: per-group constants of the leave-one-out pass, [kpad][kNlooStride] (family_math.hpp)
  float *loo_tab;             // bb, gp, bnb, dd: score of value v against the group with one such value removed,
                              // [v][kpad] (k_prepare); the leave-one-out pass is a lookup for these families
  // the leave-one-out pass's own stage plan (tile_plan.hpp plan_loo_stages; k_loo_own_lds): consecutive features of the
  // tile plan whose leave-one-out blocks share the kernel's LDS slot
  uint32_t loo_off;           // first float of this feature's block inside the slot
  uint32_t loo_rows;          // rows of kpad floats staged (lookup kinds: run_clamp + 1 table rows; nich: 12 = 6 doubles
                              // per group, group-major); 0 = not staged: the feature reads global memory
  uint32_t loo_stage_end;     // one past the last feature of this feature's stage
  uint32_t pad1;
  // a masked lookup column (bb, bbnc, gp, bnb, dd) as the tile kernels want it: a copy in which a masked row holds the
  // index of the family's ZERO table row (bb 2, dd dim, gp / bnb vcap) -- abi.cpp bind_view makes it, plan_sentinels
  // (tile_plan.hpp) puts it in the tile plan's copy of the descriptor (mask = null there), so a masked value is one more
  // table row to the lookup loops and nothing else; null when the column has no mask or the family no such row
  const void *col_sentinel;
  // FUSED bb / bbnc columns in the score / sweep kernels' plan (tile_plan.hpp plan_fused_runs): two to four bool columns
  // read as one byte column of their digits (digit j = member j's value -- a bit, or 0 / 1 / 2 = masked for columns with a
  // mask; the view keeps it, k_pack_bits) against one table of radix^n rows -- row i = the members' rows digit_j(i) summed
  // in member order -- that k_fuse_tables rebuilds into
  // `tab` at the head of every scoring / sweep call from the members' own tables (fuse_src): to every kernel it is a lookup
  // feature like any other, with a quarter of the reads and additions.  fuse_n = 0: an ordinary feature.
  const float *fuse_src[4];
  uint32_t fuse_n;
  uint32_t fuse_radix;     // 2: unmasked members; 3: masked ones (digit 2 = the member's zero row; three at a time, 27 rows)
  // nich BLOCKS of the plan's second phase (tile_plan.hpp plan_phases; family_math.hpp): the plan's features
  // [blk_first, blk_end) are one block -- consecutive plain nich features with the same nu prior, at most kNichBlock, never
  // across an LDS feature group -- scored as ONE log1p of their product where the head kernel found their c1 ln2 rows
  // bit-equal (nich_info[0].blk_ok of the block's first feature), feature by feature otherwise.  nich_info: this
  // feature's own record (device; k_fuse_tables fills it at the head of every scoring / sweep call); null outside the
  // second phase.
  uint32_t blk_first, blk_end;
  NichPlanInfo *nich_info;
  // at the FIRST feature of the score / sweep plan's second phase, when the plan may take the role-split kernels: the
  // arrays of NichPos above (null otherwise); rn_n2 positions, rn_n2p = rn_n2 rounded up to four
  float *rn_pack;
  NichPos *rn_pos;
  const float *rn_x;
  uint32_t rn_n2, rn_n2p;
  // the accumulate pass's copy of a fused bb feature (tile_plan.hpp plan_acc_list, desc_acc): the members' additive tables,
  // in the members' order -- one read of the byte column and of z feeds all of them (k_accumulate)
  long long *fuse_acc[4];
  // the first phase's LOOKUP INDEX MATRIX (round 5; tile_plan.hpp plan_look_idx, abi.cpp look_idx_matrix, k_pack_look_idx):
  // for the kernels whose first
  // phase is staged lookup runs only (role-split, lookups-only; PAIR mode too) every row's lookups as ready-made SLOT ROWS --
  // grp_off + the value clamped into the feature's block, one byte a feature, the features of an LDS feature group side by
  // side from a dword boundary on -- so a lookup wave fetches a group's indices for its rows with ONE load per group and
  // lane instead of a descriptor head, a value load, a clamp and a broadcast per feature.  Kept by the view (key: columns,
  // kinds, clamps and slot offsets).  lk_idx / lk_l4 at the plan's FIRST feature (null: the plan does not take those
  // kernels), lk_goff at every group's first feature.
  const uint32_t *lk_idx;  // uint32 [view rows][lk_l4] (+ 3 dwords of slack)
  uint32_t lk_l4;          // dwords per row
  uint32_t lk_goff;        // the group's first dword inside a row's record
};
// (the layout is the kernels': the head is the one 32-byte block a lookup run reads with one scalar load)
static_assert(sizeof(FeatDesc) == 352, "FeatDesc: the kernels' layout");
static_assert(offsetof(FeatDesc, col) == 0 && offsetof(FeatDesc, grp_off) == 8 && offsetof(FeatDesc, run_clamp) == 12 &&
                  offsetof(FeatDesc, kind) == 16 && offsetof(FeatDesc, run_end) == 20 && offsetof(FeatDesc, grp_rows) == 24 &&
                  offsetof(FeatDesc, grp_end) == 28 && offsetof(FeatDesc, family) == 32,
              "FeatDesc: the lookup runs' 32-byte head");

// one feature of the index matrix as k_pack_look_idx reads it
struct LookIdxSrc {
  const void *col;
  uint32_t kind, clamp, grp_off, byte_at;   // byte_at: the feature's byte inside a row's record
};
constexpr uint32_t kLooSlotFloats = 32768;   // 128 KiB: one workgroup of k_loo_own_lds (1024 threads) per CU
constexpr int kLooStageFeats = 6;            // features a stage holds at most (their row values travel in registers)
enum { MSC_KIND_GENERIC = 0, MSC_KIND_LOOKUP_U8 = 1, MSC_KIND_LOOKUP_U32 = 2, MSC_KIND_LOOKUP_I32 = 3 };

// families whose score is a lookup of the row's count in an exact per-group table
MSC_HOST_DEVICE inline bool is_count_family(int family) { return family == MSC_GP || family == MSC_BNB; }

// rows of a feature's block in a tile of k_chains_marginal (0: nothing to stage)
MSC_HOST_DEVICE inline uint32_t cm_table_rows(int family, uint32_t dim, uint32_t vcap) {
  switch (family) {
    case MSC_BB: return 2u;
    case MSC_DD: return dim;
    case MSC_GP:
    case MSC_BNB: return vcap;
    case MSC_NICH: return 6u;                              // (NICH_ROWS)
    default: return 0u;
  }
}

// (nich: kNlooStride doubles per group, group-major -- a row's leave-one-out pass reads ONE group's six constants: side
// by side they are 48 bytes, one cache line mostly; family_math.hpp NLOO_*)
constexpr uint32_t kNlooStride = 6;

constexpr uint32_t kTailMaxGroups = 128;
constexpr uint64_t kNarrowMaxRows = 65536;   // views from this many rows on do not take the K <= 64 narrow tiling (route.hpp narrow_lanes:
                                             // at 100k rows its sweeps already cost 2.5x the lane <-> row kernel's, at 20k they are level)
constexpr uint64_t kTailMinRows = 16384;     // fewer rows always stay with the tile kernels (lanes as groups)
constexpr uint32_t kTailStride = 65;         // floats per table row k_score_tail_rows stages (64 groups + 1)
constexpr int kPackMaxLookups = 4;                      // lookup features (after fusing the bool columns) a plan may hold and still take the nich-only kernels
constexpr double kPairTileShare = 0.62;     // what a pass of the role-split kernels costs in PAIR mode (<= 128 groups), of a full tile pass

// How a pass runs (route.hpp route_score): rows a wave of k_score_tile<R, 16> takes, PAIR mode, what scores a partly filled
// last tile (the tile kernels, k_score_tail_rows, k_score_tile_roles in PAIR mode), k_score_nich1's code (nich1_shape_for)
enum class LastTile { tiles, rows, pair };
struct ScoreShape { int wave_rows = 8; bool pair = false; LastTile last = LastTile::tiles; int nich1 = 0; };

// What the tile planner found for a state (msc_state::plan; tile_plan.hpp writes it whole, from the steps of
// tile_plan.hpp): what the launches and the routes (route.hpp) read of a plan beside its descriptors.
struct TilePlan {
  uint32_t tile_split = 0;            // the tile plan's first phase: every feature but the unmasked nich ones
  uint32_t fuse_nfeat = 0, fuse_split = 0;   // the score / sweep kernels' plan (bool columns fused): its features, its first phase
  bool fuse_any = false;
  bool nich_blocks_any = false;       // the plan has a nich block of two or more features
  // which tile kernels the plan takes -- TILE_ROLES: lookup runs only before tile_split, unmasked nich
  // features after it; NICH_PACK: no first phase at all (or a few lookups), two or more plain nich features
  // (k_score_nich_pack); LOOKUPS: staged lookup features and nothing else (k_score_lookups); else TILE
  ScorePath tile_path = MSC_PATH_TILE;
  PlanCost plan_cost;                 // what a round of the tile kernels / a launch of the lane <-> row kernel costs for THIS plan
  bool tile_narrow_tail_ok = false;   // a partly filled last tile may take k_score_tail_rows
  uint32_t tail_max_rows = 0, tail_pack_rows = 0;   // the lookup tables of the tile plan's first phase: the largest, all together
  bool tail_masked_nich = false;      // ... and masked nich columns among them (evaluated in place, under the row's mask)
  bool tail_dm = false;               // ... or dm features with their tables staged whole
  uint32_t loo_staged = 0;            // features whose leave-one-out block k_loo_own_lds stages in LDS
};

}  // namespace msc
