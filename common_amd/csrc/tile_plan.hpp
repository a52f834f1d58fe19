// tile_plan.hpp -- the tile planner: the steps that turn a state's descriptors into the plans its kernels walk, as pure
// functions over vectors of FeatDesc and plain values.  Host only: no HIP call, no object of the library -- abi.cpp
// plan_groups calls the steps in order and does the device work between them (the view's derived copies, the uploads);
// tests/cxx/test_tile_plan.cpp builds this header with the host compiler and holds each step to its rules.  A pointer in
// a descriptor is a value here: nothing is dereferenced.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "feat_desc.hpp"
#include "route.hpp"

namespace msc {

// The plan of the tile kernels (score_block.hpp).  They walk a reordered copy of the descriptors: first every
// feature except the unmasked nich ones, in the caller's order, then the unmasked nich features, which get a phase
// (and an inner loop) of their own.  (Float addition order follows this plan, not the caller's feature order.)
// Consecutive features are packed into groups whose table blocks fit the LDS slot together: greedy, at most
// kGrpRows rows per group, never across the two phases.

// Phase order and nich blocks: the tile plan `t` of the caller's descriptors `desc` (nu_bits: per feature, the bits of a
// nich feature's nu prior; nich_info: the state's records, one a feature -- device), t[i] being the caller's feature
// t_src[i] and the first `split` entries the first phase.
struct PhaseOrder {
  std::vector<uint32_t> t_src;
  uint32_t split = 0;
  bool nich_blocks_any = false;
};
inline PhaseOrder plan_phases(std::vector<FeatDesc> &desc, const std::vector<uint32_t> &nu_bits, NichPlanInfo *nich_info,
                              std::vector<FeatDesc> &t) {
  auto nich_tail = [](const FeatDesc &d) { return d.family == MSC_NICH && d.mask == nullptr && d.col != nullptr; };
  const uint32_t nfeat = (uint32_t)desc.size();
  PhaseOrder po;
  std::vector<uint32_t> &t_src = po.t_src;                  // t[i] is the caller's feature t_src[i]
  t.clear();
  for (FeatDesc &d : desc) d.blk_first = d.blk_end = 0, d.nich_info = nullptr;
  for (uint32_t i = 0; i < nfeat; i++)
    if (!nich_tail(desc[i])) t.push_back(desc[i]), t_src.push_back(i);
  po.split = (uint32_t)t.size();
  // The second phase, in BLOCKS (family_math.hpp "nich BLOCKS"): the plain nich features ordered by their nu prior
  // (stable: the caller's order among equals), runs of an equal nu cut into blocks of at most kNichBlock, as even as they
  // come (five are 3 + 2, not 4 + 1: a feature on its own pays the full logarithm).  Whether a block's c1 really are equal
  // is for the head kernel to say (the counts are the suff-stats', not the plan's).
  std::vector<uint32_t> tail;
  for (uint32_t i = 0; i < nfeat; i++) if (nich_tail(desc[i])) tail.push_back(i);
  std::stable_sort(tail.begin(), tail.end(), [&](uint32_t a, uint32_t b) { return nu_bits[a] < nu_bits[b]; });
  for (size_t a = 0; a < tail.size();) {
    size_t b = a + 1;
    while (b < tail.size() && nu_bits[tail[b]] == nu_bits[tail[a]]) b++;
    const size_t n = b - a, nb = (n + kNichBlock - 1) / kNichBlock, base = n / nb, rem = n % nb;
    for (size_t blk = 0, at = a; blk < nb; blk++) {
      const size_t len = base + (blk < rem ? 1 : 0);
      for (size_t j = 0; j < len; j++) {
        FeatDesc d = desc[tail[at + j]];
        d.blk_first = (uint32_t)(t.size() - j);
        d.blk_end = d.blk_first + (uint32_t)len;
        d.nich_info = nich_info + tail[at + j];
        t.push_back(d);
        t_src.push_back(tail[at + j]);
      }
      po.nich_blocks_any |= len >= 2;
      at += len;
    }
    a = b;
  }
  if (!po.nich_blocks_any)                                      // (no block of two or more: no records, no head-kernel work, no far rows)
    for (FeatDesc &d : t) d.nich_info = nullptr;
  return po;
}

// masked lookup columns: the tile plan reads the copy with the mask folded in (bind_view) and sees no mask -- a masked
// value selects the table's zero row, which the feature stages with the others (one more row: `extra`, returned)
inline std::vector<uint32_t> plan_sentinels(std::vector<FeatDesc> &t) {
  std::vector<uint32_t> extra(t.size(), 0u);
  for (size_t i = 0; i < t.size(); i++) {
    t[i].fuse_n = 0;
    if (t[i].mask != nullptr && t[i].col_sentinel != nullptr) {
      t[i].col = t[i].col_sentinel;
      t[i].mask = nullptr;
      extra[i] = 1;
    }
  }
  return extra;
}

// what the choice of kernels depends on, for one plan
struct PlanFacts {
  ScorePath path = MSC_PATH_TILE;      // (TilePlan::tile_path)
  bool tail_ok = false, tail_masked_nich = false, tail_dm = false;
  uint32_t tail_max_rows = 0, tail_pack_rows = 0;
};
// the tile plans whose nich waves read the pack and the x matrix (msc::NichPos)
inline bool stages_nich(ScorePath path) { return path == MSC_PATH_TILE_ROLES || path == MSC_PATH_NICH_PACK; }

// group packing, lookup kinds and runs of a plan `t` whose first `split` entries are the first phase (`extra`: one more
// table row for a masked lookup column's zero row)
inline PlanFacts plan_layout(std::vector<FeatDesc> &t, uint32_t split, const std::vector<uint32_t> &extra, const Switches &sw) {
  auto rows_of = [](const FeatDesc &d) -> uint32_t {
    if (d.fuse_n >= 2) {
      uint32_t rows = 1;
      for (uint32_t j = 0; j < d.fuse_n; j++) rows *= d.fuse_radix;
      return rows;
    }
    switch (d.family) {
      case MSC_BB:
      case MSC_BBNC: return 2;
      case MSC_NICH: return 6;
      // (a table up to the whole slot is staged -- on its own group if need be: a dd feature of 100 categories with 64 of
      // them staged was a GENERIC feature to every tile kernel, 1.03 ms for four of them beside two nich columns on a
      // million rows whatever K <= 256 is; staged whole they are lookup runs like any other)
      case MSC_DD: return std::min<uint32_t>(d.dim, (uint32_t)kGrpRows);
      case MSC_GP:
      case MSC_BNB: return std::min<uint32_t>(d.vcap, (uint32_t)kGrpRows);
      // dm: all dim + 1 tables or none (small counts: tens of rows).  Read from L2 they cost 2 KiB per row and
      // stage -- 4 x dm(4) on 1M rows ran at the L2's bandwidth, 1.9 ms
      case MSC_DM: return d.dm_meta != nullptr && d.dm_rows <= (uint32_t)kGrpRows ? d.dm_rows : 0;
      default: return 0;
    }
  };
  const uint32_t n = (uint32_t)t.size();
  uint32_t f = 0;
  while (f < n) {
    const uint32_t limit = f < split ? split : n;
    uint32_t used = 0, g = f;
    while (g < limit && used + rows_of(t[g]) + extra[g] <= (uint32_t)kGrpRows) {
      // (a nich block is staged whole: its members' constants are read side by side)
      if (t[g].blk_end > g + 1 && t[g].blk_first == g && used > 0 && used + 6u * (t[g].blk_end - g) > (uint32_t)kGrpRows) break;
      t[g].grp_off = used;
      t[g].grp_rows = rows_of(t[g]) + extra[g];
      used += t[g].grp_rows;
      g++;
    }
    if (g == f) {                                           // (a block larger than the slot: a group of its own, nothing staged)
      t[g].grp_off = 0;
      t[g].grp_rows = 0;
      g++;
    }
    for (uint32_t i = f; i < g; i++) t[i].grp_end = g;
    f = g;
  }
  // Unmasked lookup features whose whole table is staged (so that no row can miss it) take the tight inner
  // loop of the first phase; run_end lets a wave stay in it for a whole run of them.
  for (uint32_t i = 0; i < n; i++) {
    FeatDesc &d = t[i];
    d.kind = MSC_KIND_GENERIC;
    if (d.mask != nullptr || d.col == nullptr || d.grp_rows == 0) continue;
    // (run_clamp: the largest row a value may select -- with the mask folded in that is the zero row)
    if (d.fuse_n >= 2) d.kind = MSC_KIND_LOOKUP_U8, d.run_clamp = d.grp_rows - 1;
    else if (d.family == MSC_BB || d.family == MSC_BBNC) d.kind = MSC_KIND_LOOKUP_U8, d.run_clamp = 1 + extra[i];
    else if ((d.family == MSC_GP || d.family == MSC_BNB) && d.grp_rows >= d.vcap + extra[i]) d.kind = MSC_KIND_LOOKUP_U32, d.run_clamp = d.grp_rows - 1;
    else if (d.family == MSC_DD && d.grp_rows >= d.dim + extra[i]) d.kind = MSC_KIND_LOOKUP_I32, d.run_clamp = d.dim - 1 + extra[i];
  }
  PlanFacts pf;
  bool has_dm = false;
  bool roles_ok = split > 0 && split < n;
  for (uint32_t i = 0; i < n; i++) {
    has_dm |= t[i].family == MSC_DM;
    if (i < split && t[i].kind == MSC_KIND_GENERIC) roles_ok = false;
  }
  if (has_dm) roles_ok = false;
  // the kernels whose waves are all nich waves (k_score_nich_pack): no first phase at all and two or more plain nich features,
  // or a first phase of at most kPackMaxLookups lookup features beside at least twice as many nich features (the lookups
  // are gathered from L2 there, ~0.03 ms a feature and million rows: 8 bb + 8 nich sweep 0.81 -> 0.70 ms, 2 gp + 12 nich
  // 0.99 -> 0.86; with 16 bb + 4 nich -- four fused lookups, four nich -- the role-split kernels are as good or better)
  const bool nich_only = (split == 0 && n >= 2) || (roles_ok && !has_dm && split <= (uint32_t)kPackMaxLookups && n - split >= 2 * split);
  // staged lookup features and nothing else: k_score_lookups / k_sweep_lookups (sixteen lookup waves of 16 sums)
  bool lookups_only = split == n && n > 0 && !has_dm;
  for (uint32_t i = 0; i < n; i++) lookups_only &= t[i].kind != MSC_KIND_GENERIC;
  // (roles_ok needs split < n and lookups_only split == n; nich_only wins over roles_ok)
  pf.path = nich_only ? MSC_PATH_NICH_PACK : roles_ok ? MSC_PATH_TILE_ROLES : lookups_only ? MSC_PATH_LOOKUPS : MSC_PATH_TILE;
  // the lane <-> row kernel for a partly filled last tile (k_score_tail_rows): lookup features only in the first phase
  // (what it implements), whatever the second holds of plain nich features
  pf.tail_ok = !sw.no_narrow_tail;
  // (a masked nich column among them is evaluated like the second phase's features, under the row's mask; a dm feature
  // whose dim + 1 tables are staged whole -- small counts: no row of the bound column is beyond them -- is dim + 1 lookups
  // of (hi, lo) pairs, round 5; the kernel has one instantiation for either, none for both)
  for (uint32_t i = 0; i < split; i++) {
    const bool masked_nich = t[i].family == MSC_NICH && t[i].mask != nullptr && t[i].col != nullptr;
    const bool staged_dm = t[i].family == MSC_DM && t[i].col != nullptr && t[i].dm_meta != nullptr && t[i].grp_rows != 0;
    pf.tail_ok &= t[i].kind != MSC_KIND_GENERIC || masked_nich || staged_dm;
    pf.tail_masked_nich |= masked_nich;
    pf.tail_dm |= staged_dm;
  }
  if (pf.tail_dm && pf.tail_masked_nich) pf.tail_ok = false;
  for (uint32_t i = split; i < n; i++) pf.tail_ok &= t[i].family == MSC_NICH && t[i].mask == nullptr && t[i].grp_rows == 6;
  if (!pf.tail_ok) pf.tail_masked_nich = pf.tail_dm = false;
  if (pf.tail_ok)
    for (uint32_t i = 0; i < split; i++) {
      const uint32_t rows = t[i].family == MSC_DM ? t[i].dm_rows : t[i].kind == MSC_KIND_GENERIC ? 0u : t[i].run_clamp + 1;
      pf.tail_max_rows = std::max(pf.tail_max_rows, rows);
      pf.tail_pack_rows += rows;
    }
  for (uint32_t i = n; i-- > 0;) {
    FeatDesc &d = t[i];
    if (d.kind == MSC_KIND_GENERIC) d.run_end = i;
    else d.run_end = (i + 1 < d.grp_end && t[i + 1].kind != MSC_KIND_GENERIC) ? t[i + 1].run_end : i + 1;
  }
  return pf;
}

// The leave-one-out pass (k_loo_own_lds) stages what a row gathers per feature -- the lookup families' "value against
// the group minus one" tables, nich's twelve doubles per group -- for ALL kpad groups (a row's own group is any of
// them): consecutive features share the 64 KiB slot while their blocks fit; a feature whose block does not fit, or
// that is not of a staged kind, reads global memory inside its stage.  Returns the number of features staged.
inline uint32_t plan_loo_stages(std::vector<FeatDesc> &t, uint32_t kpad) {
  const uint32_t n = (uint32_t)t.size();
  uint32_t loo_staged = 0;
  for (uint32_t i = 0; i < n; i++) {
    FeatDesc &d = t[i];
    d.loo_off = d.loo_rows = 0;
    uint32_t rows = 0;
    if (d.kind != MSC_KIND_GENERIC && (d.loo_tab != nullptr || d.family == MSC_BBNC)) rows = d.run_clamp + 1;
    else if (d.family == MSC_NICH && d.mask == nullptr && d.col != nullptr && d.loo64 != nullptr) rows = 2 * kNlooStride;
    if (rows != 0 && (uint64_t)rows * kpad <= kLooSlotFloats) d.loo_rows = rows;
  }
  for (uint32_t f0 = 0; f0 < n;) {
    uint32_t used = 0, g = f0;
    while (g < n && g - f0 < (uint32_t)kLooStageFeats && used + t[g].loo_rows * kpad <= kLooSlotFloats) {
      t[g].loo_off = used;
      used += t[g].loo_rows * kpad;
      loo_staged += t[g].loo_rows != 0;
      g++;
    }
    for (uint32_t i = f0; i < g; i++) t[i].loo_stage_end = g;
    f0 = g;
  }
  return loo_staged;
}

// The score / sweep kernels' plan: the unmasked bb / bbnc columns of the first phase come first, fused four (three, two)
// at a time -- one byte column of the members' bits, one table of 2^m rows (FeatDesc::fuse_*; k_fuse_tables fills the
// tables at the head of a call) -- then the other first-phase features in the caller's order, then the second phase.
// A quarter of the LDS reads and additions for the same sum; the order and the association of the terms --
// ((t0 + t1) + t2) + t3 per fused feature -- are the same in every kernel that walks this plan.  The leave-one-out
// pass walks the plan above.
struct Fused { uint32_t first, m, radix; };               // (first: index into members[radix - 2])
struct FusedRuns {
  std::vector<uint32_t> members[2];                        // [0] unmasked, [1] masked: the fusable features, in plan order
  std::vector<Fused> quads;
  // the tile plan's feature that is member j of quad q
  uint32_t member(size_t q, uint32_t j) const { return members[quads[q].radix - 2][quads[q].first + j]; }
};
// (may_fuse: a view is bound and the no-fuse switch is not set -- the view is only looked at while it exists: a plan made
// after its view is gone -- msc_state_set_hp on a dd feature re-plans -- fuses nothing and holds no column; the next call
// that brings a view binds and plans again)
inline FusedRuns plan_fused_runs(const std::vector<FeatDesc> &t, uint32_t split, const std::vector<uint32_t> &extra, bool may_fuse) {
  FusedRuns fr;
  // (columns with a mask: their mask-folded copies, three states a value -- 0, 1, masked = the member's zero row --,
  // three at a time against 27 rows)
  for (uint32_t i = 0; i < split; i++) {
    const FeatDesc &d = t[i];
    if (may_fuse && (d.family == MSC_BB || d.family == MSC_BBNC) && d.kind == MSC_KIND_LOOKUP_U8 && d.mask == nullptr &&
        d.col != nullptr && d.tab != nullptr)
      fr.members[extra[i] ? 1 : 0].push_back(i);
  }
  for (uint32_t cls = 0; cls < 2; cls++) {
    const size_t widest = cls == 0 ? 4 : 3;
    size_t at = 0;
    for (size_t left = fr.members[cls].size(); left >= 2;) {
      const uint32_t m = left == widest + 1 ? (uint32_t)widest - 1 : (uint32_t)std::min(widest, left);    // (never a single one left over)
      fr.quads.push_back(Fused{(uint32_t)at, m, 2u + cls});
      at += m;
      left -= m;
    }
  }
  return fr;
}
// the fused plan `tf` (and its `extra_f`) of the tile plan `t`: the quads first -- quad q reads the byte column packed[q]
// (the view's, abi.cpp packed_column) against rows [q * 32 kpad, ...) of fuse_tab --, then every feature no quad took;
// block bounds of the second phase follow.  Sets fuse_any, fuse_nfeat and fuse_split of `p`.
inline void plan_fused_list(const std::vector<FeatDesc> &t, uint32_t split, const std::vector<uint32_t> &extra, const FusedRuns &fr,
                            const std::vector<const void *> &packed, float *fuse_tab, uint32_t kpad, std::vector<FeatDesc> &tf,
                            std::vector<uint32_t> &extra_f, TilePlan &p) {
  const uint32_t n = (uint32_t)t.size();
  tf.clear();
  extra_f.clear();
  std::vector<bool> taken(n, false);
  for (size_t q = 0; q < fr.quads.size(); q++) {
    const Fused &fq = fr.quads[q];
    FeatDesc d = t[fr.member(q, 0)];
    for (uint32_t j = 0; j < 4; j++) d.fuse_src[j] = nullptr;
    for (uint32_t j = 0; j < fq.m; j++) {
      d.fuse_src[j] = t[fr.member(q, j)].tab;
      taken[fr.member(q, j)] = true;
    }
    d.col = packed[q];
    d.fuse_n = fq.m;
    d.fuse_radix = fq.radix;
    d.col_type = MSC_TYPE_U8;
    d.family = MSC_BB;
    d.tab = fuse_tab + q * 32 * (size_t)kpad;
    d.loo_tab = nullptr;
    tf.push_back(d);
    extra_f.push_back(0u);
  }
  for (uint32_t i = 0; i < n; i++)
    if (!taken[i]) {
      tf.push_back(t[i]);
      extra_f.push_back(extra[i]);
    }
  p.fuse_any = !fr.quads.empty();
  p.fuse_nfeat = (uint32_t)tf.size();
  p.fuse_split = split - (n - p.fuse_nfeat);
  for (uint32_t i = p.fuse_split; i < p.fuse_nfeat; i++) {     // (block bounds are indices into the plan they sit in)
    tf[i].blk_first -= n - p.fuse_nfeat;
    tf[i].blk_end -= n - p.fuse_nfeat;
  }
}

// the accumulate pass's list: a fused feature reads z and its byte column once for all its members (their additive
// tables: fuse_acc); everything else as the caller gave it.  (Histograms of 2 m K counters: while they fit LDS.)
inline void plan_acc_list(const std::vector<FeatDesc> &desc, const std::vector<uint32_t> &t_src, const std::vector<FeatDesc> &tf,
                          const FusedRuns &fr, uint32_t K, std::vector<FeatDesc> &ta) {
  const uint32_t n = (uint32_t)desc.size();
  ta.clear();
  std::vector<bool> covered(n, false);
  for (size_t q = 0; q < fr.quads.size(); q++) {
    const Fused &fq = fr.quads[q];
    if ((size_t)K * 8u * fq.m * 4u > 64u * 1024u) continue;
    FeatDesc d = tf[q];
    for (uint32_t j = 0; j < 4; j++) d.fuse_acc[j] = nullptr;
    for (uint32_t j = 0; j < fq.m; j++) {
      const uint32_t src = t_src[fr.member(q, j)];
      d.fuse_acc[j] = desc[src].acc_i64;
      covered[src] = true;
    }
    ta.push_back(d);
  }
  for (uint32_t i = 0; i < n; i++)
    if (!covered[i]) ta.push_back(desc[i]);
}

// what a plan reads of the bound view's derived copies (the x matrix, the lookup index matrix): none until the steps
// below say so
inline void clear_view_reads(std::vector<FeatDesc> &v) {
  for (FeatDesc &d : v) d.rn_pack = nullptr, d.rn_pos = nullptr, d.rn_x = nullptr, d.rn_n2 = d.rn_n2p = 0;
  for (FeatDesc &d : v) d.lk_idx = nullptr, d.lk_l4 = d.lk_goff = 0;
}
// the kernels that read those copies need the view; without it (a plan made while no view is bound) the plan does not
// take those kernels, and the next call with a view plans again
inline ScorePath path_for_view(ScorePath path, bool view_bound) {
  return !view_bound && (stages_nich(path) || path == MSC_PATH_LOOKUPS) ? MSC_PATH_TILE : path;
}

// what the role-split kernels' nich waves read (msc::NichPos): the positions of the fused plan's second phase
// tf[s0 .. s0 + n2), padded to a multiple of four, and the columns of the x matrix (the pack: k_fuse_tables fills it at
// the head of every call)
inline void plan_nich_pos(const std::vector<FeatDesc> &tf, uint32_t s0, std::vector<NichPos> &pos, std::vector<const void *> &xcols) {
  const uint32_t n2 = (uint32_t)tf.size() - s0, n2p = (n2 + 3u) & ~3u;
  pos.assign(n2p, NichPos());
  xcols.assign(n2, nullptr);
  for (uint32_t i = 0; i < n2p; i++) {
    NichPos &q = pos[i];
    q.xlim = INFINITY, q.blk_ok = 0u;                       // (the head kernel writes these two for real positions)
    if (i < n2) {
      const FeatDesc &d = tf[s0 + i];
      q.blk = (d.blk_first - s0) | (d.blk_end - d.blk_first) << 16, q.seg_end = d.grp_end - s0;
      xcols[i] = d.col;
    } else q.blk = i | 1u << 16, q.seg_end = n2p;
  }
}

// The lookup index matrix of a plan's first phase tf[0 .. split) (msc::FeatDesc::lk_idx): a row's record is the groups'
// features side by side, a byte each, every group from a dword boundary on; sets lk_goff at every group's first feature.
// (C3: 36 features in ten groups, 48 bytes a row.)  false: no matrix for this plan -- a feature that is no staged lookup,
// or a slot row beyond a byte.
struct LookIdxLayout {
  std::vector<LookIdxSrc> src;
  std::vector<uint64_t> key;       // what the view keeps the matrix by
  uint32_t l4 = 0;                 // dwords a row
};
inline bool plan_look_idx(std::vector<FeatDesc> &tf, uint32_t split, LookIdxLayout &lay) {
  lay.src.assign(split, LookIdxSrc());
  lay.key.clear();
  uint32_t l4 = 0;
  for (uint32_t f0 = 0; f0 < split;) {
    const uint32_t f1 = tf[f0].grp_end;
    tf[f0].lk_goff = l4;
    for (uint32_t i = f0; i < f1; i++) {
      const FeatDesc &d = tf[i];
      if (d.kind == MSC_KIND_GENERIC || d.col == nullptr || d.grp_off + d.run_clamp >= 256u) return false;
      lay.src[i] = LookIdxSrc{d.col, d.kind, d.run_clamp, d.grp_off, 4u * l4 + (i - f0)};
      lay.key.push_back(reinterpret_cast<uintptr_t>(d.col));
      lay.key.push_back((uint64_t)d.kind | (uint64_t)d.run_clamp << 8 | (uint64_t)d.grp_off << 32);
      lay.key.push_back(lay.src[i].byte_at);
    }
    l4 += (f1 - f0 + 3u) / 4u;
    f0 = f1;
  }
  lay.l4 = l4;
  return true;
}

// the prices the kernels are chosen by (PlanCost): staged lookup features and table rows of the first
// phase, nich features (the second phase's, and masked ones evaluated in the first)
inline PlanCost plan_prices(const std::vector<FeatDesc> &tf, uint32_t fuse_split, ScorePath path) {
  double lookups = 0, rows = 0, nich = (double)((uint32_t)tf.size() - fuse_split);
  for (uint32_t i = 0; i < fuse_split; i++) {
    if (tf[i].family == MSC_NICH) nich += 1;
    else if (tf[i].family == MSC_DM) lookups += 2.0 * (tf[i].dim + 1), rows += tf[i].grp_rows;   // (dim + 1 stages of (hi, lo) pairs)
    else lookups += 1, rows += tf[i].grp_rows;
  }
  PlanCost pc;
  const double first = 6.0 + 0.45 * lookups + 0.012 * rows;
  pc.tile_round_us = path == MSC_PATH_NICH_PACK ? 6.0 + 1.3 * nich + 3.0 * lookups : path == MSC_PATH_TILE_ROLES ? first + 0.75 * nich
                     : path == MSC_PATH_LOOKUPS ? 0.75 * first : first + 1.5 * nich;
  pc.sweep_round_us = pc.tile_round_us + 2.5;              // (+ the draws)
  pc.tail_fixed_us = 2.0;                                  // (per launch and round of 1024 rows a CU: tools/scans/grid_scan.py at 1M rows,
  pc.tail_group_us = 0.5 + 0.03 * lookups + 0.057 * nich;  //  K = 8 against K = 32 for six feature lists; C3: 2 + 2.5 a group)
  return pc;
}

}  // namespace msc
