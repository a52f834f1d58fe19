// Host test of common_amd/csrc/tile_plan.hpp alone (with feat_desc.hpp and route.hpp, which it includes): the tile
// planner's steps against the rules written beside them and in DESIGN.md section 4.  No device: a pointer here is a dummy
// value, a "view" a flag.  Every expectation is worked out from the rule, none from a run of the planner.
#include "plan_cases.hpp"

#include <set>

using namespace cases;

// the invariants every plan keeps, checked on every plan this program makes
static void check_invariants(const std::vector<FeatDesc> &t, uint32_t split, uint32_t kpad) {
  const uint32_t n = (uint32_t)t.size();
  for (uint32_t f0 = 0; f0 < n;) {                      // LDS groups: at most kGrpRows rows, never across the phases
    const uint32_t f1 = t[f0].grp_end;
    CHECK(f1 > f0 && f1 <= n);
    if (f1 <= f0) return;
    uint32_t rows = 0;
    for (uint32_t i = f0; i < f1; i++) {
      CHECK(t[i].grp_end == f1);
      CHECK(t[i].grp_off == rows);
      rows += t[i].grp_rows;
    }
    CHECK(rows <= (uint32_t)kGrpRows);
    CHECK(f0 >= split || f1 <= split);
    f0 = f1;
  }
  for (uint32_t i = 0; i < n; i++) {
    if (t[i].blk_end > t[i].blk_first) {                // a nich block: whole inside one group, within the second phase
      CHECK(t[i].blk_first >= split && t[i].blk_end <= n && i >= t[i].blk_first && i < t[i].blk_end);
      CHECK(t[i].blk_end - t[i].blk_first <= (uint32_t)kNichBlock);
      CHECK(t[t[i].blk_first].grp_end == t[i].grp_end);
    }
    if (t[i].kind == MSC_KIND_GENERIC) CHECK(t[i].run_end == i);   // runs: lookup features only, inside one group
    else CHECK(t[i].run_end > i && t[i].run_end <= t[i].grp_end);
  }
  for (uint32_t f0 = 0; f0 < n;) {                      // leave-one-out stages
    const uint32_t f1 = t[f0].loo_stage_end;
    CHECK(f1 > f0 && f1 <= n && f1 - f0 <= (uint32_t)kLooStageFeats);
    if (f1 <= f0) return;
    uint64_t floats = 0;
    for (uint32_t i = f0; i < f1; i++) {
      CHECK(t[i].loo_off == floats);
      floats += (uint64_t)t[i].loo_rows * kpad;
    }
    CHECK(floats <= kLooSlotFloats);
    f0 = f1;
  }
}
static Planned planned(const Spec &s, uint32_t K, bool view, const Switches &sw = Switches()) {
  Planned r = plan(s, K, view, sw);
  const uint32_t kpad = (K + kGroupTile - 1) / kGroupTile * kGroupTile;
  check_invariants(r.t, r.p.tile_split, kpad);
  // (the fused plan keeps the tile plan's leave-one-out fields: only its groups and runs are its own)
  std::vector<FeatDesc> tf = r.tf;
  plan_loo_stages(tf, kpad);
  check_invariants(tf, r.p.fuse_split, kpad);
  CHECK(r.p.fuse_nfeat == r.tf.size() && r.p.fuse_any == !r.fr.quads.empty());
  return r;
}
static std::vector<uint32_t> block_lengths(const Planned &r) {
  std::vector<uint32_t> out;
  for (uint32_t i = r.p.tile_split; i < r.t.size(); i = r.t[i].blk_end) {
    CHECK(r.t[i].blk_first == i);
    out.push_back(r.t[i].blk_end - i);
  }
  return out;
}
static std::vector<uint32_t> quad_sizes(const Planned &r, uint32_t radix) {
  std::vector<uint32_t> out;
  for (const Fused &q : r.fr.quads)
    if (q.radix == radix) out.push_back(q.m);
  return out;
}
using U = std::vector<uint32_t>;

static void test_nich_blocks() {
  CHECK(block_lengths(planned(Spec().nichs(5), 256, true)) == (U{3, 2}));
  CHECK(block_lengths(planned(Spec().nichs(9), 256, true)) == (U{3, 3, 3}));
  CHECK(block_lengths(planned(Spec().nichs(4), 256, true)) == (U{4}));
  CHECK(planned(Spec().nichs(5), 256, true).p.nich_blocks_any);
  {                                                     // one nich feature: a block of one, no records
    const Planned r = planned(Spec().bbs(2).nichs(1), 256, true);
    CHECK(block_lengths(r) == (U{1}) && !r.p.nich_blocks_any && r.t[2].nich_info == nullptr);
  }
  {                                                     // nu 1, 2, 1, 2, 1: the sort is stable, no block across a nu boundary
    Spec s;
    for (int i = 0; i < 5; i++) s.nich(i % 2 ? 2.0f : 1.0f);
    const Planned r = planned(s, 256, true);
    CHECK(r.t_src == (U{0, 2, 4, 1, 3}));
    CHECK(block_lengths(r) == (U{3, 2}));
    CHECK(r.t[0].nich_info == dummy<NichPlanInfo>(P_MISC, 0) + 0 && r.t[3].nich_info == dummy<NichPlanInfo>(P_MISC, 0) + 1);
  }
  {                                                     // a masked nich feature stays in the first phase
    Spec s;
    s.nich(1.0f, true), s.nich(), s.nich();
    const Planned r = planned(s, 256, true);
    CHECK(r.p.tile_split == 1 && r.t_src == (U{0, 1, 2}) && r.t[0].mask != nullptr && r.t[0].kind == MSC_KIND_GENERIC);
    CHECK(block_lengths(r) == (U{2}));
  }
}

static void test_group_packing() {
  {                                                     // 22 nich of one nu: blocks 4 4 4 4 3 3; the last block's first member
    const Planned r = planned(Spec().nichs(22), 256, true);   // would fit the first group (19 x 6 + 6 rows), the block would not
    CHECK(block_lengths(r) == (U{4, 4, 4, 4, 3, 3}));
    CHECK(r.t[18].grp_end == 19 && r.t[19].grp_off == 0 && r.t[19].grp_end == 22);
  }
  {                                                     // two dd(100): 200 rows, two groups, each a lookup run of its own
    Spec s;
    s.dd(100), s.dd(100);
    const Planned r = planned(s, 256, true);
    CHECK(r.t[0].grp_end == 1 && r.t[1].grp_end == 2 && r.t[0].grp_rows == 100 && r.t[1].grp_rows == 100);
    CHECK(r.t[0].kind == MSC_KIND_LOOKUP_I32 && r.t[0].run_clamp == 99 && r.t[0].run_end == 1 && r.t[1].run_end == 2);
  }
  {                                                     // dd(200): 128 rows staged, not the whole table: generic
    Spec s;
    s.dd(200);
    const Planned r = planned(s, 256, true);
    CHECK(r.t[0].kind == MSC_KIND_GENERIC && r.t[0].grp_rows == 128);
  }
  {                                                     // gp by the rows of its exact table
    Spec s;
    s.gp(1024), s.gp(100);
    const Planned r = planned(s, 256, true);
    CHECK(r.t[0].kind == MSC_KIND_GENERIC && r.t[0].grp_rows == 128);
    CHECK(r.t[1].kind == MSC_KIND_LOOKUP_U32 && r.t[1].grp_rows == 100 && r.t[1].run_clamp == 99);
  }
  {                                                     // dm: all its tables or none
    Spec s;
    s.dm(4, 40), s.dm(4, 200);
    const Planned r = planned(s, 256, true);
    CHECK(r.t[0].grp_rows == 40 && r.t[1].grp_rows == 0);
    CHECK(r.t[0].kind == MSC_KIND_GENERIC && r.t[1].kind == MSC_KIND_GENERIC);
  }
}

static void test_lookup_runs() {
  {                                                     // bb bb | dd(200) | bb bb: 132 rows do not share a group
    Spec s;
    s.bb(), s.bb(), s.dd(200), s.bb(), s.bb();
    const Planned r = planned(s, 256, false);
    (void)r;
    const Planned v = planned(s, 256, true, [] { Switches sw; sw.no_bb_fuse = true; return sw; }());
    CHECK(v.t[0].grp_end == 2 && v.t[2].grp_end == 3 && v.t[3].grp_end == 5);
    CHECK(v.t[0].run_end == 2 && v.t[1].run_end == 2 && v.t[2].run_end == 2 && v.t[3].run_end == 5 && v.t[4].run_end == 5);
  }
  {                                                     // a generic feature inside the group ends the run
    Spec s;
    s.bb(), s.nich(1.0f, true), s.bb();
    const Planned r = planned(s, 256, true);
    CHECK(r.t[0].grp_end == 3 && r.t[0].run_end == 1 && r.t[1].run_end == 1 && r.t[2].run_end == 3);
  }
}

static void test_sentinel() {
  Spec s;
  s.bb(true), s.dd(10, true), s.bb();
  const Planned r = planned(s, 256, true, [] { Switches sw; sw.no_bb_fuse = true; return sw; }());
  CHECK(r.t[0].col == s.desc[0].col_sentinel && r.t[0].mask == nullptr && r.extra[0] == 1);
  CHECK(r.t[0].kind == MSC_KIND_LOOKUP_U8 && r.t[0].grp_rows == 3 && r.t[0].run_clamp == 2);     // rows 0, 1 and the zero row
  CHECK(r.t[1].col == s.desc[1].col_sentinel && r.t[1].mask == nullptr && r.extra[1] == 1);
  CHECK(r.t[1].kind == MSC_KIND_LOOKUP_I32 && r.t[1].grp_rows == 11 && r.t[1].run_clamp == 10);
  CHECK(r.t[2].col == s.desc[2].col && r.extra[2] == 0 && r.t[2].grp_rows == 2 && r.t[2].run_clamp == 1);
  CHECK(r.desc[0].mask != nullptr);                    // (the caller's descriptors keep the mask: the accumulate pass reads it)
}

static void test_fusing() {
  CHECK(quad_sizes(planned(Spec().bbs(16), 256, true), 2) == (U{4, 4, 4, 4}));
  CHECK(quad_sizes(planned(Spec().bbs(5), 256, true), 2) == (U{3, 2}));
  CHECK(quad_sizes(planned(Spec().bbs(6), 256, true), 2) == (U{4, 2}));
  CHECK(quad_sizes(planned(Spec().bbs(9), 256, true), 2) == (U{4, 3, 2}));
  CHECK(planned(Spec().bbs(1), 256, true).fr.quads.empty());
  CHECK(quad_sizes(planned(Spec().bbs(4, true), 256, true), 3) == (U{2, 2}));
  CHECK(quad_sizes(planned(Spec().bbs(7, true), 256, true), 3) == (U{3, 2, 2}));
  CHECK(quad_sizes(planned(Spec().bbs(7, true), 256, true), 2).empty());
  CHECK(planned(Spec().bbs(16), 256, false).fr.quads.empty());
  Switches no_fuse;
  no_fuse.no_bb_fuse = true;
  CHECK(planned(Spec().bbs(16), 256, true, no_fuse).fr.quads.empty());
  {                                                     // a quad's table rows, clamp and sources
    const Planned r = planned(Spec().bbs(5), 256, true);
    CHECK(r.tf.size() == 2 && r.tf[0].fuse_n == 3 && r.tf[0].fuse_radix == 2 && r.tf[0].grp_rows == 8 && r.tf[0].run_clamp == 7);
    CHECK(r.tf[1].fuse_n == 2 && r.tf[1].grp_rows == 4 && r.tf[1].grp_off == 8 && r.tf[1].kind == MSC_KIND_LOOKUP_U8);
    CHECK(r.tf[0].fuse_src[0] == r.desc[0].tab && r.tf[0].fuse_src[2] == r.desc[2].tab && r.tf[0].fuse_src[3] == nullptr);
    CHECK(r.tf[1].fuse_src[0] == r.desc[3].tab && r.tf[0].col != r.desc[0].col && r.tf[0].col_type == MSC_TYPE_U8);
    const Planned m = planned(Spec().bbs(3, true), 256, true);      // masked: three digits of three states, 27 rows
    CHECK(m.tf.size() == 1 && m.tf[0].fuse_radix == 3 && m.tf[0].grp_rows == 27 && m.tf[0].run_clamp == 26);
  }
  {                                                     // 8 bb + 5 nich: six features fused away, the blocks move down by six
    const Planned r = planned(Spec().bbs(8).nichs(5), 256, true);
    CHECK(r.p.tile_split == 8 && r.t[8].blk_first == 8 && r.t[8].blk_end == 11 && r.t[11].blk_first == 11 && r.t[11].blk_end == 13);
    CHECK(r.p.fuse_nfeat == 7 && r.p.fuse_split == 2);
    CHECK(r.tf[2].blk_first == 2 && r.tf[2].blk_end == 5 && r.tf[5].blk_first == 5 && r.tf[6].blk_end == 7);
  }
}

static void test_acc_list() {
  {
    const Planned r = planned(Spec().bbs(4), 512, true);     // 512 groups x 8 counters x 4 bytes x 4 members = 64 KiB: fits
    CHECK(r.ta.size() == 1 && r.ta[0].fuse_n == 4);
    for (uint32_t j = 0; j < 4; j++) CHECK(r.ta[0].fuse_acc[j] == r.desc[j].acc_i64);
    const Planned w = planned(Spec().bbs(4), 513, true);     // one group more: singly, as the caller gave them
    CHECK(w.ta.size() == 4 && w.fr.quads.size() == 1);
    for (uint32_t j = 0; j < 4; j++) CHECK(w.ta[j].fuse_n == 0 && w.ta[j].acc_i64 == w.desc[j].acc_i64 && w.ta[j].col == w.desc[j].col);
  }
  for (uint32_t K : {100u, 512u, 700u, 1500u}) {             // every feature exactly once (3 members fit up to 682 groups, 2 up to 1024)
    Spec s;
    s.bbs(9).nichs(2), s.dd(12), s.bb(true), s.bb(true);
    const Planned r = planned(s, K, true);
    std::multiset<const void *> seen;
    for (const FeatDesc &d : r.ta)
      if (d.fuse_n >= 2) for (uint32_t j = 0; j < d.fuse_n; j++) seen.insert(d.fuse_acc[j]);
      else seen.insert(d.acc_i64);
    CHECK(seen.size() == s.desc.size());
    for (const FeatDesc &d : s.desc) CHECK(seen.count(d.acc_i64) == 1);
  }
}

static void test_paths() {
  CHECK(planned(Spec().bbs(8).nichs(8), 256, true).p.tile_path == MSC_PATH_NICH_PACK);     // two fused lookups, eight nich
  CHECK(planned(Spec().bbs(16).nichs(4), 256, true).p.tile_path == MSC_PATH_TILE_ROLES);   // four and four
  CHECK(planned(Spec().bbs(32), 256, true).p.tile_path == MSC_PATH_LOOKUPS);
  CHECK(planned(Spec().nichs(2), 256, true).p.tile_path == MSC_PATH_NICH_PACK);
  CHECK(planned(Spec().nichs(7), 256, true).p.tile_path == MSC_PATH_NICH_PACK);
  CHECK(planned(Spec().nichs(1), 256, true).p.tile_path == MSC_PATH_TILE);
  {
    Spec s;
    s.bbs(4).nichs(2), s.dm(4, 40);
    CHECK(planned(s, 256, true).p.tile_path == MSC_PATH_TILE);
    Spec g;
    g.bbs(4).nichs(8), g.dd(200);
    CHECK(planned(g, 256, true).p.tile_path == MSC_PATH_TILE);
    Spec m;
    m.bbs(4).nichs(8), m.nich(1.0f, true);
    CHECK(planned(m, 256, true).p.tile_path == MSC_PATH_TILE);
  }
  for (ScorePath path : {MSC_PATH_TILE_ROLES, MSC_PATH_NICH_PACK, MSC_PATH_LOOKUPS, MSC_PATH_TILE}) {
    CHECK(path_for_view(path, false) == MSC_PATH_TILE);
    CHECK(path_for_view(path, true) == path);
  }
  CHECK(planned(Spec().bbs(8).nichs(8), 256, false).p.tile_path == MSC_PATH_TILE);
  CHECK(planned(Spec().bbs(16).nichs(4), 256, false).p.tile_path == MSC_PATH_TILE);
  CHECK(planned(Spec().bbs(32), 256, false).p.tile_path == MSC_PATH_TILE);
  CHECK(planned(Spec().nichs(2), 256, false).p.tile_path == MSC_PATH_TILE);
  {                                                     // the lane <-> row kernel's share of the plan
    const Planned r = planned(Spec().bbs(16).nichs(4), 256, true);
    CHECK(r.p.tile_narrow_tail_ok && r.p.tail_max_rows == 16 && r.p.tail_pack_rows == 64 && !r.p.tail_masked_nich && !r.p.tail_dm);
    Switches sw;
    sw.no_narrow_tail = true;
    CHECK(!planned(Spec().bbs(16).nichs(4), 256, true, sw).p.tile_narrow_tail_ok);
    Spec g;
    g.bbs(4), g.dd(200);
    CHECK(!planned(g, 256, true).p.tile_narrow_tail_ok);
  }
}

static void test_loo_stages() {
  {
    const Planned r = planned(Spec().bbs(16).nichs(4), 256, true);
    CHECK(r.p.loo_staged == 20);
    for (uint32_t i = 0; i < 16; i++) CHECK(r.t[i].loo_rows == 2);
    for (uint32_t i = 16; i < 20; i++) CHECK(r.t[i].loo_rows == 2 * kNlooStride);
    CHECK(r.t[0].loo_stage_end == 6 && r.t[6].loo_stage_end == 12 && r.t[18].loo_stage_end == 20);
  }
  {                                                     // 8192 groups: twelve rows of a nich feature are 96 Ki floats, two of a bb 16 Ki
    const Planned r = planned(Spec().bbs(3).nichs(4), 8192, true);
    for (uint32_t i = 0; i < 3; i++) CHECK(r.t[i].loo_rows == 2);
    for (uint32_t i = 3; i < 7; i++) CHECK(r.t[i].loo_rows == 0);
    CHECK(r.p.loo_staged == 3);
    CHECK(r.t[0].loo_stage_end == 2);                   // (two bb blocks fill the slot)
  }
}

static void test_look_idx() {
  {                                                     // C3's counts: 36 first-phase features in ten groups, two of them of six
    Spec s;
    s.bbs(16);                                          // four quads, 64 rows
    s.dd(32), s.dd(32);                                 // ... and 64: group one, six features
    for (int i = 0; i < 6; i++) s.dd(21);               // 126 rows: group two, six features
    for (int i = 0; i < 24; i++) s.dd(40);              // three to a group (120 rows): eight groups
    s.nichs(16);
    const Planned r = planned(s, 256, true);
    CHECK(r.p.fuse_split == 36 && r.p.tile_path == MSC_PATH_TILE_ROLES && r.look_idx_ok);
    uint32_t groups = 0;
    for (uint32_t f0 = 0; f0 < 36; f0 = r.tf[f0].grp_end) groups++;
    CHECK(groups == 10);
    CHECK(r.lay.l4 == 12);                              // 2 + 2 + 8 dwords: 48 bytes a row
    std::set<uint32_t> bytes;
    for (uint32_t f0 = 0; f0 < 36; f0 = r.tf[f0].grp_end) {
      CHECK(r.lay.src[f0].byte_at == 4u * r.tf[f0].lk_goff);
      for (uint32_t i = f0; i < r.tf[f0].grp_end; i++) {
        CHECK(r.lay.src[i].byte_at == r.lay.src[f0].byte_at + (i - f0) && r.lay.src[i].byte_at < 4u * r.lay.l4);
        CHECK(r.lay.src[i].col == r.tf[i].col && r.lay.src[i].clamp == r.tf[i].run_clamp && r.lay.src[i].grp_off == r.tf[i].grp_off);
        bytes.insert(r.lay.src[i].byte_at);
      }
    }
    CHECK(bytes.size() == 36);
    CHECK(r.lay.key.size() == 3 * 36);
  }
  {                                                     // a slot row must fit a byte
    std::vector<FeatDesc> tf(1);
    std::memset(&tf[0], 0, sizeof(FeatDesc));
    tf[0].col = dummy<void>(P_COL, 0), tf[0].kind = MSC_KIND_LOOKUP_U8, tf[0].grp_end = 1, tf[0].grp_off = 200;
    LookIdxLayout lay;
    tf[0].run_clamp = 55;
    CHECK(plan_look_idx(tf, 1, lay) && lay.l4 == 1);
    tf[0].run_clamp = 56;
    CHECK(!plan_look_idx(tf, 1, lay));
    tf[0].run_clamp = 1, tf[0].kind = MSC_KIND_GENERIC;
    CHECK(!plan_look_idx(tf, 1, lay));
  }
}

static void test_nich_pos() {
  const Planned r = planned(Spec().bbs(16).nichs(5), 256, true);     // blocks 3 + 2 at positions 0 and 3, padded to eight
  CHECK(r.pos.size() == 8);
  CHECK(r.pos[0].blk == (0u | 3u << 16) && r.pos[2].blk == (0u | 3u << 16) && r.pos[3].blk == (3u | 2u << 16));
  CHECK(r.pos[0].seg_end == 5 && r.pos[4].seg_end == 5);
  CHECK(r.pos[5].blk == (5u | 1u << 16) && r.pos[7].blk == (7u | 1u << 16) && r.pos[7].seg_end == 8);
  for (const NichPos &q : r.pos) CHECK(q.blk_ok == 0u && q.xlim > 3.0e38f);
}

int main() {
  test_nich_blocks();
  test_group_packing();
  test_lookup_runs();
  test_sentinel();
  test_fusing();
  test_acc_list();
  test_paths();
  test_loo_stages();
  test_look_idx();
  test_nich_pos();
  if (g_failures) return 1;
  std::printf("tile_plan ok\n");
  return 0;
}
