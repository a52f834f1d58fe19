// What test_tile_plan.cpp and test_route.cpp share: descriptors with dummy pointers, and the planner's steps run in the
// order abi.cpp plan_groups runs them, with every device step taken as done (a "view" is a flag plus non-null column
// pointers: its copies are dummy pointers too).  Includes tile_plan.hpp, route.hpp and feat_desc.hpp only; no pointer
// made here is ever dereferenced.
#pragma once

#include <cstdio>
#include <cstring>
#include <vector>

#include "tile_plan.hpp"

namespace cases {
using namespace msc;

static int g_failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      cases::g_failures++;                                                  \
    }                                                                       \
  } while (0)

// distinct non-null addresses per feature index and purpose
static char g_mem[8][4096];
template <typename T>
T *dummy(int purpose, uint32_t i) { return reinterpret_cast<T *>(&g_mem[purpose][(i % 512u) * 8u]); }
enum { P_COL, P_MASK, P_SENT, P_TAB, P_ACC, P_LOO, P_META, P_MISC };

inline uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

// a state's feature list as the caller gives it; each adder returns the feature's index
struct Spec {
  std::vector<FeatDesc> desc;
  std::vector<uint32_t> nu;
  uint32_t add(int family, uint32_t dim, bool masked, bool sentinel) {
    const uint32_t i = (uint32_t)desc.size();
    FeatDesc d;
    std::memset(&d, 0, sizeof d);
    d.family = family, d.dim = dim;
    d.col = dummy<void>(P_COL, i);
    d.tab = dummy<float>(P_TAB, i);
    d.acc_i64 = dummy<long long>(P_ACC, i);
    if (masked) d.mask = dummy<uint8_t>(P_MASK, i);
    if (masked && sentinel) d.col_sentinel = dummy<void>(P_SENT, i);
    if (family == MSC_NICH) d.loo64 = dummy<double>(P_LOO, i);
    else if (family != MSC_DM) d.loo_tab = dummy<float>(P_LOO, i);
    desc.push_back(d);
    nu.push_back(0u);
    return i;
  }
  uint32_t bb(bool masked = false, bool sentinel = true) { return add(MSC_BB, 0, masked, sentinel); }
  uint32_t dd(uint32_t dim, bool masked = false) { return add(MSC_DD, dim, masked, masked); }
  uint32_t gp(uint32_t vcap, bool masked = false) {
    const uint32_t i = add(MSC_GP, 0, masked, masked);
    desc[i].vcap = vcap;
    return i;
  }
  uint32_t nich(float nu_prior = 1.0f, bool masked = false) {
    const uint32_t i = add(MSC_NICH, 0, masked, false);
    nu[i] = bits_of(nu_prior);
    return i;
  }
  uint32_t dm(uint32_t dim, uint32_t dm_rows) {
    const uint32_t i = add(MSC_DM, dim, false, false);
    desc[i].dm_rows = dm_rows;
    desc[i].dm_meta = dummy<uint32_t>(P_META, i);
    return i;
  }
  Spec &bbs(uint32_t n, bool masked = false) { for (uint32_t i = 0; i < n; i++) bb(masked); return *this; }
  Spec &nichs(uint32_t n, float nu_prior = 1.0f) { for (uint32_t i = 0; i < n; i++) nich(nu_prior); return *this; }
};

// everything plan_groups leaves behind for one state
struct Planned {
  std::vector<FeatDesc> desc, t, tf, ta;
  std::vector<uint32_t> t_src, extra, extra_f;
  FusedRuns fr;
  PlanFacts layout;                  // of the plan the kernels walk, before the view is looked at
  bool look_idx_ok = false;
  LookIdxLayout lay;
  std::vector<NichPos> pos;
  TilePlan p;
};
inline Planned plan(const Spec &s, uint32_t K, bool view, const Switches &sw = Switches()) {
  Planned r;
  r.desc = s.desc;
  if (!view)                                       // (a state whose view is gone holds no column: abi.cpp bound_view_of)
    for (FeatDesc &d : r.desc) d.col = nullptr, d.mask = nullptr, d.col_sentinel = nullptr;
  const uint32_t kpad = (K + kGroupTile - 1) / kGroupTile * kGroupTile;
  const PhaseOrder po = plan_phases(r.desc, s.nu, dummy<NichPlanInfo>(P_MISC, 0), r.t);
  r.t_src = po.t_src;
  r.p.tile_split = po.split, r.p.nich_blocks_any = po.nich_blocks_any;
  r.extra = plan_sentinels(r.t);
  PlanFacts facts = plan_layout(r.t, po.split, r.extra, sw);
  r.p.loo_staged = plan_loo_stages(r.t, kpad);
  r.fr = plan_fused_runs(r.t, po.split, r.extra, view && !sw.no_bb_fuse);
  std::vector<const void *> packed;
  for (size_t q = 0; q < r.fr.quads.size(); q++) packed.push_back(dummy<void>(P_MISC, 100 + (uint32_t)q));
  plan_fused_list(r.t, po.split, r.extra, r.fr, packed, dummy<float>(P_MISC, 50), kpad, r.tf, r.extra_f, r.p);
  plan_acc_list(r.desc, po.t_src, r.tf, r.fr, K, r.ta);
  if (r.p.fuse_any) facts = plan_layout(r.tf, r.p.fuse_split, r.extra_f, sw);
  r.layout = facts;
  clear_view_reads(r.tf);
  clear_view_reads(r.t);
  facts.path = path_for_view(facts.path, view);
  if (stages_nich(facts.path)) {
    std::vector<const void *> xcols;
    plan_nich_pos(r.tf, r.p.fuse_split, r.pos, xcols);
  }
  if (facts.path == MSC_PATH_TILE_ROLES || facts.path == MSC_PATH_LOOKUPS) {
    r.look_idx_ok = plan_look_idx(r.tf, r.p.fuse_split, r.lay);
    if (!r.look_idx_ok) facts.path = MSC_PATH_TILE;
  }
  r.p.tile_path = facts.path;
  r.p.plan_cost = plan_prices(r.tf, r.p.fuse_split, facts.path);
  r.p.tile_narrow_tail_ok = facts.tail_ok;
  r.p.tail_masked_nich = facts.tail_masked_nich, r.p.tail_dm = facts.tail_dm;
  r.p.tail_max_rows = facts.tail_max_rows, r.p.tail_pack_rows = facts.tail_pack_rows;
  return r;
}

// the route's facts for a planned state on a chip of 256 CUs (the two kernel limits as kernels_sweep.hip has them for
// the shapes used here: a niw feature of dim <= 4, the single-nich rows kernel)
inline RouteFacts facts_of(const Spec &s, const Planned &pl, uint32_t K, uint64_t view_rows) {
  RouteFacts rf;
  rf.K = K, rf.kpad = (K + kGroupTile - 1) / kGroupTile * kGroupTile, rf.num_cus = 256;
  rf.nfeat = (uint32_t)s.desc.size();
  rf.nich1 = rf.nfeat == 1 && s.desc[0].family == MSC_NICH;
  for (const FeatDesc &d : s.desc) {
    rf.has_dm |= d.family == MSC_DM, rf.n_niw += d.family == MSC_NIW;
    rf.feats.push_back(RouteFeat{d.family, d.dim, d.vcap, false});
  }
  rf.plan = pl.p;
  rf.view_rows = view_rows;
  rf.niw1_max_groups = 256;
  rf.nich1_rows_max_groups = 32768;
  return rf;
}

}  // namespace cases
