// blocked.cpp -- the blocked Gibbs sampler and the split-merge move built on it (kernels_blocked.hip,
// kernels_splitmerge.hip): msc_blocked_*, msc_sweep_blocked, msc_split_merge and msc_split_merge_tables.  Host logic only;
// the core it stands on is abi.cpp, through abi_internal.hpp.
#include <algorithm>
#include <string>

#include "abi_internal.hpp"
#include "blocked_niw.hpp"
#include "blocked_post.hpp"
#include "launchers.hpp"
#include "splitmerge_math.hpp"

using namespace msc;

// ---------------------------------------------------------------------------
// The blocked (uncollapsed) Gibbs sampler (kernels_blocked.hip, blocked_post.hpp): draw every slot's parameters and the
// stick weights from the tables, then every row's slot independently under them.
// ---------------------------------------------------------------------------
// (Which assign kernel a state takes, and whether the sampler takes it at all: route_calls.hpp route_sweep_blocked.)

// a feature's slices in a state's parameter table (UINT32_MAX: row 0, the log weights), as msc_blocked_tables and
// msc_split_merge_tables hand them out
static void blocked_table_slices(const msc_state *st, uint32_t feature, const float **dev, uint32_t *nslices, uint32_t *ld) {
  const bool w = feature == UINT32_MAX;
  if (dev) *dev = st->blk.tab + (w ? 0 : (size_t)st->blk.feats_host[feature].slice0 * st->kpad);
  if (nslices) *nslices = w ? 1u : st->blk.feats_host[feature].nslices;
  if (ld) *ld = st->kpad;
}

// the parameter table and the features as the kernels read them (columns from the current binding, if any)
static int blocked_setup(msc_state *st) {
  if (!st->blk.tab) {
    uint32_t rows = 1;
    for (const auto &h : st->feats) rows += blocked_slices(h.family, h.dim);
    MSC_TRY(alloc_zeroed(st->blk.tab, (size_t)rows * st->kpad));
    MSC_TRY(alloc_zeroed(st->blk.work, 2 * (size_t)st->K));
    MSC_TRY(alloc_zeroed(st->blk.feats_dev, std::max<size_t>(1, st->nfeat)));
    st->blk.rows = rows;
  }
  // a state of one niw feature (BlockedKernel::niw1): the drawn matrices in double, zero until the first draw
  if (st->nfeat == 1 && st->feats[0].family == MSC_NIW && !st->blk.niw_mean) {
    const uint32_t d = st->feats[0].dim;
    MSC_TRY(alloc_zeroed(st->blk.niw_mean, (size_t)st->K * d));
    MSC_TRY(alloc_zeroed(st->blk.niw_whiten, (size_t)st->K * blocked::ntri(d)));
    MSC_TRY(alloc_zeroed(st->blk.niw_w64, (size_t)st->K * niw_w_stream(d)));
    MSC_TRY(alloc_zeroed(st->blk.niw_mu64, (size_t)st->K * niw_b_stream(d)));
  }
  std::vector<BlkFeat> fs(st->nfeat);
  uint32_t row = 1;
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const msc_feature_host &h = st->feats[f];
    const FeatDesc &d = st->desc_host[f];
    BlkFeat &b = fs[f];
    std::memset(&b, 0, sizeof(b));
    switch (h.family) {
      case MSC_BB: b.kind = MSC_BLK_SELECT; break;
      case MSC_GP:
      case MSC_BNB: b.kind = MSC_BLK_LINEAR; break;
      case MSC_DD: b.kind = MSC_BLK_GATHER; break;
      case MSC_NICH: b.kind = MSC_BLK_NICH; break;
      default: b.kind = MSC_BLK_NOOP; break;
    }
    b.slice0 = row;
    b.nslices = blocked_slices(h.family, h.dim);
    row += b.nslices;
    b.family = h.family;
    b.dim = h.dim;
    b.tag = f;
    b.col = d.col;
    b.mask = d.mask;
    b.hp = h.hp_dev;
    b.raw_u32 = h.raw_u32;
    b.raw_f32 = h.raw_f32;
  }
  if (fs.size() != st->blk.feats_host.size() ||
      (!fs.empty() && std::memcmp(fs.data(), st->blk.feats_host.data(), fs.size() * sizeof(BlkFeat)) != 0)) {
    if (!fs.empty()) {
      MSC_HIP(hipMemcpyAsync(st->blk.feats_dev, fs.data(), fs.size() * sizeof(BlkFeat), hipMemcpyHostToDevice, st->ctx->stream));
      MSC_HIP(hipStreamSynchronize(st->ctx->stream));
    }
    st->blk.feats_host = std::move(fs);
  }
  return MSC_OK;
}

static int blocked_draw_impl(msc_state *st, const BlockedRoute &route, uint64_t seed, uint64_t sweep) {
  // the draw reads the reference's fields and the group counts: both current before (the additive sums and the score
  // constants it does not read are left as they are)
  MSC_TRY(ensure_raw(st));
  MSC_TRY(blocked_setup(st));
  if (route.kernel == BlockedKernel::niw1) {
    if (launch_blocked_draw_niw(st->ctx->stream, st->blk.feats_dev, st->K, st->kpad, st->cnt_u32, st->alpha, seed, sweep,
                                st->blk.work, st->blk.tab, st->blk.niw_mean, st->blk.niw_whiten, st->blk.niw_w64,
                                st->blk.niw_mu64))
      return MSC_EHIP;
  } else if (launch_blocked_draw(st->ctx->stream, st->blk.feats_dev, st->nfeat, st->K, st->kpad, st->cnt_u32, st->alpha, seed,
                                 sweep, st->blk.work, st->blk.tab))
    return MSC_EHIP;
  st->valid.drawn();
  return MSC_OK;
}

static int blocked_assign_impl(msc_state *st, const BlockedRoute &route, const msc_dataview *view, const uint32_t *cols,
                               uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep) {
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  MSC_REQUIRE(st->valid.draw_current(), "msc_blocked_assign: no parameter draw made from the tables as they stand (msc_blocked_draw "
                                        "first; whatever changes tables, hyper-parameters, alpha or group counts makes a draw stale)");
  MSC_TRY(blocked_setup(st));
  if (route.kernel == BlockedKernel::niw1) {
    if (launch_blocked_assign_niw(st->ctx->stream, st->feats[0].dim, st->blk.feats_dev, st->blk.tab, st->blk.niw_w64,
                                  st->blk.niw_mu64, st->K, st->kpad, row0, nrows, row_id0, z_dev, seed, sweep))
      return MSC_EHIP;
  } else if (launch_blocked_assign(st->ctx->stream, route.kernel, route.block, st->blk.feats_dev, (int)st->nfeat, st->blk.tab,
                                   st->K, st->kpad, row0, nrows, row_id0, z_dev, seed, sweep))
    return MSC_EHIP;
  return MSC_OK;
}

extern "C" int msc_blocked_draw(msc_state *st, uint64_t seed, uint64_t sweep) {
  MSC_REQUIRE(st, "null state");
  MSC_TRY(refuse_mid_step(st, "msc_blocked_draw"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  const BlockedRoute route = route_sweep_blocked(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  return blocked_draw_impl(st, route, seed, sweep);
}

extern "C" int msc_blocked_tables(msc_state *st, uint32_t feature, const float **dev, uint32_t *nslices, uint32_t *ld) {
  MSC_REQUIRE(st, "null state");
  MSC_REQUIRE(feature == UINT32_MAX || feature < st->nfeat, "feature %u out of range", feature);
  MSC_HIP(hipSetDevice(st->ctx->device));
  const BlockedRoute route = route_sweep_blocked(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  MSC_TRY(blocked_setup(st));
  blocked_table_slices(st, feature, dev, nslices, ld);
  return MSC_OK;
}

extern "C" int msc_blocked_niw_params(msc_state *st, uint32_t feature, const double **mean, const double **whiten,
                                      uint32_t *dim) {
  MSC_REQUIRE(st, "null state");
  MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
  MSC_HIP(hipSetDevice(st->ctx->device));
  const BlockedRoute route = route_sweep_blocked(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  MSC_REQUIRE(route.kernel == BlockedKernel::niw1, "msc_blocked_niw_params: feature %u is not a niw feature", feature);
  MSC_TRY(blocked_setup(st));
  if (mean) *mean = st->blk.niw_mean;
  if (whiten) *whiten = st->blk.niw_whiten;
  if (dim) *dim = st->feats[feature].dim;
  return MSC_OK;
}

extern "C" int msc_blocked_assign(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                                  uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep) {
  MSC_REQUIRE(st && view && (z_dev || nrows == 0), "null argument");
  MSC_TRY(refuse_mid_step(st, "msc_blocked_assign"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  const BlockedRoute route = route_sweep_blocked(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  return blocked_assign_impl(st, route, view, cols, row0, nrows, row_id0, z_dev, seed, sweep);
}

extern "C" int msc_sweep_blocked(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                                 uint64_t row_id0, int32_t *z_dev, uint32_t nsweeps, uint64_t seed, uint64_t sweep,
                                 int32_t *trace_dev, uint32_t *top_slot_dev) {
  MSC_REQUIRE(st && view && (z_dev || nrows == 0), "null argument");
  MSC_TRY(refuse_mid_step(st, "msc_sweep_blocked"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  const BlockedRoute route = route_sweep_blocked(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  hipStream_t s = st->ctx->stream;
  for (uint32_t i = 0; i < nsweeps; i++) {
    MSC_TRY(blocked_draw_impl(st, route, seed, sweep + i));
    MSC_TRY(blocked_assign_impl(st, route, view, cols, row0, nrows, row_id0, z_dev, seed, sweep + i));
    MSC_TRY(accumulate_impl(st, view, cols, row0, nrows, z_dev, MSC_ACC_RESET));
    if (trace_dev && nrows)
      MSC_HIP(hipMemcpyAsync(trace_dev + (size_t)i * nrows, z_dev, nrows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (top_slot_dev && launch_blocked_top_slot(s, st->cnt_u32, st->K, top_slot_dev + i)) return MSC_EHIP;
  }
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// The split-merge move (kernels_splitmerge.hip, splitmerge_math.hpp): Metropolis-Hastings proposals that split one group
// in two or merge two groups, the launch state reached by restricted BLOCKED Gibbs passes over the rows of the two groups.
// ---------------------------------------------------------------------------
// (Which assign kernel a state takes, and whether the move takes it at all: route_calls.hpp route_splitmerge.)
// The pair state (three slots: the pair's two, and their union for score_data), created at the first call; its
// hyper-parameters and alpha follow the state's before every call
constexpr uint32_t kSmSlots = 3;
static int sm_setup(msc_state *st) {
  if (!st->sm.pair) {
    std::vector<msc_feature_spec> specs(st->nfeat);
    for (uint32_t f = 0; f < st->nfeat; f++) {
      specs[f].family = st->feats[f].family;
      specs[f].dim = st->feats[f].dim;
    }
    MSC_TRY(alloc_zeroed(st->sm.prop, 1));
    MSC_TRY(alloc_zeroed(st->sm.sd, (size_t)st->nfeat * kSmSlots));
    MSC_TRY(msc_state_create(st->ctx, specs.data(), st->nfeat, kSmSlots, &st->sm.pair));
  }
  msc_state *pair = st->sm.pair;
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (pair->feats[f].hp != st->feats[f].hp)
      MSC_TRY(msc_state_set_hp(pair, f, st->feats[f].hp.data(), st->feats[f].hp.size()));
  pair->alpha = st->alpha;
  return MSC_OK;
}

extern "C" int msc_split_merge(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                               uint64_t row_id0, int32_t *z_dev, uint32_t nproposals, uint32_t launch_iters, uint64_t seed,
                               uint64_t sweep, double *log_dev, int32_t *trace_dev, int32_t *proposed_dev,
                               uint64_t *counters_dev) {
  MSC_REQUIRE(st && view && z_dev, "null argument");
  MSC_TRY(refuse_mid_step(st, "msc_split_merge"));
  MSC_REQUIRE(launch_iters <= 1024, "launch_iters %u beyond 1024", launch_iters);
  MSC_REQUIRE(nrows < (1ull << 48), "msc_split_merge takes fewer than 2^48 rows");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  const BlockedRoute route = route_splitmerge(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  MSC_TRY(ensure_raw(st));                                 // (the group sizes: where a split finds its empty slot)
  MSC_TRY(sm_setup(st));
  msc_state *pair = st->sm.pair;
  hipStream_t s = st->ctx->stream;
  const uint32_t nparts = sm_assign_blocks(nrows, route.block);
  MSC_HIP(reserve_synced(s, st->sm.ell, (size_t)std::max<uint64_t>(nrows, 1)));
  MSC_HIP(reserve_synced(s, st->sm.part, nparts));
  ZeroSpans zero;
  zero.a = reinterpret_cast<unsigned long long *>(pair->red_i64.get());
  zero.na = pair->n_i64;
  zero.b = reinterpret_cast<unsigned long long *>(pair->red_f64.get());
  zero.nb = pair->n_f64;
  // the proposals move the group sizes on the device (k_sm_relabel); everything else is rebuilt at the end
  st->valid.counts_changed();
  for (uint32_t p = 0; p < nproposals; p++) {
    const uint64_t sw = sweep + p;
    if (launch_sm_begin(s, z_dev, nrows, row_id0, st->cnt_u32, st->K, seed, sw, st->sm.prop, st->sm.ell, zero)) return MSC_EHIP;
    for (uint32_t t = 0; t <= launch_iters; t++) {
      // the pair slots' suff-stats from the labels, their parameters and the K = 2 stick, then the rows' labels
      MSC_TRY(accumulate_impl(pair, view, cols, row0, nrows, st->sm.ell, MSC_ACC_RESET | kAccZeroed));
      MSC_TRY(blocked_setup(pair));
      if (launch_blocked_draw(s, pair->blk.feats_dev, pair->nfeat, 2, pair->kpad, pair->cnt_u32, st->alpha,
                              sm::stream_key(seed, sm::kStreamPass0 + t) ^ blocked::kKey, sw, pair->blk.work, pair->blk.tab))
        return MSC_EHIP;
      if (launch_sm_assign(s, route.kernel, route.block, t == launch_iters, t, pair->blk.feats_dev, (int)pair->nfeat,
                           pair->blk.tab, pair->kpad, row0, nrows, row_id0, z_dev, st->sm.ell, st->sm.prop, seed, sw,
                           st->sm.part, zero))
        return MSC_EHIP;
    }
    if (proposed_dev && nrows)
      MSC_HIP(hipMemcpyAsync(proposed_dev + (size_t)p * nrows, st->sm.ell, nrows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // score_data of the two blocks and of their union (slot 2 = the sum of the additive tables of slots 0 and 1)
    MSC_TRY(accumulate_impl(pair, view, cols, row0, nrows, st->sm.ell, MSC_ACC_RESET | kAccZeroed | MSC_ACC_NO_COMMIT));
    if (launch_sm_merge_slots(s, pair->red_i64, (uint32_t)(pair->n_i64 / pair->kpad), pair->red_f64,
                              (uint32_t)(pair->n_f64 / pair->kpad), pair->kpad))
      return MSC_EHIP;
    MSC_TRY(commit(pair));
    if (launch_score_data(s, pair->desc_dev, (int)pair->nfeat, kSmSlots, pair->kpad, st->sm.sd))
      return fail(MSC_EHIP, "k_score_data launch failed");
    if (launch_sm_decide(s, st->sm.prop, st->sm.part, nparts, st->sm.sd, st->nfeat, pair->cnt_u32, st->alpha, seed, sw,
                         log_dev ? log_dev + (size_t)p * 8 : nullptr, reinterpret_cast<unsigned long long *>(counters_dev)))
      return MSC_EHIP;
    if (launch_sm_relabel(s, nrows, z_dev, st->sm.ell, st->sm.prop, pair->cnt_u32, st->cnt_u32)) return MSC_EHIP;
    if (trace_dev && nrows)
      MSC_HIP(hipMemcpyAsync(trace_dev + (size_t)p * nrows, z_dev, nrows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  }
  return accumulate_impl(st, view, cols, row0, nrows, z_dev, MSC_ACC_RESET);
}

// What msc_chains_split_merge (chains.cpp) takes from here for one member: whether the move takes the state at all, and
// the member's pair state -- created at the first call, its hyper-parameters and alpha following the member's, bound to the
// view, its parameter-table features as the kernels read them -- as the pair half of the chain's table entry.
namespace msc {
int sm_chain_route(msc_state *st) {
  const BlockedRoute route = route_splitmerge(route_facts_now(st));
  return route.rc != MSC_OK ? fail(route.rc, "%s", route.why.c_str()) : MSC_OK;
}
int sm_chain_pair(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t nrows, SmChain *entry) {
  MSC_TRY(sm_setup(st));
  msc_state *pair = st->sm.pair;
  MSC_TRY(bind_view(pair, view, cols, 0, nrows));
  MSC_TRY(blocked_setup(pair));
  entry->pair_feats = pair->desc_dev;
  entry->pair_blk = pair->blk.feats_dev;
  entry->pair_tab = pair->blk.tab;
  entry->pair_cnt_acc = pair->red_i64;
  entry->pair_cnt_u32 = pair->cnt_u32;
  return MSC_OK;
}
}  // namespace msc

extern "C" int msc_split_merge_tables(msc_state *st, uint32_t feature, const float **dev, uint32_t *nslices, uint32_t *ld) {
  MSC_REQUIRE(st, "null state");
  MSC_REQUIRE(feature == UINT32_MAX || feature < st->nfeat, "feature %u out of range", feature);
  MSC_HIP(hipSetDevice(st->ctx->device));
  const BlockedRoute route = route_splitmerge(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why.c_str());
  MSC_TRY(sm_setup(st));
  msc_state *pair = st->sm.pair;
  MSC_TRY(blocked_setup(pair));
  blocked_table_slices(pair, feature, dev, nslices, ld);
  return MSC_OK;
}
