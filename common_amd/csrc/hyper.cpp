// hyper.cpp -- hyper-parameter inference on the device: grids (kernels_hp.hip: msc_hp_grid_*) and slice sampling
// (kernels_slice.hip: msc_hp_slice, msc_theta_slice), and the log joint their targets add up to (kernels_joint.hip:
// msc_score_joint).  Host logic only; the core it stands on is abi.cpp, through
// abi_internal.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <new>

#include "abi_internal.hpp"
#include "launchers.hpp"

using namespace msc;

// ---------------------------------------------------------------------------
// grid hyper-parameter inference (kernels_hp.hip)
// ---------------------------------------------------------------------------
// group blocks of a score launch: enough workgroups for a few per CU, at least one LDS stage of slots per block
static uint32_t hp_group_blocks(const msc_state *st, size_t point_blocks) {
  const uint32_t stages = (st->K + 63) / 64;
  const size_t want = (4 * (size_t)st->ctx->num_cus + point_blocks - 1) / point_blocks;
  return (uint32_t)std::max<size_t>(1, std::min<size_t>(stages, want));
}

extern "C" int msc_hp_grid_create(msc_state *st, uint32_t feature, const float *host_blocks, size_t block_floats,
                                  uint32_t npoints, const double *host_logprior, msc_hp_grid **out) {
  MSC_REQUIRE(st && host_blocks && out, "null argument");
  *out = nullptr;
  MSC_REQUIRE(npoints > 0, "a grid needs at least one point");
  HpJob job;
  std::memset(&job, 0, sizeof job);
  if (feature == MSC_HP_CLUSTER) {
    MSC_REQUIRE(block_floats == 1, "the alpha grid has blocks of one float, not %zu", block_floats);
    for (uint32_t g = 0; g < npoints; g++)
      MSC_REQUIRE(host_blocks[g] > 0.f, "alpha grid point %u is %g: alpha must be positive (group_manager.hpp:78)", g,
                  (double)host_blocks[g]);
    job.family = kHpCluster;
  } else {
    MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
    const msc_feature_host &h = st->feats[feature];
    if (h.family == MSC_NIW)
      return fail(MSC_EUNSUPPORTED, "feature %u: niw has no hyper-parameter grid (upstream defines none, and every point "
                  "would need its own factorisation of Psi)", feature);
    MSC_REQUIRE(block_floats == h.hp.size(), "feature %u: hp block has %zu floats, expected %zu", feature, block_floats,
                h.hp.size());
    job.family = h.family;
    job.dim = h.dim;
    job.nu32 = raw_u32_rows(h.family, h.dim);
    job.nf32 = raw_f32_rows(h.family);
    job.raw_u32 = h.raw_u32;
    job.raw_f32 = h.raw_f32;
  }
  job.hpf = (uint32_t)block_floats;
  job.npoints = npoints;
  MSC_HIP(hipSetDevice(st->ctx->device));
  std::unique_ptr<msc_hp_grid> g(new (std::nothrow) msc_hp_grid());
  if (!g) return fail(MSC_ENOMEM, "out of host memory");
  g->st = st;
  g->feature = feature;
  g->blocks.assign(host_blocks, host_blocks + (size_t)npoints * block_floats);
  const hipStream_t s = st->ctx->stream;
  MSC_HIP(g->grid_dev.alloc(g->blocks.size()));
  MSC_HIP(hipMemcpyAsync(g->grid_dev, g->blocks.data(), g->blocks.size() * sizeof(float), hipMemcpyHostToDevice, s));
  if (host_logprior) {
    MSC_HIP(g->logprior_dev.alloc(npoints));
    MSC_HIP(hipMemcpyAsync(g->logprior_dev, host_logprior, (size_t)npoints * sizeof(double), hipMemcpyHostToDevice, s));
  }
  job.grid = g->grid_dev;
  job.logprior = g->logprior_dev;
  g->job = job;
  MSC_HIP(g->job_dev.alloc(1));
  MSC_HIP(hipMemcpyAsync(g->job_dev, &g->job, sizeof(HpJob), hipMemcpyHostToDevice, s));
  MSC_HIP(hipStreamSynchronize(s));
  *out = g.get();
  st->hp.grids.push_back(std::move(g));
  return MSC_OK;
}

extern "C" int msc_hp_grid_destroy(msc_hp_grid *grid) {
  if (!grid) return MSC_OK;
  msc_state *st = grid->st;
  (void)hipSetDevice(st->ctx->device);
  (void)hipStreamSynchronize(st->ctx->stream);
  st->hp.grids.erase(std::remove_if(st->hp.grids.begin(), st->hp.grids.end(),
                                    [grid](const std::unique_ptr<msc_hp_grid> &g) { return g.get() == grid; }),
                     st->hp.grids.end());   // (the state owns its grids: this deletes it)
  return MSC_OK;
}

extern "C" int msc_hp_grid_score(msc_hp_grid *grid, const uint8_t *slots_dev, double *out_dev) {
  MSC_REQUIRE(grid && out_dev, "null argument");
  msc_state *st = grid->st;
  MSC_TRY(refuse_mid_step(st, "msc_hp_grid_score"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  const uint32_t np = grid->job.npoints;
  if (grid->job.family == kHpCluster) {
    if (launch_crp_grid_score(st->ctx->stream, grid->job_dev, np, st->cnt_u32, st->K, out_dev))
      return fail(MSC_EHIP, "k_crp_grid_score launch failed");
    return MSC_OK;
  }
  const uint32_t nblk = hp_group_blocks(st, (np + 255) / 256);
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.part, (size_t)nblk * np));
  if (launch_hp_grid_score(st->ctx->stream, grid->job_dev, 1, np, st->K, st->kpad, st->cnt_u32, slots_dev, nblk,
                           st->hp.part, out_dev))
    return fail(MSC_EHIP, "k_hp_grid_score launch failed");
  return MSC_OK;
}

// A kernel has written a feature's hp block (and, dd / dm, its alpha sum into the state's descriptor) on the device; the
// host's bookkeeping follows as msc_state_set_hp keeps it: the host copy, the score tables' staleness and the alpha sum
// in every host copy of the descriptor.  (msc_hp_grid_gibbs, msc_hp_slice and msc_chains_hp_slice.)
void msc::hp_installed(msc_state *st, uint32_t feature, const float *blk) {
  msc_feature_host &h = st->feats[feature];
  std::copy(blk, blk + h.hp.size(), h.hp.begin());
  st->valid.hp_changed(feature);
  (void)refresh_alpha_sum(st, feature);
}
// the same for alpha, which the device takes from the host at the next call that reads it (msc_state_set_alpha)
void msc::alpha_installed(msc_state *st, float alpha) {
  st->alpha = alpha;
  st->valid.alpha_changed();
}

extern "C" int msc_hp_grid_gibbs(msc_state *st, msc_hp_grid *const *grids, uint32_t n, const uint8_t *slots_dev,
                                 uint64_t seed, uint64_t sweep, uint32_t *chosen_host, double *const *scores_dev) {
  MSC_REQUIRE(st && grids && chosen_host, "null argument");
  MSC_REQUIRE(n > 0, "no grids");
  MSC_TRY(refuse_mid_step(st, "msc_hp_grid_gibbs"));
  // the feature grids first (one score launch), the alpha grid last; order[j] = the caller's index of job j
  std::vector<uint32_t> order;
  std::vector<bool> seen(st->nfeat + 1, false);
  for (int pass = 0; pass < 2; pass++)
    for (uint32_t i = 0; i < n; i++) {
      MSC_REQUIRE(grids[i] && grids[i]->st == st, "grid %u is null or belongs to another state", i);
      const bool cluster = grids[i]->feature == MSC_HP_CLUSTER;
      if (cluster != (pass == 1)) continue;
      const uint32_t slot = cluster ? st->nfeat : grids[i]->feature;
      MSC_REQUIRE(!seen[slot], "two grids of %s %u in one step", cluster ? "alpha" : "feature", grids[i]->feature);
      seen[slot] = true;
      order.push_back(i);
    }
  const uint32_t nfj = (uint32_t)(order.size() - (seen[st->nfeat] ? 1 : 0));
  size_t max_np = 0, pblocks = 0;
  for (uint32_t j = 0; j < nfj; j++) {
    const uint32_t np = grids[order[j]]->job.npoints;
    max_np = std::max<size_t>(max_np, np);
    pblocks += (np + 255) / 256;
  }
  const uint32_t nblk = nfj ? hp_group_blocks(st, pblocks) : 1;
  std::vector<HpJob> &jobs = st->hp.jobs_host;
  jobs.assign(n, HpJob());
  size_t part = 0, out = 0;
  for (uint32_t j = 0; j < n; j++) {
    const msc_hp_grid *g = grids[order[j]];
    HpJob &J = jobs[j];
    J = g->job;
    J.part_off = part;
    J.out_off = out;
    part += (size_t)nblk * J.npoints;
    out += J.npoints;
    J.scores_out = scores_dev ? scores_dev[order[j]] : nullptr;
    if (g->feature == MSC_HP_CLUSTER) {
      J.stream = UINT64_MAX - st->nfeat;
    } else {
      const msc_feature_host &h = st->feats[g->feature];
      J.stream = UINT64_MAX - g->feature;
      J.hp_dst = h.hp_dev;
      J.aux_dst = h.family == MSC_DD || h.family == MSC_DM ? &st->desc_dev[g->feature].aux : nullptr;
    }
  }
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.part, part));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.out, out));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.jobs_dev, n));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.chosen_dev, n));
  const hipStream_t s = st->ctx->stream;
  MSC_HIP(hipMemcpyAsync(st->hp.jobs_dev, jobs.data(), n * sizeof(HpJob), hipMemcpyHostToDevice, s));
  if (nfj && launch_hp_grid_score(s, st->hp.jobs_dev, nfj, (uint32_t)max_np, st->K, st->kpad, st->cnt_u32, slots_dev, nblk,
                                  st->hp.part, st->hp.out))
    return fail(MSC_EHIP, "k_hp_grid_score launch failed");
  if (nfj < n && launch_crp_grid_score(s, st->hp.jobs_dev + nfj, jobs[nfj].npoints, st->cnt_u32, st->K, st->hp.out))
    return fail(MSC_EHIP, "k_crp_grid_score launch failed");
  if (launch_hp_grid_draw(s, st->hp.jobs_dev, n, st->hp.out, seed, sweep, st->hp.chosen_dev))
    return fail(MSC_EHIP, "k_hp_grid_draw launch failed");
  std::vector<uint32_t> picked(n);
  MSC_HIP(hipMemcpyAsync(picked.data(), st->hp.chosen_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));                   // the step's one wait
  // the draw kernel has set the device hp (and a dd / dm descriptor's alpha sum); the host's bookkeeping follows as
  // msc_state_set_hp / msc_state_set_alpha keep it
  int rc = MSC_OK;
  for (uint32_t j = 0; j < n; j++) {
    const msc_hp_grid *g = grids[order[j]];
    const uint32_t k = picked[j];
    chosen_host[order[j]] = k;
    if (k >= jobs[j].npoints) {
      rc = fail(MSC_EINVAL, "grid %u: no point has a finite positive weight; nothing installed", order[j]);
      continue;
    }
    const float *blk = g->blocks.data() + (size_t)k * jobs[j].hpf;
    if (g->feature == MSC_HP_CLUSTER) alpha_installed(st, blk[0]);
    else hp_installed(st, g->feature, blk);
  }
  return rc;
}

// ---------------------------------------------------------------------------
// slice sampling of hyper-parameters and bbnc group parameters (downstream's hp / theta kernels; kernels_slice.hip)
// ---------------------------------------------------------------------------
static size_t slice_align(size_t n) { return (n + 15) & ~(size_t)15; }

// the support of a coordinate: every coordinate sliced is a positive float but nich mu
static const char *slice_unsupported(int family, uint32_t coord) {
  switch (family) {
    case MSC_BB: case MSC_BBNC: case MSC_GP: case MSC_NICH: return nullptr;
    case MSC_BNB: return coord == 2 ? "bnb r is an integer" : nullptr;
    case MSC_DD: case MSC_DM: return "dd / dm alphas are not sliced";
    case MSC_NIW: return "niw hyper-parameters are not sliced";
    default: return "the family has no hyper-parameters";
  }
}

// The argument checks of a slice step and its plan: the targets in order of first appearance (slot nfeat = alpha), each
// with its entries in the caller's order.  Reads of `st` only what msc_chains_create makes equal over an ensemble's
// members (the feature list), so one plan serves them all.
int msc::slice_plan(const msc_state *st, const msc_slice_coord *coords, uint32_t n, SlicePlan &plan) {
  std::vector<int32_t> tix(st->nfeat + 1, -1);
  std::vector<std::vector<uint32_t>> members;
  std::vector<uint32_t> &tslot = plan.tslot;
  tslot.clear();
  for (uint32_t i = 0; i < n; i++) {
    const msc_slice_coord &c = coords[i];
    const bool cluster = c.feature == MSC_HP_CLUSTER;
    uint32_t hpf = 1;
    if (cluster) {
      MSC_REQUIRE(c.coord == 0, "entry %u: alpha has one coordinate, not %u", i, c.coord);
      MSC_REQUIRE(c.prior != MSC_PRIOR_NONINF_BETA, "entry %u: alpha has no partner for a noninformative beta prior", i);
    } else {
      MSC_REQUIRE(c.feature < st->nfeat, "entry %u: feature %u out of range", i, c.feature);
      const msc_feature_host &h = st->feats[c.feature];
      if (const char *why = slice_unsupported(h.family, c.coord))
        return fail(MSC_EUNSUPPORTED, "entry %u (feature %u): %s", i, c.feature, why);
      hpf = (uint32_t)h.hp.size();
      MSC_REQUIRE(c.coord < hpf, "entry %u: coordinate %u outside feature %u's hp block of %u floats", i, c.coord,
                  c.feature, hpf);
      MSC_REQUIRE(c.prior != MSC_PRIOR_NONINF_BETA || (c.partner < hpf && c.partner != c.coord),
                  "entry %u: partner %u is not another coordinate of feature %u", i, c.partner, c.feature);
    }
    MSC_REQUIRE(c.width > 0.f && std::isfinite(c.width), "entry %u: width %g is not a positive finite float", i,
                (double)c.width);
    MSC_REQUIRE(c.prior <= MSC_PRIOR_NONINF_BETA, "entry %u: unknown prior %u", i, c.prior);
    MSC_REQUIRE(c.prior != MSC_PRIOR_EXPONENTIAL || (c.prior_a > 0.f && std::isfinite(c.prior_a)),
                "entry %u: exponential prior with lambda %g", i, (double)c.prior_a);
    MSC_REQUIRE(c.prior != MSC_PRIOR_NORMAL || (c.prior_b > 0.f && std::isfinite(c.prior_b) && std::isfinite(c.prior_a)),
                "entry %u: normal prior with mu %g, sigma2 %g", i, (double)c.prior_a, (double)c.prior_b);
    const uint32_t slot = cluster ? st->nfeat : c.feature;
    if (tix[slot] < 0) {
      tix[slot] = (int32_t)members.size();
      members.emplace_back();
      tslot.push_back(slot);
    }
    members[(size_t)tix[slot]].push_back(i);
  }
  const uint32_t nt = (uint32_t)members.size();
  plan.first.assign(nt, 0);
  plan.count.assign(nt, 0);
  plan.dc.assign(n, SliceCoord());
  plan.caller.assign(n, 0);
  uint32_t at = 0;
  for (uint32_t t = 0; t < nt; t++) {
    plan.first[t] = at;
    plan.count[t] = (uint32_t)members[t].size();
    for (uint32_t i : members[t]) {
      const msc_slice_coord &c = coords[i];
      plan.dc[at] = SliceCoord{c.coord, c.prior, c.prior == MSC_PRIOR_NONINF_BETA ? c.partner : 0u, c.width, c.prior_a,
                               c.prior_b};
      plan.caller[at++] = i;
    }
  }
  return MSC_OK;
}

// the plan's targets as state `st` holds them now: its tables, its hp blocks, its alpha
void msc::slice_targets(const msc_state *st, const SlicePlan &plan, SliceTarget *targets) {
  for (uint32_t t = 0; t < plan.ntargets(); t++) {
    SliceTarget &T = targets[t];
    std::memset(&T, 0, sizeof T);
    const uint32_t slot = plan.tslot[t];
    T.target = slot;
    T.first = plan.first[t];
    T.n = plan.count[t];
    if (slot == st->nfeat) {
      T.family = kHpCluster;
      T.hpf = 1;
      T.alpha = st->alpha;
    } else {
      const msc_feature_host &h = st->feats[slot];
      T.family = h.family;
      T.hpf = (uint32_t)h.hp.size();
      T.nu32 = raw_u32_rows(h.family, h.dim);
      T.nf32 = raw_f32_rows(h.family);
      T.raw_u32 = h.raw_u32;
      T.raw_f32 = h.raw_f32;
      T.hp = h.hp_dev;
    }
  }
}

// A slice kernel has written every target's final values (val / ev / stat: the plan's n entries in device order) and
// every feature's final block into its device hp; the host's bookkeeping of `st` follows, the caller's outputs (nullable,
// in the caller's order) are filled, and a target that was not finite at its current value is reported -- naming the
// chain when chain >= 0.
int msc::slice_installed(msc_state *st, const SlicePlan &plan, const msc_slice_coord *coords, const float *val,
                         const uint32_t *ev, const uint32_t *stat, float *values_host, uint32_t *evals_host, int64_t chain) {
  int rc = MSC_OK;
  for (uint32_t t = 0; t < plan.ntargets(); t++) {
    const uint32_t first = plan.first[t], end = first + plan.count[t];
    if (plan.tslot[t] == st->nfeat) {
      alpha_installed(st, val[end - 1]);
    } else {
      std::vector<float> blk = st->feats[plan.tslot[t]].hp;
      for (uint32_t e = first; e < end; e++) blk[plan.dc[e].coord] = val[e];
      hp_installed(st, plan.tslot[t], blk.data());
    }
  }
  char who[32] = "";
  if (chain >= 0) std::snprintf(who, sizeof who, "chain %lld, ", (long long)chain);
  for (uint32_t e = 0; e < plan.n(); e++) {
    const uint32_t i = plan.caller[e];
    if (values_host) values_host[i] = val[e];
    if (evals_host) evals_host[i] = ev[e];
    if (stat[e] == kSliceNonFinite)
      rc = fail(MSC_EINVAL, "%sentry %u (%s %u, coordinate %u): the target at the current value is not finite; left "
                "unchanged", who, i, coords[i].feature == MSC_HP_CLUSTER ? "alpha" : "feature",
                coords[i].feature == MSC_HP_CLUSTER ? 0u : coords[i].feature, coords[i].coord);
  }
  return rc;
}

extern "C" int msc_hp_slice(msc_state *st, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                            uint64_t seed, uint64_t sweep, float *values_host, uint32_t *evals_host) {
  MSC_REQUIRE(st && coords, "null argument");
  MSC_REQUIRE(n > 0, "no coordinates");
  MSC_TRY(refuse_mid_step(st, "msc_hp_slice"));
  SlicePlan plan;
  MSC_TRY(slice_plan(st, coords, n, plan));
  const uint32_t nt = plan.ntargets();
  std::vector<SliceTarget> targets(nt);
  slice_targets(st, plan, targets.data());
  const std::vector<SliceCoord> &dc = plan.dc;
  // one buffer: targets | entries | values | evals | status
  const size_t o_coord = slice_align(nt * sizeof(SliceTarget)), o_val = o_coord + slice_align(n * sizeof(SliceCoord));
  const size_t o_ev = o_val + slice_align(n * 4), o_stat = o_ev + slice_align(n * 4), total = o_stat + slice_align(n * 4);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.slice_buf, total));
  std::vector<unsigned char> up(o_val);
  std::memcpy(up.data(), targets.data(), nt * sizeof(SliceTarget));
  std::memcpy(up.data() + o_coord, dc.data(), n * sizeof(SliceCoord));
  const hipStream_t s = st->ctx->stream;
  unsigned char *b = st->hp.slice_buf;
  MSC_HIP(hipMemcpyAsync(b, up.data(), up.size(), hipMemcpyHostToDevice, s));
  if (launch_hp_slice(s, reinterpret_cast<const SliceTarget *>(b), nt, reinterpret_cast<const SliceCoord *>(b + o_coord),
                      st->K, st->kpad, st->cnt_u32, slots_dev, seed ^ kSliceKey, sweep, reinterpret_cast<float *>(b + o_val),
                      reinterpret_cast<uint32_t *>(b + o_ev), reinterpret_cast<uint32_t *>(b + o_stat)))
    return fail(MSC_EHIP, "k_hp_slice launch failed");
  std::vector<unsigned char> down(total - o_val);
  MSC_HIP(hipMemcpyAsync(down.data(), b + o_val, down.size(), hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));                   // the call's one wait
  const float *val = reinterpret_cast<const float *>(down.data());
  const uint32_t *ev = reinterpret_cast<const uint32_t *>(down.data() + (o_ev - o_val));
  const uint32_t *stat = reinterpret_cast<const uint32_t *>(down.data() + (o_stat - o_val));
  return slice_installed(st, plan, coords, val, ev, stat, values_host, evals_host, -1);
}

extern "C" int msc_theta_slice(msc_state *st, const uint32_t *features, const float *widths, uint32_t n,
                               const uint8_t *slots_dev, uint64_t seed, uint64_t sweep, uint64_t *evals_host) {
  MSC_REQUIRE(st && features && widths, "null argument");
  MSC_REQUIRE(n > 0, "no features");
  MSC_TRY(refuse_mid_step(st, "msc_theta_slice"));
  std::vector<bool> seen(st->nfeat, false);
  std::vector<ThetaJob> jobs(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = features[i];
    MSC_REQUIRE(f < st->nfeat, "feature %u out of range", f);
    const msc_feature_host &h = st->feats[f];
    MSC_REQUIRE(h.family == MSC_BBNC, "feature %u is not bbnc: only bbnc groups carry a parameter", f);
    MSC_REQUIRE(!seen[f], "feature %u twice in one call", f);
    seen[f] = true;
    MSC_REQUIRE(widths[i] > 0.f && std::isfinite(widths[i]), "feature %u: width %g is not a positive finite float", f,
                (double)widths[i]);
    jobs[i] = ThetaJob{h.raw_u32, h.raw_f32, h.hp_dev, widths[i], f};
  }
  const uint32_t nb = theta_slice_blocks(st->K);
  const size_t np = (size_t)n * nb;
  const size_t o_ev = slice_align(n * sizeof(ThetaJob)), o_bad = o_ev + np * 8, total = o_bad + slice_align(np * 4);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  MSC_HIP(reserve_synced(st->ctx->stream, st->hp.slice_buf, total));
  const hipStream_t s = st->ctx->stream;
  unsigned char *b = st->hp.slice_buf;
  MSC_HIP(hipMemcpyAsync(b, jobs.data(), n * sizeof(ThetaJob), hipMemcpyHostToDevice, s));
  if (launch_theta_slice(s, reinterpret_cast<const ThetaJob *>(b), n, st->K, st->kpad, st->cnt_u32, slots_dev,
                         seed ^ kSliceKey, sweep, reinterpret_cast<unsigned long long *>(b + o_ev),
                         reinterpret_cast<uint32_t *>(b + o_bad)))
    return fail(MSC_EHIP, "k_theta_slice launch failed");
  std::vector<unsigned char> down(total - o_ev);
  MSC_HIP(hipMemcpyAsync(down.data(), b + o_ev, down.size(), hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));                   // the call's one wait
  const unsigned long long *ev = reinterpret_cast<const unsigned long long *>(down.data());
  const uint32_t *bad = reinterpret_cast<const uint32_t *>(down.data() + np * 8);
  int rc = MSC_OK;
  for (uint32_t i = 0; i < n; i++) {
    st->valid.hp_changed(features[i]);                // (p is read by the bbnc prepare and the fused bool tables)
    uint64_t t = 0;
    uint32_t first_bad = 0xffffffffu;
    for (uint32_t x = 0; x < nb; x++) {
      t += ev[(size_t)i * nb + x];
      first_bad = std::min(first_bad, bad[(size_t)i * nb + x]);
    }
    if (evals_host) evals_host[i] = t;
    if (first_bad != 0xffffffffu)
      rc = fail(MSC_EINVAL, "feature %u, slot %u: the target at the current p is not finite; the slot is left unchanged",
                features[i], first_bad);
  }
  return rc;
}

// ---------------------------------------------------------------------------
// the log joint log p(X, z | hp, alpha) of a state (kernels_joint.hip)
// ---------------------------------------------------------------------------
// What msc_score_joint and msc_chains_score_joint (chains.cpp) check of a state's feature list and of the entries before
// anything is launched, and the entries as the kernels take them, in the CALLER's order (the order p is added in).
int msc::joint_entries(const msc_state *st, const char *who, const msc_slice_coord *coords, uint32_t n,
                       std::vector<JointCoord> &entries) {
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (st->feats[f].family == MSC_NIW)
      return fail(MSC_EUNSUPPORTED, "%s: feature %u is niw, whose score_data the double evaluator (hp_eval) does not have", who,
                  f);
  entries.clear();
  if (n == 0) return MSC_OK;
  SlicePlan plan;
  MSC_TRY(slice_plan(st, coords, n, plan));          // msc_hp_slice's checks
  entries.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const msc_slice_coord &c = coords[i];
    entries.push_back(JointCoord{c.feature, c.coord, c.prior, c.prior == MSC_PRIOR_NONINF_BETA ? c.partner : c.coord,
                                 c.prior_a, c.prior_b});
  }
  return MSC_OK;
}

extern "C" int msc_score_joint(msc_state *st, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                               double *out_dev) {
  MSC_REQUIRE(st, "null state");
  const joint::JointCheck chk = joint::check_score_joint("msc_score_joint", out_dev != nullptr, coords != nullptr, n, st->nfeat,
                                                         joint::joint_row(st->nfeat), slots_dev != nullptr, 0, st->K);
  MSC_REQUIRE(chk.ok, "%s", chk.message);
  MSC_TRY(refuse_mid_step(st, "msc_score_joint"));
  std::vector<JointCoord> entries;
  MSC_TRY(joint_entries(st, "msc_score_joint", coords, n, entries));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  MSC_TRY(ensure_raw(st));
  if (launch_score_joint(st->ctx->stream, st->desc_dev, st->nfeat, st->K, st->kpad, st->cnt_u32, slots_dev, st->alpha,
                         entries.data(), n, out_dev))
    return fail(MSC_EHIP, "k_score_joint launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MSC_OK;
}
