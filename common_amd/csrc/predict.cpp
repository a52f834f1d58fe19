// predict.cpp -- predictions from a state: the row predictive log-density (kernels_marginal.hip: msc_score_marginal) and
// posterior predictive sampling (kernels_pred.hip: msc_sample_predictive).  Host logic only; the core it stands on is
// abi.cpp, through abi_internal.hpp.
#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "launchers.hpp"

using namespace msc;

// ---------------------------------------------------------------------------
// row predictive log-density (kernels_marginal.hip): a row's K totals -- what msc_score_value with the prior defines --
// reduced to their log-sum-exp, arg-max and the arg-max's log responsibility
// ---------------------------------------------------------------------------
// (Which kernels reduce a state's rows: route_calls.hpp route_marginal, by the state and the view's rows alone.)

extern "C" int msc_score_marginal(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                                  const int32_t *z_dev, uint32_t flags, float *logp_dev, int32_t *map_dev,
                                  float *map_logresp_dev) {
  MSC_REQUIRE(st && (logp_dev || nrows == 0), "null argument");
  MSC_REQUIRE(flags == 0, "unknown flags 0x%x", flags);
  MSC_TRY(refuse_mid_step(st, "msc_score_marginal"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  MSC_TRY(ensure_derived(st));
  MSC_TRY(ensure_crp(st));
  hipStream_t s = st->ctx->stream;
  const int cus = st->ctx->num_cus;
  MSC_HIP(grow_retained(st->retired, st->marg_norm, 2));
  MSC_TRY(launch_marginal_norm(s, st->cnt_u32, st->K, st->alpha, st->marg_norm));
  switch (route_marginal(route_facts_now(st), read_switches())) {                        // (the launchers report their own failures)
    case MarginalKind::nich1:
      return launch_marginal_nich1(s, cus, st->desc_dev, st->K, st->kpad, row0, nrows, z_dev, st->logpc, st->marg_norm, logp_dev,
                                   map_dev, map_logresp_dev);
    case MarginalKind::tile:
      if (z_dev) MSC_TRY(run_loo_own(st, row0, nrows, z_dev, true));
      MSC_TRY(refresh_fused_tables(st));                  // (the kernel walks the fused plan)
      return launch_marginal_tile(s, cus, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows,
                                  z_dev, st->own, st->logpc, st->marg_norm, logp_dev, map_dev, map_logresp_dev);
    case MarginalKind::generic: {
      // (the chunk of SweepKind::generic; the scratch is the state's and stays with it, grown to what the largest call
      // asked for)
      const auto [ld, chunk] = score_chunk(st->K, st->kpad, nrows);
      MSC_HIP(grow_retained(st->retired, st->scratch, chunk * ld));
      for (uint64_t at = 0; at < nrows; at += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, nrows - at);
        MSC_TRY(run_score(st, row0 + at, n, z_dev ? z_dev + at : nullptr, true, false, st->scratch, ld));
        MSC_TRY(launch_row_lse(s, cus, st->scratch, ld, st->K, n, z_dev ? z_dev + at : nullptr, st->marg_norm, logp_dev + at,
                               map_dev ? map_dev + at : nullptr, map_logresp_dev ? map_logresp_dev + at : nullptr));
      }
      return MSC_OK;
    }
  }
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// posterior predictive sampling (group::sample_value, base.hpp:29, for a block of rows; kernels_pred.hip)
// ---------------------------------------------------------------------------
static constexpr uint64_t kPredGroupKey = 0xD1B54A32D192ED03ull;   // the group draw's key is seed ^ this

extern "C" int msc_sample_predictive(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                     uint64_t nrows, uint64_t row_id0, const int32_t *z_dev, int32_t *z_out_dev,
                                     uint32_t flags, uint64_t seed, uint64_t sweep, void *const *out_dev) {
  MSC_REQUIRE(st && view && out_dev, "null argument");
  MSC_REQUIRE((flags & ~MSC_PRED_MASKED_ONLY) == 0, "unknown flags 0x%x", flags);
  MSC_TRY(refuse_mid_step(st, "msc_sample_predictive"));
  for (uint32_t f = 0; f < st->nfeat; f++) {
    if (out_dev[f] == nullptr) continue;
    const int fam = st->feats[f].family;
    if (fam == MSC_DM)
      return fail(MSC_EUNSUPPORTED, "feature %u: dm has no sample_value upstream (dm.cpp:100-111)", f);
    if (fam == MSC_NOOP) return fail(MSC_EUNSUPPORTED, "feature %u: the noop model has no values to draw", f);
    MSC_REQUIRE(f < 0x8000u, "feature %u: the draw's Philox counter holds feature indices below 32768", f);
  }
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  MSC_TRY(ensure_derived(st));                              // (raw tables current; niw: the whitening matrices)
  const hipStream_t s = st->ctx->stream;
  // the features drawn and their parameter blocks
  std::vector<PredFeat> pfs;
  std::vector<size_t> par_off;                              // each drawn feature's first double in pred_par
  size_t par_len = 0;
  for (uint32_t f = 0; f < st->nfeat; f++) {
    if (out_dev[f] == nullptr) continue;
    const msc_feature_host &h = st->feats[f];
    const FeatDesc &d = st->desc_host[f];
    PredFeat p;
    p.family = h.family;
    p.dim = h.dim;
    p.feature = f;
    p.stride = pred_par_stride(h.family, h.dim);
    p.par = nullptr;                                        // (set below, once the buffer is known)
    p.hp = h.hp_dev;
    p.raw_u32 = h.raw_u32;
    p.raw_f32 = h.raw_f32;
    p.niw_w64 = h.niw_w64;
    p.col = d.col;
    p.mask = d.mask;
    p.out = out_dev[f];
    pfs.push_back(p);
    par_off.push_back(par_len);
    par_len += (size_t)p.stride * st->K;
  }
  MSC_HIP(reserve_synced(st->ctx->stream, st->pred.par, par_len));
  if (pfs.size() > st->pred.feats_dev.size() || !st->pred.feats_dev) st->pred.feats_host.clear();   // (a new buffer holds nothing)
  MSC_HIP(reserve_synced(st->ctx->stream, st->pred.feats_dev, pfs.size()));
  for (size_t i = 0; i < pfs.size(); i++) pfs[i].par = st->pred.par + par_off[i];
  // the descriptors go up only when they changed (a loop of calls uploads nothing)
  const size_t pbytes = pfs.size() * sizeof(PredFeat);
  if (pbytes && (st->pred.feats_host.size() != pfs.size() ||
                 std::memcmp(st->pred.feats_host.data(), pfs.data(), pbytes) != 0)) {
    PredFeat *stage = nullptr;
    MSC_HIP(st->pred.upload.begin(pbytes, &stage));
    std::memcpy(stage, pfs.data(), pbytes);
    MSC_HIP(st->pred.upload.commit(s, st->pred.feats_dev, pbytes));
    st->pred.feats_host = pfs;
  }
  if (launch_pred_prepare(s, st->pred.feats_dev, pfs, st->K, st->kpad)) return fail(MSC_EHIP, "k_pred_prepare launch failed");
  // the group draw: the sweep's own assignment pass for rows that are all unassigned, under a key no sweep uses; the
  // sweep's (seed, sweep) pair on the device is put back afterwards
  const int32_t *z = z_dev;
  if (z == nullptr) {
    MSC_HIP(reserve_synced(st->ctx->stream, st->pred.z, nrows));
    MSC_HIP(hipMemsetAsync(st->pred.z, 0xff, nrows * sizeof(int32_t), s));
    const RngMirror had = st->rng.snapshot();
    MSC_TRY(sweep_assign_impl(st, view, cols, row0, nrows, row_id0, st->pred.z, seed ^ kPredGroupKey, sweep));
    st->rng.invalidate();
    if (had.valid()) {
      if (launch_rng_set(s, st->rng_dev, had.seed(), had.sweep())) return fail(MSC_EHIP, "k_rng_set launch failed");
      st->rng.restore(had);
    }
    z = st->pred.z;
  }
  if (launch_pred_sample(s, st->pred.feats_dev, pfs, st->K, row0, nrows, row_id0, z, z_out_dev,
                         (flags & MSC_PRED_MASKED_ONLY) != 0, seed, sweep))
    return fail(MSC_EHIP, "k_pred_sample launch failed");
  return MSC_OK;
}
