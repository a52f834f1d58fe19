// chains.cpp -- the sequential collapsed Gibbs sweep and the ensembles of such chains (kernels_seq.hip):
// msc_sweep_sequential and msc_chains_*, the sweep at a temperature, the exchange of temperatures and the annealing weights (kernels_temper.hip), the
// ensemble's row predictive density (kernels_chains_marginal.hip), its
// posterior predictive draws (kernels_chains_pred.hip) and its split-merge proposals (kernels_chains_sm.hip) among them.
// Host logic only; the core it stands on is abi.cpp, through abi_internal.hpp.
#include <algorithm>
#include <memory>
#include <new>

#include "abi_internal.hpp"
#include "chains_layout.hpp"
#include "launchers.hpp"
#include "temper_math.hpp"

using namespace msc;

// ---------------------------------------------------------------------------
// The sequential sweep (k_sweep_seq): one workgroup carries the chain; the state carries over in global memory between
// launches, and a launch takes as many row visits as fit kSeqLaunchUs by seq_visit_us (route_calls.hpp: whether the
// kernel takes a state, route_sequential; a launch's share, units_per_launch).
// ---------------------------------------------------------------------------

extern "C" int msc_sweep_sequential(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                    uint64_t nrows, uint64_t row_id0, int32_t *z_dev, const uint32_t *order_dev,
                                    uint32_t nsweeps, uint64_t seed, uint64_t sweep, int32_t *trace_dev) {
  MSC_REQUIRE(st && view && (z_dev || nrows == 0), "null argument");
  MSC_REQUIRE(nrows < (1ull << 32), "the sequential sweep takes at most 2^32 - 1 rows per call");
  MSC_TRY(refuse_mid_step(st, "msc_sweep_sequential"));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  const SeqRoute route = route_sequential(route_facts_now(st));
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why);
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  if (nrows == 0 || nsweeps == 0) return MSC_OK;
  // every table current before (as msc_entity_op)
  hipStream_t s = st->ctx->stream;
  MSC_TRY(ensure_all_current(st));
  const uint64_t visits = (uint64_t)nsweeps * nrows;
  const uint64_t per_launch = units_per_launch(1, st->ctx->num_cus, seq_visit_us(route_facts_now(st)));
  for (uint64_t v0 = 0; v0 < visits; v0 += per_launch) {
    const uint64_t v1 = std::min(visits, v0 + per_launch);
    const int rc = launch_sweep_seq(s, st->desc_dev, (int)st->nfeat, st->K, st->kpad, row0, nrows, row_id0, z_dev, order_dev,
                                    v0, v1, seed, sweep, st->red_i64, st->cnt_u32, st->alpha, st->logpc, trace_dev);
    if (rc == -2) return fail(MSC_EUNSUPPORTED, "k_sweep_seq does not take this shape");
    if (rc) return fail(MSC_EHIP, "k_sweep_seq launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  // the kernel kept every table current: additive sums, fields, constants, counts and CRP terms
  st->valid.kept_current();
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// Many sequential chains in one launch (k_sweep_seq_chains): workgroup c carries the chain of member state c.
// ---------------------------------------------------------------------------
struct msc_chains {
  msc_context *ctx = nullptr;
  std::vector<msc_state *> states;
  // The table of a call, whichever call it is: filled on the host through `upload` and copied to call_tab on the stream.
  // One device buffer serves every call because every ensemble call enqueues on ctx->stream: a call's copy queues behind
  // the launches of the call before it, which are the last readers of what it overwrites.  (msc_context_set_stream
  // between two calls leaves that ordering to the caller, as it does for every buffer of a state.)  Sized at create for
  // the largest of the layouts that nchains and nfeat fix; msc_chains_hp_slice, whose block follows the call's
  // coordinates, grows it by reserve_synced.
  msc::StagedUpload upload;
  msc::DevBuf<unsigned char> call_tab;
  // msc_chains_hp_slice: what the call brings back (values | evals | status), grown by reserve_synced, and its host image
  msc::DevBuf<unsigned char> hp_out;
  std::vector<unsigned char> hp_down;
  // msc_chains_score_marginal: the normalised log weights and log(n + alpha) of every chain; the slices' (M, S) pairs,
  // grown without a wait (the buffer it replaces may still be read)
  msc::DevBuf<double> marg_w;             // [2 nchains]: lw | norm
  msc::DevBuf<double> marg_part;
  // msc_chains_sample_predictive: the chains' rows of a chunk (float [nchains][chunk]) and the chunk's rows' chain and
  // group (int32 [2][chunk]), grown as marg_part is
  msc::DevBuf<float> pred_lf;
  msc::DevBuf<int32_t> pred_cz;
  // msc_chains_split_merge: the chains' pair labels, int32 [nchains][nrows], grown by reserve_synced
  msc::DevBuf<int32_t> sm_ell;
  msc::Retired retired;

  template <typename T>
  T *table() const { return reinterpret_cast<T *>(call_tab.get()); }   // call_tab as the table the call uploaded
};

// the marginal / predictive call's block for nsel selected features
static layout::MargBlock marg_block(const msc_chains *ch, uint32_t nsel) {
  return layout::marg_block(ch->states.size(), nsel, ch->states[0]->nfeat, sizeof(MargChain), sizeof(MargFeat),
                            sizeof(void *));
}

// How every call on an ensemble begins.  No member mid-step (chains_refuse_mid_step, for a call that checks its own
// arguments between that and the device); the device, and what an earlier kernel reported; with a view, the view bound
// to every member; then the members' tables as current as the call's kernels need them.
static int chains_refuse_mid_step(const msc_chains *ch, const char *who) {
  for (uint32_t c = 0; c < ch->states.size(); c++)
    MSC_REQUIRE(!ch->states[c]->rng.mid_step(), "%s: state %u is between msc_sweep_step_begin and "
                                                "msc_state_commit_reduce: its additive tables hold uncommitted sums", who, c);
  return MSC_OK;
}
static int chains_device(const msc_chains *ch) {
  MSC_HIP(hipSetDevice(ch->ctx->device));
  return device_error_check(ch->ctx);
}
enum class ChainsEnsure { none, raw, derived_crp, all_current };
static int chains_enter(msc_chains *ch, const char *who, ChainsEnsure ensure, const msc_dataview *view = nullptr,
                        const uint32_t *cols = nullptr, uint64_t row0 = 0, uint64_t nrows = 0) {
  MSC_TRY(chains_refuse_mid_step(ch, who));
  MSC_TRY(chains_device(ch));
  if (view)
    for (msc_state *st : ch->states) MSC_TRY(bind_view(st, view, cols, row0, nrows));
  for (msc_state *st : ch->states) {
    if (ensure == ChainsEnsure::raw) MSC_TRY(ensure_raw(st));
    if (ensure == ChainsEnsure::derived_crp) MSC_TRY(ensure_derived(st));
    if (ensure == ChainsEnsure::derived_crp) MSC_TRY(ensure_crp(st));
    if (ensure == ChainsEnsure::all_current) MSC_TRY(ensure_all_current(st));
  }
  return MSC_OK;
}

extern "C" int msc_chains_create(msc_state *const *states, uint32_t nchains, msc_chains **out) {
  MSC_REQUIRE(states && out, "null argument");
  *out = nullptr;
  MSC_REQUIRE(nchains >= 1, "msc_chains_create: at least one state");
  for (uint32_t c = 0; c < nchains; c++) {
    const msc_state *st = states[c];
    MSC_REQUIRE(st, "msc_chains_create: state %u is null", c);
    MSC_REQUIRE(st->ctx == states[0]->ctx, "msc_chains_create: state %u lives on another context than state 0", c);
    for (uint32_t b = 0; b < c; b++)
      MSC_REQUIRE(states[b] != st, "msc_chains_create: state %u is state %u again (two workgroups on one state's tables "
                                   "would race)", c, b);
    MSC_REQUIRE(st->K == states[0]->K, "msc_chains_create: state %u has %u groups, state 0 has %u", c, st->K, states[0]->K);
    MSC_REQUIRE(st->nfeat == states[0]->nfeat, "msc_chains_create: state %u has %u features, state 0 has %u", c, st->nfeat,
                states[0]->nfeat);
    for (uint32_t f = 0; f < st->nfeat; f++)
      MSC_REQUIRE(st->feats[f].family == states[0]->feats[f].family && st->feats[f].dim == states[0]->feats[f].dim,
                  "msc_chains_create: feature %u of state %u (family %d, dim %u) differs from state 0's (family %d, dim %u)",
                  f, c, st->feats[f].family, st->feats[f].dim, states[0]->feats[f].family, states[0]->feats[f].dim);
  }
  const SeqRoute route = route_sequential(route_facts_now(states[0]));   // (equal feature lists and K: one answer for all)
  if (route.rc != MSC_OK) return fail(route.rc, "%s", route.why);
  msc_context *ctx = states[0]->ctx;
  MSC_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<msc_chains> ch(new (std::nothrow) msc_chains());
  if (!ch) return fail(MSC_ENOMEM, "out of host memory");
  ch->ctx = ctx;
  ch->states.assign(states, states + nchains);
  // the largest table a call uploads but msc_chains_hp_slice's: an entry a chain, or the sampling call's block
  const size_t entry = std::max({sizeof(SeqChain), sizeof(ClonePair), sizeof(SmChain), sizeof(JointChain)});
  const size_t tab_bytes = std::max(nchains * entry, marg_block(ch.get(), states[0]->nfeat).bytes);
  hipError_t e = ch->call_tab.alloc(tab_bytes);
  if (e == hipSuccess) e = ch->upload.reserve(tab_bytes);
  if (e == hipSuccess) e = ch->marg_w.alloc(2 * (size_t)nchains);
  if (e != hipSuccess) return fail(MSC_EHIP, "msc_chains_create: %s", hipGetErrorString(e));
  for (msc_state *st : ch->states) st->chain_members++;
  *out = ch.release();
  return MSC_OK;
}

extern "C" int msc_chains_destroy(msc_chains *ch) {
  if (!ch) return MSC_OK;
  (void)hipSetDevice(ch->ctx->device);
  (void)hipStreamSynchronize(ch->ctx->stream);             // (a launch may still read the table)
  for (msc_state *st : ch->states) st->chain_members--;
  delete ch;
  return MSC_OK;
}

extern "C" int msc_chains_size(const msc_chains *ch, uint32_t *nchains) {
  MSC_REQUIRE(ch && nchains, "null argument");
  *nchains = (uint32_t)ch->states.size();
  return MSC_OK;
}

// What msc_chains_sweep, msc_chains_sweep_tempered and msc_chains_visit share: visits [v0, v1) of a call's nsweeps x nrows
// for every chain (visit v is sweep v / nrows, position v % nrows of the order), with the outputs each has (null: not
// wanted).  beta_dev (msc_chains_sweep_tempered; else null): the chains' temperatures on the device, handed to the
// kernel as they lie -- never read or uploaded here, so what msc_chains_exchange swapped is what the launch reads.
struct ChainsOutputs {
  uint32_t trace_every = 1;           // >= 1
  uint64_t ntrace = 0;                // samples per chain of trace / occupied
  int32_t *trace = nullptr;           // [nchains][ntrace][nrows]
  uint32_t *occupied = nullptr;       // [nchains][ntrace]
  double *logw = nullptr;             // [nchains]
  float *visit_logp = nullptr;        // chain c's at + c * ld_logp
  uint64_t ld_logp = 0;
};
static int chains_visits_impl(msc_chains *ch, const char *who, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                              uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev,
                              uint64_t ld_order, uint64_t v0, uint64_t v1, const uint64_t *host_seeds, uint64_t sweep,
                              const ChainsOutputs &out, const float *beta_dev = nullptr) {
  const uint32_t n = (uint32_t)ch->states.size();
  const char *kernel = beta_dev ? "k_sweep_seq_chains_tempered" : "k_sweep_seq_chains";
  MSC_REQUIRE((z_dev && host_seeds) || v0 >= v1, "null argument");
  MSC_REQUIRE(nrows < (1ull << 32), "the sequential sweep takes at most 2^32 - 1 rows per call");
  MSC_REQUIRE(ld_z >= nrows, "%s: ld_z %llu < nrows %llu", who, (unsigned long long)ld_z, (unsigned long long)nrows);
  MSC_REQUIRE(!order_dev || ld_order == 0 || ld_order >= nrows, "%s: ld_order %llu is neither 0 (one order "
              "for all chains) nor >= nrows %llu", who, (unsigned long long)ld_order, (unsigned long long)nrows);
  // every table of every member current before visits are made, as msc_sweep_sequential
  MSC_TRY(chains_enter(ch, who, v0 < v1 ? ChainsEnsure::all_current : ChainsEnsure::none, view, cols, row0, nrows));
  if (v0 >= v1) return MSC_OK;
  hipStream_t s = ch->ctx->stream;
  double visit_us = 0.0;                                    // (as msc_sweep_sequential, by the costliest member)
  for (msc_state *st : ch->states) visit_us = std::max(visit_us, seq_visit_us(route_facts_now(st)));
  // the table of this call (pointers and alpha may have changed since the last one)
  SeqChain *tab = nullptr;
  MSC_HIP(ch->upload.begin(sizeof(SeqChain) * n, &tab));
  for (uint32_t c = 0; c < n; c++) {
    const msc_state *st = ch->states[c];
    SeqChain &e = tab[c];
    e.feats = st->desc_dev;
    e.cnt_acc = st->red_i64;
    e.cnt_u32 = st->cnt_u32;
    e.crp = st->logpc;
    e.z = z_dev + (size_t)c * ld_z;
    e.order = order_dev ? order_dev + (size_t)c * ld_order : nullptr;
    e.trace = out.trace && out.ntrace ? out.trace + (size_t)c * out.ntrace * nrows : nullptr;
    e.occupied = out.occupied && out.ntrace ? out.occupied + (size_t)c * out.ntrace : nullptr;
    e.logw = out.logw ? out.logw + c : nullptr;
    e.visit_logp = out.visit_logp ? out.visit_logp + (size_t)c * out.ld_logp : nullptr;
    e.seed = host_seeds[c];
    e.alpha = st->alpha;
    e.pad = 0;
  }
  MSC_HIP(ch->upload.commit(s, ch->call_tab, sizeof(SeqChain) * n));
  const msc_state *st0 = ch->states[0];
  const uint64_t per_launch = units_per_launch(n, ch->ctx->num_cus, visit_us);
  for (uint64_t w0 = v0; w0 < v1; w0 += per_launch) {
    const uint64_t w1 = std::min(v1, w0 + per_launch);
    const int rc = beta_dev ? launch_sweep_seq_chains_tempered(s, ch->table<SeqChain>(), beta_dev, n, (int)st0->nfeat, st0->K,
                                                               st0->kpad, row0, nrows, row_id0, w0, w1, sweep, out.trace_every)
                            : launch_sweep_seq_chains(s, ch->table<SeqChain>(), n, (int)st0->nfeat, st0->K, st0->kpad, row0, nrows,
                                                      row_id0, w0, w1, sweep, out.trace_every);
    if (rc == -2) return fail(MSC_EUNSUPPORTED, "%s does not take this shape", kernel);
    if (rc) return fail(MSC_EHIP, "%s launch failed: %s", kernel, hipGetErrorString(hipGetLastError()));
  }
  // the kernel kept every table of every member current: additive sums, fields, constants, counts and CRP terms
  for (msc_state *st : ch->states) st->valid.kept_current();
  return MSC_OK;
}

extern "C" int msc_chains_sweep(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                                uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order,
                                uint32_t nsweeps, const uint64_t *host_seeds, uint64_t sweep, uint32_t trace_every,
                                int32_t *trace_dev, uint32_t *occupied_dev) {
  MSC_REQUIRE(ch && view, "null argument");
  if (ch->states.empty()) return MSC_OK;
  const bool tracing = trace_dev != nullptr || occupied_dev != nullptr;
  MSC_REQUIRE(!tracing || trace_every >= 1, "msc_chains_sweep: trace_every must be >= 1 with a trace or an occupied array");
  ChainsOutputs out;
  out.trace_every = tracing ? trace_every : 1u;
  out.ntrace = tracing ? nsweeps / trace_every : 0;
  out.trace = trace_dev;
  out.occupied = occupied_dev;
  return chains_visits_impl(ch, "msc_chains_sweep", view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, 0,
                            (uint64_t)nsweeps * nrows, host_seeds, sweep, out);
}

// msc_chains_sweep with every chain at its own temperature: the same prologue, table and launch slicing; the kernel is
// k_sweep_seq_chains_tempered, which reads beta_dev[c] on the device at every launch.  No wait, no upload of beta.
extern "C" int msc_chains_sweep_tempered(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                         uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t ld_z,
                                         const uint32_t *order_dev, uint64_t ld_order, uint32_t nsweeps,
                                         const uint64_t *host_seeds, uint64_t sweep, const float *beta_dev, uint32_t trace_every,
                                         int32_t *trace_dev, uint32_t *occupied_dev) {
  MSC_REQUIRE(ch && view, "null argument");
  if (ch->states.empty()) return MSC_OK;
  const uint64_t visits = (uint64_t)nsweeps * nrows;
  MSC_REQUIRE(beta_dev || visits == 0, "msc_chains_sweep_tempered: beta_dev is null");
  const bool tracing = trace_dev != nullptr || occupied_dev != nullptr;
  MSC_REQUIRE(!tracing || trace_every >= 1, "msc_chains_sweep_tempered: trace_every must be >= 1 with a trace or an occupied "
                                            "array");
  ChainsOutputs out;
  out.trace_every = tracing ? trace_every : 1u;
  out.ntrace = tracing ? nsweeps / trace_every : 0;
  out.trace = trace_dev;
  out.occupied = occupied_dev;
  return chains_visits_impl(ch, "msc_chains_sweep_tempered", view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order,
                            0, visits, host_seeds, sweep, out, beta_dev);
}

extern "C" int msc_chains_visit(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                                uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order,
                                uint64_t pos0, uint64_t npos, const uint64_t *host_seeds, uint64_t sweep, double *logw_dev,
                                float *visit_logp_dev, uint64_t ld_logp) {
  MSC_REQUIRE(ch && view, "null argument");
  MSC_REQUIRE(pos0 <= nrows && npos <= nrows - pos0, "msc_chains_visit: positions [%llu, %llu + %llu) beyond nrows %llu",
              (unsigned long long)pos0, (unsigned long long)pos0, (unsigned long long)npos, (unsigned long long)nrows);
  MSC_REQUIRE(!visit_logp_dev || ld_logp >= nrows, "msc_chains_visit: ld_logp %llu < nrows %llu", (unsigned long long)ld_logp,
              (unsigned long long)nrows);
  if (ch->states.empty() || npos == 0) return MSC_OK;
  ChainsOutputs out;
  out.logw = logw_dev;
  out.visit_logp = visit_logp_dev;
  out.ld_logp = ld_logp;
  return chains_visits_impl(ch, "msc_chains_visit", view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, pos0,
                            pos0 + npos, host_seeds, sweep, out);
}

extern "C" int msc_chains_clone(msc_chains *ch, const uint32_t *host_ancestors, int32_t *z_dev, uint64_t ld_z, uint64_t nrows) {
  MSC_REQUIRE(ch && host_ancestors, "null argument");
  const uint32_t n = (uint32_t)ch->states.size();
  MSC_REQUIRE(z_dev || nrows == 0, "null argument");
  MSC_REQUIRE(ld_z >= nrows, "msc_chains_clone: ld_z %llu < nrows %llu", (unsigned long long)ld_z, (unsigned long long)nrows);
  uint32_t npairs = 0;
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t a = host_ancestors[c];
    MSC_REQUIRE(a < n, "msc_chains_clone: ancestor %u of chain %u is not a chain (%u chains)", a, c, n);
    MSC_REQUIRE(host_ancestors[a] == a, "msc_chains_clone: chain %u copies chain %u, which is itself overwritten (by chain "
                                        "%u): a source must survive in place", c, a, host_ancestors[a]);
    npairs += a != c;
  }
  MSC_TRY(chains_refuse_mid_step(ch, "msc_chains_clone"));
  if (npairs == 0) return MSC_OK;
  MSC_TRY(chains_enter(ch, "msc_chains_clone", ChainsEnsure::none));
  hipStream_t s = ch->ctx->stream;
  // a source's additive tables hold the truth before they are read (after a sweep they do: this launches nothing then)
  for (uint32_t c = 0; c < n; c++)
    if (host_ancestors[c] != c) MSC_TRY(ensure_additive(ch->states[host_ancestors[c]]));
  ClonePair *tab = nullptr;
  MSC_HIP(ch->upload.begin(sizeof(ClonePair) * npairs, &tab));
  const msc_state *st0 = ch->states[0];
  uint32_t p = 0;
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t a = host_ancestors[c];
    if (a == c) continue;
    const msc_state *src = ch->states[a];
    msc_state *dst = ch->states[c];
    ClonePair &e = tab[p++];
    e.src_i64 = src->red_i64;
    e.dst_i64 = dst->red_i64;
    e.src_f64 = src->red_f64;
    e.dst_f64 = dst->red_f64;
    e.src_z = z_dev + (size_t)a * ld_z;
    e.dst_z = z_dev + (size_t)c * ld_z;
  }
  MSC_HIP(ch->upload.commit(s, ch->call_tab, sizeof(ClonePair) * npairs));
  if (launch_chains_clone(s, ch->table<ClonePair>(), npairs, st0->n_i64, st0->n_f64, nrows))
    return fail(MSC_EHIP, "k_chains_clone launch failed: %s", hipGetErrorString(hipGetLastError()));
  // a destination's additive tables were replaced as a whole and alone hold its truth now, as after an accumulate that
  // has not committed: the fields, the score constants and the CRP terms are rebuilt from them by the next call's ensure
  // steps.  (additive_rewritten(), msc_state_reduce_unpack's event, would not do: that call comes between an uncommitted
  // accumulate and a commit, so the fields are already marked stale there; a chain a sweep kept current has them marked
  // current, and they would stay the destination's old ones.)
  for (uint32_t c = 0; c < n; c++)
    if (host_ancestors[c] != c) ch->states[c]->valid.accumulated();
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// Split-merge proposals for every chain in one launch (k_sm_chains, kernels_chains_sm.hip): workgroup c makes the
// proposals of member c and keeps its tables current, as the sweep's kernel does.
// ---------------------------------------------------------------------------
// An upper estimate of one proposal of one chain, in microseconds: a fixed part (anchors, coins, decision, apply) plus
// launch_iters + 2 passes -- launch_iters + 1 of suff-stats, draws and labels, and the decision's suff-stats -- each a fixed
// part (barriers, the stick), a part per feature (a barrier, the slots' draws in double), a part per row (its label, the
// dart, the two-way softmax) and a part per (row, feature) (a row's value is read once for the sums and once for the
// scores), a row being the work of one of 256 threads.
// Fitted to profiles/chains_splitmerge.txt (one nich column and the C3 mix of 64 columns, 4 096 and 65 536 rows,
// launch_iters 0 / 2 / 5, 1 to 256 chains): what a pass adds there is at most 0.0163 us a row on one nich column and
// 0.605 us a row on the C3 mix, below 0.009 + 0.0095 D; the estimate is above the measured time per proposal at every
// shape of the table, by 19 % where it is closest.
constexpr double kSmFixedUs = 30.0, kSmPassUs = 25.0, kSmPassFeatUs = 3.0, kSmRowUs = 0.009, kSmRowFeatUs = 0.0095;
static double sm_proposal_us(uint64_t nrows, uint32_t nfeat, uint32_t launch_iters) {
  const double passes = (double)launch_iters + 2.0;
  return kSmFixedUs + passes * (kSmPassUs + kSmPassFeatUs * (double)nfeat + (kSmRowUs + kSmRowFeatUs * (double)nfeat) * (double)nrows);
}

extern "C" int msc_chains_split_merge(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t nrows,
                                      uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, uint32_t nproposals,
                                      uint32_t launch_iters, const uint64_t *host_seeds, uint64_t sweep, double *log_dev,
                                      int32_t *trace_dev, int32_t *proposed_dev, uint64_t *counters_dev) {
  MSC_REQUIRE(ch && view, "null argument");
  const uint32_t n = (uint32_t)ch->states.size();
  if (n == 0) return MSC_OK;
  MSC_REQUIRE((z_dev && host_seeds) || nproposals == 0, "null argument");
  MSC_REQUIRE(launch_iters <= 1024, "launch_iters %u beyond 1024", launch_iters);
  MSC_REQUIRE(nrows == view->nrows, "msc_chains_split_merge covers the whole view: nrows %llu, the view has %llu rows",
              (unsigned long long)nrows, (unsigned long long)view->nrows);
  MSC_REQUIRE(nrows < (1ull << 32), "msc_chains_split_merge takes at most 2^32 - 1 rows");
  MSC_REQUIRE(ld_z >= nrows, "msc_chains_split_merge: ld_z %llu < nrows %llu", (unsigned long long)ld_z,
              (unsigned long long)nrows);
  MSC_TRY(chains_refuse_mid_step(ch, "msc_chains_split_merge"));
  const msc_state *st0 = ch->states[0];
  MSC_TRY(sm_chain_route(ch->states[0]));                   // (equal feature lists: one answer for all)
  // a launch takes the whole proposals that fit the sweep's launch budget, by the estimate above times the rounds the grid
  // runs in (one workgroup a compute unit is what the estimate was measured at).  What is refused is a proposal that
  // alone exceeds the budget in ONE round: with more chains than compute units a launch of one proposal -- the least a
  // launch can take -- runs `rounds` such rounds, as msc_chains_sweep's launch of one visit does.
  const double one_us = sm_proposal_us(nrows, st0->nfeat, launch_iters);
  if (one_us > kSeqLaunchUs)
    return fail(MSC_EUNSUPPORTED, "msc_chains_split_merge: one proposal over %llu rows x %u features at launch_iters %u is "
                "estimated at %.0f us, beyond a launch's %.0f us: this kernel gives a chain one workgroup; "
                "msc_split_merge (State.split_merge) on each member has the row-parallel kernels for large tables",
                (unsigned long long)nrows, st0->nfeat, launch_iters, one_us, kSeqLaunchUs);
  if (nproposals == 0) return MSC_OK;
  // every table of every member current before, as msc_chains_sweep
  MSC_TRY(chains_enter(ch, "msc_chains_split_merge", ChainsEnsure::all_current, view, cols, 0, nrows));
  hipStream_t s = ch->ctx->stream;
  MSC_HIP(reserve_synced(s, ch->sm_ell, (size_t)n * std::max<uint64_t>(nrows, 1)));
  SmChain *tab = nullptr;
  MSC_HIP(ch->upload.begin(sizeof(SmChain) * n, &tab));
  for (uint32_t c = 0; c < n; c++) {
    msc_state *st = ch->states[c];
    SmChain &e = tab[c];
    MSC_TRY(sm_chain_pair(st, view, cols, nrows, &e));
    e.feats = st->desc_dev;
    e.cnt_acc = st->red_i64;
    e.cnt_u32 = st->cnt_u32;
    e.crp = st->logpc;
    e.z = z_dev + (size_t)c * ld_z;
    e.ell = ch->sm_ell.get() + (size_t)c * nrows;
    e.log = log_dev ? log_dev + (size_t)c * nproposals * 8 : nullptr;
    e.trace = trace_dev ? trace_dev + (size_t)c * nproposals * nrows : nullptr;
    e.proposed = proposed_dev ? proposed_dev + (size_t)c * nproposals * nrows : nullptr;
    e.counters = counters_dev ? reinterpret_cast<unsigned long long *>(counters_dev) + (size_t)c * 5 : nullptr;
    e.seed = host_seeds[c];
    e.alpha = st->alpha;
    e.pad = 0;
  }
  MSC_HIP(ch->upload.commit(s, ch->call_tab, sizeof(SmChain) * n));
  const uint32_t per_launch = (uint32_t)std::min<uint64_t>(nproposals, units_per_launch(n, ch->ctx->num_cus, one_us));
  const uint32_t pair_kpad = st0->sm.pair->kpad;
  for (uint32_t p0 = 0; p0 < nproposals; p0 += per_launch) {
    const uint32_t p1 = std::min(nproposals, p0 + per_launch);
    const int rc = launch_sm_chains(s, ch->table<SmChain>(), n, (int)st0->nfeat, st0->K, st0->kpad, pair_kpad, nrows, row_id0,
                                    p0, p1, launch_iters, sweep);
    if (rc == -2) return fail(MSC_EUNSUPPORTED, "k_sm_chains does not take this shape");
    if (rc) return fail(MSC_EHIP, "k_sm_chains launch failed: %s", hipGetErrorString(hipGetLastError()));
  }
  // the kernel kept every table of every member current (which also drops a blocked draw made before); a member's pair
  // state holds the last proposal's suff-stats, as after msc_split_merge's last commit
  for (msc_state *st : ch->states) {
    st->valid.kept_current();
    st->sm.pair->valid.accumulated();
    st->sm.pair->valid.committed();
  }
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// The slice step of every chain in one launch (k_hp_slice_chains), and the rebuild of what it made stale in another
// (k_chains_prepare): msc_hp_slice on every member, with one host synchronisation for the call.
// ---------------------------------------------------------------------------
extern "C" int msc_chains_hp_slice(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                                   uint64_t ld_slots, const uint64_t *host_seeds, uint64_t sweep, float *values_host,
                                   uint32_t *evals_host) {
  MSC_REQUIRE(ch && coords && host_seeds, "null argument");
  MSC_REQUIRE(n > 0, "no coordinates");
  const uint32_t nc = (uint32_t)ch->states.size();
  if (nc == 0) return MSC_OK;
  const msc_state *st0 = ch->states[0];
  MSC_REQUIRE(!slots_dev || ld_slots == 0 || ld_slots >= st0->K, "msc_chains_hp_slice: ld_slots %llu is neither 0 (one mask "
              "for all chains) nor >= ngroups %u", (unsigned long long)ld_slots, st0->K);
  MSC_TRY(chains_refuse_mid_step(ch, "msc_chains_hp_slice"));
  // msc_hp_slice's argument checks, once: the members' feature lists are equal (msc_chains_create)
  SlicePlan plan;
  MSC_TRY(slice_plan(st0, coords, n, plan));
  const uint32_t nt = plan.ntargets();
  MSC_TRY(chains_enter(ch, "msc_chains_hp_slice", ChainsEnsure::raw));
  uint32_t slices = 1;                                // (the count moves no bit: prepare_group deals whole rows out)
  for (const msc_state *st : ch->states) slices = std::max(slices, prepare_value_slices(st));
  // up, through the call table: chains | targets [nchains][nt] | entries; down: values | evals | status, [nchains][n] each
  const layout::HpBlocks lay = layout::hp_blocks(nc, nt, n, sizeof(HpChain), sizeof(SliceTarget), sizeof(SliceCoord));
  hipStream_t s = ch->ctx->stream;
  MSC_HIP(reserve_synced(s, ch->call_tab, lay.up_bytes));
  MSC_HIP(reserve_synced(s, ch->hp_out, lay.down_bytes));
  unsigned char *up = nullptr;
  MSC_HIP(ch->upload.begin(lay.up_bytes, &up));
  HpChain *hc = reinterpret_cast<HpChain *>(up + lay.chains);
  SliceTarget *tg = reinterpret_cast<SliceTarget *>(up + lay.targets);
  for (uint32_t c = 0; c < nc; c++) {
    const msc_state *st = ch->states[c];
    HpChain &e = hc[c];
    e.feats = st->desc_dev;
    e.cnt = st->cnt_u32;
    e.slots = slots_dev ? slots_dev + (size_t)c * ld_slots : nullptr;
    e.crp = st->logpc;
    e.key = host_seeds[c] ^ kSliceKey;
    e.alpha = st->alpha;
    e.pad = 0;
    slice_targets(st, plan, tg + (size_t)c * nt);
  }
  std::memcpy(up + lay.coords, plan.dc.data(), n * sizeof(SliceCoord));
  MSC_HIP(ch->upload.commit(s, ch->call_tab, lay.up_bytes));
  unsigned char *b = ch->call_tab, *o = ch->hp_out;
  if (launch_hp_slice_chains(s, reinterpret_cast<const SliceTarget *>(b + lay.targets), nt,
                             reinterpret_cast<HpChain *>(b + lay.chains), nc, reinterpret_cast<const SliceCoord *>(b + lay.coords),
                             n, st0->K, st0->kpad, sweep, reinterpret_cast<float *>(o + lay.values),
                             reinterpret_cast<uint32_t *>(o + lay.evals), reinterpret_cast<uint32_t *>(o + lay.status)))
    return fail(MSC_EHIP, "k_hp_slice_chains launch failed: %s", hipGetErrorString(hipGetLastError()));
  // every chain's score tables from its new hp blocks, its CRP table from its new alpha (which the step left in its entry)
  if (launch_chains_prepare(s, reinterpret_cast<const HpChain *>(b + lay.chains), nc, st0->nfeat, st0->K, st0->kpad, slices))
    return fail(MSC_EHIP, "k_chains_prepare launch failed: %s", hipGetErrorString(hipGetLastError()));
  ch->hp_down.resize(lay.down_bytes);
  MSC_HIP(hipMemcpyAsync(ch->hp_down.data(), o, lay.down_bytes, hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));                   // the call's one wait
  const float *val = reinterpret_cast<const float *>(ch->hp_down.data() + lay.values);
  const uint32_t *ev = reinterpret_cast<const uint32_t *>(ch->hp_down.data() + lay.evals);
  const uint32_t *stat = reinterpret_cast<const uint32_t *>(ch->hp_down.data() + lay.status);
  int rc = MSC_OK;
  // per member what msc_hp_slice's bookkeeping reports (hp_changed / alpha_changed for what moved), then what the second
  // launch rebuilt.  The first chain with a target that was not finite names the call's error.
  for (uint32_t c = nc; c-- > 0;) {
    msc_state *st = ch->states[c];
    const size_t at = (size_t)c * n;
    const int r = slice_installed(st, plan, coords, val + at, ev + at, stat + at, values_host ? values_host + at : nullptr,
                                  evals_host ? evals_host + at : nullptr, (int64_t)c);
    if (r != MSC_OK) rc = r;
    st->valid.prepared();
    st->valid.crp_prepared();
  }
  return rc;
}

// ---------------------------------------------------------------------------
// The log joint of every chain in one launch (k_chains_score_joint), and the best sample of every chain kept on the
// device (k_chains_keep_best).  Neither waits for the stream nor changes a state.
// ---------------------------------------------------------------------------
extern "C" int msc_chains_score_joint(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                                      uint64_t ld_slots, double *out_dev, uint64_t ld_out) {
  MSC_REQUIRE(ch, "null argument");
  const uint32_t nc = (uint32_t)ch->states.size();
  if (nc == 0) return MSC_OK;
  const msc_state *st0 = ch->states[0];
  const joint::JointCheck chk = joint::check_score_joint("msc_chains_score_joint", out_dev != nullptr, coords != nullptr, n,
                                                         st0->nfeat, ld_out, slots_dev != nullptr, ld_slots, st0->K);
  MSC_REQUIRE(chk.ok, "%s", chk.message);
  MSC_TRY(chains_refuse_mid_step(ch, "msc_chains_score_joint"));
  // the checks of the features and of the entries, once: the members' feature lists are equal (msc_chains_create)
  std::vector<JointCoord> entries;
  MSC_TRY(joint_entries(st0, "msc_chains_score_joint", coords, n, entries));
  MSC_TRY(chains_enter(ch, "msc_chains_score_joint", ChainsEnsure::raw));
  hipStream_t s = ch->ctx->stream;
  JointChain *tab = nullptr;
  MSC_HIP(ch->upload.begin(sizeof(JointChain) * nc, &tab));
  for (uint32_t c = 0; c < nc; c++) {
    const msc_state *st = ch->states[c];
    JointChain &e = tab[c];
    e.feats = st->desc_dev;
    e.cnt = st->cnt_u32;
    e.slots = slots_dev ? slots_dev + (size_t)c * ld_slots : nullptr;
    e.out = out_dev + (size_t)c * ld_out;
    e.alpha = st->alpha;
    e.pad = 0;
  }
  MSC_HIP(ch->upload.commit(s, ch->call_tab, sizeof(JointChain) * nc));
  if (launch_chains_score_joint(s, ch->table<JointChain>(), nc, st0->nfeat, st0->K, st0->kpad, entries.data(), n))
    return fail(MSC_EHIP, "k_chains_score_joint launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MSC_OK;
}

extern "C" int msc_chains_keep_best(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, const int32_t *z_dev,
                                    uint64_t ld_z, uint64_t nrows, uint64_t iter, double *best_dev, int32_t *best_z_dev,
                                    uint64_t ld_best, int64_t *best_iter_dev) {
  MSC_REQUIRE(ch, "null argument");
  const joint::JointCheck chk = joint::check_keep_best("msc_chains_keep_best", joint_dev && z_dev && best_dev && best_z_dev &&
                                                       best_iter_dev, ld_joint, nrows, ld_z, ld_best);
  MSC_REQUIRE(chk.ok, "%s", chk.message);
  MSC_REQUIRE(iter <= (uint64_t)INT64_MAX, "msc_chains_keep_best: iteration %llu does not fit best_iter's int64",
              (unsigned long long)iter);
  const uint32_t nc = (uint32_t)ch->states.size();
  if (nc == 0) return MSC_OK;
  MSC_TRY(chains_device(ch));
  if (launch_chains_keep_best(ch->ctx->stream, nc, joint_dev, ld_joint, z_dev, ld_z, nrows, (int64_t)iter, best_dev,
                              best_z_dev, ld_best, best_iter_dev))
    return fail(MSC_EHIP, "k_chains_keep_best launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// Between the sweeps of a tempered ensemble (kernels_temper.hip; the arithmetic and the checks: temper_math.hpp): the
// exchange of temperatures between neighbouring rungs of every ladder, and the weights of an annealing step.  Neither
// reads or changes a state, uploads a table or waits: one launch each on the arrays the caller holds.
// ---------------------------------------------------------------------------
extern "C" int msc_chains_exchange(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, uint32_t nrungs, float *beta_dev,
                                   int32_t *rung_dev, uint64_t parity, uint64_t seed, uint64_t sweep, uint32_t *proposed_dev,
                                   uint32_t *accepted_dev) {
  MSC_REQUIRE(ch, "null argument");
  const uint32_t nc = (uint32_t)ch->states.size();
  const uint32_t nfeat = nc ? ch->states[0]->nfeat : 0;
  const joint::JointCheck chk = temper::check_exchange("msc_chains_exchange", joint_dev && beta_dev && rung_dev && proposed_dev &&
                                                       accepted_dev, nrungs, nc, ld_joint, nfeat);
  MSC_REQUIRE(chk.ok, "%s", chk.message);
  if (nc == 0) return MSC_OK;
  MSC_TRY(chains_device(ch));
  // the kernel reports a broken ladder into the context's error word, whose device address travels as an argument
  void *err_dev = nullptr;
  MSC_HIP(hipHostGetDevicePointer(&err_dev, const_cast<uint32_t *>(ch->ctx->err_host), 0));
  if (launch_chains_exchange(ch->ctx->stream, nc, nfeat, joint_dev, ld_joint, nrungs, beta_dev, rung_dev, parity, seed, sweep,
                             proposed_dev, accepted_dev, static_cast<uint32_t *>(err_dev)))
    return fail(MSC_EHIP, "k_chains_exchange launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MSC_OK;
}

extern "C" int msc_chains_anneal_weights(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, const float *beta_from_dev,
                                         const float *beta_to_dev, double *logw_dev) {
  MSC_REQUIRE(ch, "null argument");
  const uint32_t nc = (uint32_t)ch->states.size();
  const uint32_t nfeat = nc ? ch->states[0]->nfeat : 0;
  const joint::JointCheck chk = temper::check_anneal_weights("msc_chains_anneal_weights", joint_dev && beta_from_dev &&
                                                             beta_to_dev && logw_dev, ld_joint, nfeat);
  MSC_REQUIRE(chk.ok, "%s", chk.message);
  if (nc == 0) return MSC_OK;
  MSC_TRY(chains_device(ch));
  if (launch_chains_anneal_weights(ch->ctx->stream, nc, nfeat, joint_dev, ld_joint, beta_from_dev, beta_to_dev, logw_dev))
    return fail(MSC_EHIP, "k_chains_anneal_weights launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// The posterior-averaged row predictive density over the chains (kernels_chains_marginal.hip)
// ---------------------------------------------------------------------------
// (How the chains are cut over the grid's second dimension, and the tile plan of a call: route_calls.hpp
// route_chains_marginal and plan_chains_marginal -- by the ensemble, the features and the view's rows, never the call's.)

// what msc_chains_score_marginal and msc_chains_sample_predictive check and bind before anything is launched
static int chains_marginal_begin(msc_chains *ch, const char *who, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                 uint64_t nrows) {
  const uint32_t n = (uint32_t)ch->states.size();
  const msc_state *st0 = ch->states[0];
  // where rows are scored, every member's score tables and CRP terms current, as msc_score_marginal
  MSC_TRY(chains_enter(ch, who, nrows ? ChainsEnsure::derived_crp : ChainsEnsure::none, view, cols, row0, nrows));
  // one tile plan serves every chain, so every member's exact count tables must have member 0's rows: they follow from
  // the view's column maxima and the member's own column bounds (msc_state_set_col_bounds), which may differ
  for (uint32_t c = 1; c < n; c++)
    for (uint32_t f = 0; f < st0->nfeat; f++) {
      const int fam = st0->feats[f].family;
      MSC_REQUIRE((fam != MSC_GP && fam != MSC_BNB) || ch->states[c]->desc_host[f].vcap == st0->desc_host[f].vcap,
                  "%s: feature %u: state %u's exact count table has %u rows, state 0's %u (their "
                  "column bounds differ: msc_state_set_col_bounds)", who, f, c, ch->states[c]->desc_host[f].vcap,
                  st0->desc_host[f].vcap);
    }
  return MSC_OK;
}

// The table of a call on the device, and what the first launch leaves beside it
struct MargCall {
  const MargChain *chains_dev = nullptr;
  const MargFeat *plan_dev = nullptr;
  void *const *outs_dev = nullptr;     // [nfeat], when the call gave outs
  CmPlan plan;
  uint32_t nsel = 0;
  double *lw = nullptr, *norm = nullptr;
};
// The table of this call through the call table -- the chains (chain c's row of chain_logp at logp + c * ld_logp), the
// selected features' tile plan (from member 0's facts as of its binding: families and dims are equal by
// msc_chains_create, the count columns' table sizes were compared by chains_marginal_begin), the output pointers of a
// sampling call -- and k_chains_marginal_prep's launch.
static int chains_marginal_stage(msc_chains *ch, const uint32_t *features, uint32_t nfeatures, const double *logw_dev,
                                 float *logp, uint64_t ld_logp, void *const *outs, MargCall &call) {
  const uint32_t n = (uint32_t)ch->states.size();
  const msc_state *st0 = ch->states[0];
  const bool all = features == nullptr || nfeatures == 0;
  hipStream_t s = ch->ctx->stream;
  const uint32_t nsel = all ? st0->nfeat : nfeatures;
  const layout::MargBlock blk = marg_block(ch, nsel);
  unsigned char *area = nullptr;
  MSC_HIP(ch->upload.begin(blk.bytes, &area));
  MargChain *tab = reinterpret_cast<MargChain *>(area + blk.chains);
  MargFeat *pf = reinterpret_cast<MargFeat *>(area + blk.feats);
  for (uint32_t c = 0; c < n; c++) {
    const msc_state *st = ch->states[c];
    MargChain &e = tab[c];
    e.feats = st->desc_dev;
    e.cnt = st->cnt_u32;
    e.crp = st->logpc;
    e.logp = logp ? logp + (size_t)c * ld_logp : nullptr;
    e.alpha = st->alpha;
    e.pad = 0;
  }
  std::vector<uint32_t> sel(nsel);
  for (uint32_t i = 0; i < nsel; i++) sel[i] = all ? i : features[i];
  call.plan = plan_chains_marginal(st0->route.feats.data(), sel.data(), nsel, st0->K, pf);
  call.nsel = nsel;
  unsigned char *dev = ch->call_tab;
  if (outs != nullptr) {
    std::memcpy(area + blk.outs, outs, (size_t)st0->nfeat * sizeof(void *));
    call.outs_dev = reinterpret_cast<void *const *>(dev + blk.outs);
  }
  MSC_HIP(ch->upload.commit(s, dev, outs ? blk.bytes : blk.outs));
  call.chains_dev = reinterpret_cast<const MargChain *>(dev + blk.chains);
  call.plan_dev = reinterpret_cast<const MargFeat *>(dev + blk.feats);
  call.lw = ch->marg_w;
  call.norm = call.lw + n;
  return launch_chains_marginal_prep(s, call.chains_dev, n, st0->K, logw_dev, call.lw, call.norm);
}

extern "C" int msc_chains_score_marginal(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                         uint64_t nrows, const uint32_t *features, uint32_t nfeatures, const double *logw_dev,
                                         uint32_t flags, float *mix_dev, float *chain_logp_dev, uint64_t ld_logp) {
  MSC_REQUIRE(ch && view, "null argument");
  MSC_REQUIRE(flags == 0, "unknown flags 0x%x", flags);
  MSC_REQUIRE(mix_dev || chain_logp_dev, "msc_chains_score_marginal: mix_dev and chain_logp_dev are both null");
  MSC_REQUIRE(!chain_logp_dev || ld_logp >= nrows, "msc_chains_score_marginal: ld_logp %llu < nrows %llu",
              (unsigned long long)ld_logp, (unsigned long long)nrows);
  MSC_REQUIRE(nrows < (1ull << 32), "msc_chains_score_marginal takes at most 2^32 - 1 rows per call");
  const uint32_t n = (uint32_t)ch->states.size();
  if (n == 0) return MSC_OK;
  const msc_state *st0 = ch->states[0];
  const bool all = features == nullptr || nfeatures == 0;
  if (!all)
    for (uint32_t i = 0; i < nfeatures; i++) {
      MSC_REQUIRE(features[i] < st0->nfeat, "msc_chains_score_marginal: feature %u outside the state (%u features)", features[i],
                  st0->nfeat);
      MSC_REQUIRE(i == 0 || features[i] > features[i - 1], "msc_chains_score_marginal: the feature list is not strictly "
                  "ascending at entry %u", i);
    }
  MSC_TRY(chains_marginal_begin(ch, "msc_chains_score_marginal", view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  const uint64_t view_rows = route_facts_now(ch->states[0]).view_rows;
  const uint32_t nslices = route_chains_marginal(n, view_rows, ch->ctx->num_cus);
  // the slices' workspace holds the whole VIEW's rows (what the slice count follows from): one size per view and device,
  // so calls over sub-ranges of any lengths never grow it again
  if (nslices > 1 && mix_dev)
    MSC_HIP(grow_retained(ch->retired, ch->marg_part, 2 * (size_t)nslices * std::max<uint64_t>(nrows, view_rows)));
  MargCall call;
  MSC_TRY(chains_marginal_stage(ch, features, nfeatures, logw_dev, chain_logp_dev, ld_logp, nullptr, call));
  return launch_chains_marginal(ch->ctx->stream, call.chains_dev, call.plan_dev, call.nsel, call.plan, n, nslices, st0->K,
                                st0->kpad, row0, nrows, call.lw, call.norm, mix_dev, ch->marg_part);
}

// ---------------------------------------------------------------------------
// Posterior predictive draws from the model average (kernels_chains_pred.hip)
// ---------------------------------------------------------------------------
// The rows of a call go through the handle's scratch -- the chains' rows Lf [nchains][chunk] floats, then the rows' chain
// and group -- a chunk at a time (route_calls.hpp pred_chunk).  A row depends on the row alone, so the cut moves no bit.

extern "C" int msc_chains_sample_predictive(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                            uint64_t nrows, uint64_t row_id0, const double *logw_dev, uint32_t flags,
                                            uint64_t seed, uint64_t sweep, int32_t *chain_out_dev, int32_t *z_out_dev,
                                            void *const *out_dev) {
  MSC_REQUIRE(ch && view && out_dev, "null argument");
  MSC_REQUIRE((flags & ~MSC_PRED_MASKED_ONLY) == 0, "unknown flags 0x%x", flags);
  MSC_REQUIRE(nrows < (1ull << 32), "msc_chains_sample_predictive takes at most 2^32 - 1 rows per call");
  const uint32_t n = (uint32_t)ch->states.size();
  if (n == 0) return MSC_OK;
  const msc_state *st0 = ch->states[0];
  bool light = false, heavy = false;
  for (uint32_t f = 0; f < st0->nfeat; f++) {
    if (out_dev[f] == nullptr) continue;
    const int fam = st0->feats[f].family;
    if (fam == MSC_NOOP) return fail(MSC_EUNSUPPORTED, "feature %u: the noop model has no values to draw", f);
    MSC_REQUIRE(f < 0x8000u, "feature %u: the draw's Philox counter holds feature indices below 32768", f);
    const bool h = fam == MSC_GP || fam == MSC_BNB || fam == MSC_NICH;
    heavy |= h;
    light |= !h || (flags & MSC_PRED_MASKED_ONLY) != 0;      // (the copies of observed entries are the light kernel's)
  }
  MSC_TRY(chains_marginal_begin(ch, "msc_chains_sample_predictive", view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  // the scratch: Lf, then chain and group of the chunk's rows (the caller's arrays where it gave them)
  const uint64_t chunk = pred_chunk(n, nrows);
  MSC_HIP(grow_retained(ch->retired, ch->pred_lf, (size_t)n * chunk));
  MSC_HIP(grow_retained(ch->retired, ch->pred_cz, 2 * (size_t)chunk));
  float *Lf = ch->pred_lf;
  MargCall call;
  MSC_TRY(chains_marginal_stage(ch, nullptr, 0, logw_dev, Lf, chunk, out_dev, call));
  hipStream_t s = ch->ctx->stream;
  // (the grid's cut only: with no mix, no slice writes a part)
  const uint32_t nslices = route_chains_marginal(n, route_facts_now(ch->states[0]).view_rows, ch->ctx->num_cus);
  const int batch = chains_draw_batch(st0->K, call.plan.large);
  for (uint64_t at = 0; at < nrows; at += chunk) {
    const uint64_t m = std::min<uint64_t>(chunk, nrows - at);
    int32_t *chain = chain_out_dev ? chain_out_dev + at : ch->pred_cz.get();
    int32_t *z = z_out_dev ? z_out_dev + at : ch->pred_cz.get() + chunk;
    MSC_TRY(launch_chains_marginal(s, call.chains_dev, call.plan_dev, call.nsel, call.plan, n, nslices, st0->K, st0->kpad,
                                   row0 + at, m, call.lw, call.norm, nullptr, nullptr));
    MSC_TRY(launch_chains_pick(s, call.lw, Lf, chunk, n, m, row_id0 + at, seed, sweep, chain));
    MSC_TRY(launch_chains_draw(s, call.chains_dev, call.plan.large, batch, st0->nfeat, st0->K, st0->kpad, row0 + at, m,
                               row_id0 + at, seed, sweep, chain, z));
    if (light || heavy)
      MSC_TRY(launch_chains_values(s, call.chains_dev, call.outs_dev, light, heavy, st0->nfeat, st0->kpad, row0 + at, m,
                                   row_id0 + at, at, chain, z, (flags & MSC_PRED_MASKED_ONLY) != 0, seed, sweep));
  }
  return MSC_OK;
}
