// summary.cpp -- summaries of posterior samples, none of which touches a state: the z-matrix accumulator with its
// partition losses and refinement (msc_zmatrix_*), single linkage (msc_linkage_single), distances between partitions
// (msc_partition_distances) and refinement under the exact expected VI (msc_vi_table, msc_partition_refine_vi).  Host
// logic only; of the core in abi.cpp it needs the device error check alone (abi_internal.hpp).
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "abi_internal.hpp"
#include "host_checks.hpp"
#include "launchers.hpp"
#include "linkage_host.hpp"

using namespace msc;

// A workspace of n elements that only direct calls use (reserve_synced): MSC_ENOMEM when the device has no room for it,
// MSC_EHIP for any other failure.  who: the entry point, what: the buffer, as the message names them.
template <typename T>
static int reserve_or_fail(hipStream_t stream, DevBuf<T> &buf, size_t n, const char *who, const char *what) {
  const hipError_t e = reserve_synced(stream, buf, n);
  if (e == hipSuccess) return MSC_OK;
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? MSC_ENOMEM : MSC_EHIP, "%s: the %s of %zu bytes: %s", who, what, n * sizeof(T),
              hipGetErrorString(e));
}

// host_order as require_permutation (host_checks.hpp) found it: MSC_EINVAL with its message unless it is one
static int permutation_ok(const PermutationCheck &c) { return c.ok ? MSC_OK : fail(MSC_EINVAL, "%s", c.message); }

// The two refinement loops launch every sweep without waiting for the stream -- up to kBlindSweeps of them; a caller who
// allows more pays one wait per kBlindSweeps further ones, so that the launches end when the starts have.  Before sweep
// `sweep` of a chunk of k starts: whether it should be launched -- always, except at such a wait, where the starts'
// running totals (st_dev) are fetched into st_host and the answer is whether any start is still active.
constexpr uint32_t kBlindSweeps = 64;
static int any_start_active(hipStream_t s, uint32_t sweep, const RefineStart *st_dev, uint32_t k,
                            std::vector<RefineStart> &st_host, bool *any) {
  *any = true;
  if (sweep < kBlindSweeps || sweep % kBlindSweeps != 0) return MSC_OK;
  st_host.resize(k);
  MSC_HIP(hipMemcpyAsync(st_host.data(), st_dev, (size_t)k * sizeof(RefineStart), hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));
  *any = false;
  for (uint32_t i = 0; i < k; i++) *any = *any || st_host[i].active != 0u;
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// z-matrix accumulator (microscopes.common.query.zmatrix; kernels_query.hip)
// ---------------------------------------------------------------------------
static size_t zm_count_words(uint32_t nt) { return (size_t)nt * (nt + 1) / 2 * kZmTile * kZmTile; }

// the buffer's allocation, MSC_ENOMEM (with the footprint) when the device has no room
static int zm_alloc(DevBuf<uint32_t> &buf, size_t bytes, const char *what, uint32_t m) {
  const hipError_t e = buf.alloc(bytes / 4);
  if (e == hipSuccess) return MSC_OK;
  (void)hipGetLastError();
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
    return fail(MSC_ENOMEM, "msc_zmatrix_create: m = %u needs %zu bytes for the %s (include/microscopes_hip.h gives the "
                "footprint); the device has no room", m, bytes, what);
  return fail(MSC_EHIP, "allocating the %s failed: %s", what, hipGetErrorString(e));
}

extern "C" int msc_zmatrix_create(msc_context *ctx, uint64_t n, const uint32_t *host_rows, uint32_t m, uint32_t nlabels,
                                  msc_zmatrix **out) {
  MSC_REQUIRE(ctx && out, "null argument");
  *out = nullptr;
  MSC_REQUIRE(n > 0, "msc_zmatrix_create: n is 0");
  MSC_REQUIRE(host_rows || (uint64_t)m == n, "msc_zmatrix_create: without rows m (%u) must equal n (%llu)", m,
              (unsigned long long)n);
  MSC_REQUIRE(m >= 1 && m <= kZmMaxRows, "msc_zmatrix_create: m = %u outside [1, %u]", m, kZmMaxRows);
  MSC_REQUIRE(nlabels >= 1 && nlabels <= kZmMaxLabels, "msc_zmatrix_create: nlabels = %u outside [1, %u]", nlabels,
              kZmMaxLabels);
  std::vector<uint32_t> rows(m);
  for (uint32_t a = 0; a < m; a++) {
    rows[a] = host_rows ? host_rows[a] : a;
    MSC_REQUIRE(rows[a] < n, "msc_zmatrix_create: rows[%u] = %u is not below n = %llu", a, rows[a], (unsigned long long)n);
  }
  MSC_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<msc_zmatrix> zm(new (std::nothrow) msc_zmatrix());
  if (!zm) return fail(MSC_ENOMEM, "out of host memory");
  zm->ctx = ctx;
  zm->n = n;
  zm->m = m;
  zm->nlabels = nlabels;
  zm->nt = (m + kZmTile - 1) / kZmTile;
  zm->wide = nlabels > 256;
  const size_t batch_bytes = (size_t)zm->nt * kZmTile * kZmBatchWords * 4;
  const size_t count_bytes = zm_count_words(zm->nt) * 4;
  MSC_TRY(zm_alloc(zm->counts, count_bytes, "counts", m));
  MSC_TRY(zm_alloc(zm->batch, batch_bytes, "sample batch", m));
  MSC_TRY(zm_alloc(zm->bad, (kZmBatchMax + 1) * 4, "batch flags", m));
  MSC_TRY(zm_alloc(zm->rows_dev, (size_t)m * 4, "rows", m));
  MSC_TRY(zm_alloc(zm->order_dev, (size_t)m * 4, "order", m));
  const hipStream_t s = ctx->stream;
  MSC_HIP(hipMemsetAsync(zm->counts, 0, count_bytes, s));
  MSC_HIP(hipMemsetAsync(zm->batch, 0, batch_bytes, s));
  MSC_HIP(hipMemsetAsync(zm->bad, 0, (kZmBatchMax + 1) * 4, s));
  MSC_HIP(hipMemcpyAsync(zm->rows_dev, rows.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
  MSC_HIP(hipStreamSynchronize(s));
  *out = zm.release();
  return MSC_OK;
}

// the staged samples into the counts, then an empty batch
static int zmatrix_flush(msc_zmatrix *zm) {
  if (zm->staged == 0) return MSC_OK;
  const hipStream_t s = zm->ctx->stream;
  if (launch_zm_count(s, zm->batch, zm->nt, zm->wide, zm->staged, zm->bad, zm->counts))
    return fail(MSC_EHIP, "k_zm_count launch failed");
  MSC_HIP(hipMemsetAsync(zm->batch, 0, (size_t)zm->nt * kZmTile * kZmBatchWords * 4, s));
  MSC_HIP(hipMemsetAsync(zm->bad, 0, (kZmBatchMax + 1) * 4, s));
  zm->staged = 0;
  return MSC_OK;
}

extern "C" int msc_zmatrix_add(msc_zmatrix *zm, const int32_t *z_dev, uint32_t nsamples, uint64_t ld) {
  MSC_REQUIRE(zm && z_dev, "null argument");
  MSC_REQUIRE(ld >= zm->n, "msc_zmatrix_add: ld = %llu is below n = %llu", (unsigned long long)ld,
              (unsigned long long)zm->n);
  MSC_TRY(device_error_check(zm->ctx));
  if (nsamples == 0) return MSC_OK;
  MSC_HIP(hipSetDevice(zm->ctx->device));
  const uint32_t cap = zm_batch_cap(zm->wide);
  for (uint32_t done = 0; done < nsamples;) {
    const uint32_t k = std::min(nsamples - done, cap - zm->staged);
    if (launch_zm_stage(zm->ctx->stream, z_dev + (uint64_t)done * ld, ld, k, zm->rows_dev, zm->m, zm->nlabels, zm->wide,
                        zm->staged, zm->bad, zm->batch))
      return fail(MSC_EHIP, "k_zm_check / k_zm_pack launch failed");
    zm->staged += k;
    zm->nsamples += k;
    done += k;
    if (zm->staged == cap) MSC_TRY(zmatrix_flush(zm));
  }
  return MSC_OK;
}

extern "C" int msc_zmatrix_nsamples(const msc_zmatrix *zm, uint64_t *out) {
  MSC_REQUIRE(zm && out, "null argument");
  *out = zm->nsamples;
  return MSC_OK;
}

static int zmatrix_write(msc_zmatrix *zm, const uint32_t *host_order, void *out_dev, uint64_t ld_out, bool norm) {
  MSC_REQUIRE(zm && out_dev, "null argument");
  MSC_REQUIRE(ld_out >= zm->m, "ld_out = %llu is below m = %u", (unsigned long long)ld_out, zm->m);
  MSC_REQUIRE(!norm || zm->nsamples > 0, "msc_zmatrix_result: no sample has been added (empty assignments list)");
  MSC_TRY(permutation_ok(require_permutation(host_order, zm->m, norm ? "msc_zmatrix_result" : "msc_zmatrix_counts")));
  MSC_TRY(device_error_check(zm->ctx));
  MSC_HIP(hipSetDevice(zm->ctx->device));
  MSC_TRY(zmatrix_flush(zm));
  const hipStream_t s = zm->ctx->stream;
  if (host_order) MSC_HIP(hipMemcpyAsync(zm->order_dev, host_order, (size_t)zm->m * 4, hipMemcpyHostToDevice, s));
  if (launch_zm_finish(s, zm->counts, zm->nt, zm->m, host_order ? zm->order_dev : nullptr, norm, (float)zm->nsamples,
                       out_dev, ld_out))
    return fail(MSC_EHIP, "k_zm_finish launch failed");
  return MSC_OK;
}

extern "C" int msc_zmatrix_counts(msc_zmatrix *zm, const uint32_t *host_order, uint32_t *out_dev, uint64_t ld_out) {
  return zmatrix_write(zm, host_order, out_dev, ld_out, false);
}

extern "C" int msc_zmatrix_result(msc_zmatrix *zm, const uint32_t *host_order, float *out_dev, uint64_t ld_out) {
  return zmatrix_write(zm, host_order, out_dev, ld_out, true);
}

// candidate partitions against the counts (kernels_partition.hip): the checks both entries share, the flush, and the
// label buffer of one chunk of candidates
static int zm_partition_begin(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t ncand, uint64_t ld, const char *who) {
  MSC_REQUIRE(zm && cand_dev, "null argument");
  MSC_REQUIRE(zm->nsamples > 0, "%s: no sample has been added", who);
  MSC_REQUIRE(ncand > 0, "%s: ncand is 0", who);
  MSC_REQUIRE(ld >= zm->n, "%s: ld = %llu is below n = %llu", who, (unsigned long long)ld, (unsigned long long)zm->n);
  MSC_TRY(device_error_check(zm->ctx));
  MSC_HIP(hipSetDevice(zm->ctx->device));
  MSC_TRY(zmatrix_flush(zm));
  return MSC_OK;
}

// w / size (either may be null) of candidates [0, k) at cand_dev into [k][m] arrays
static int zm_partition_chunk_sums(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t k, uint64_t ld, uint64_t *w_dev,
                                   uint32_t *size_dev) {
  const hipStream_t s = zm->ctx->stream;
  if (launch_zm_partition_gather(s, cand_dev, ld, k, zm->rows_dev, zm->m, zm->nt, zm->part_lab))
    return fail(MSC_EHIP, "k_zm_partition_gather launch failed");
  if (launch_zm_partition_sums(s, zm->counts, zm->nt, zm->m, zm->nsamples < kZmPartPackedMax, zm->part_lab, k, w_dev,
                               size_dev))
    return fail(MSC_EHIP, "k_zm_partition_sums launch failed");
  return MSC_OK;
}

extern "C" int msc_zmatrix_partition_sums(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t ncand, uint64_t ld,
                                          uint64_t *w_dev, uint32_t *size_dev) {
  const char *who = "msc_zmatrix_partition_sums";
  MSC_TRY(zm_partition_begin(zm, cand_dev, ncand, ld, who));
  if (!w_dev && !size_dev) return MSC_OK;
  const uint32_t chunk = zm_partition_chunk(zm->nt);
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->part_lab, (size_t)chunk * zm->nt * kZmTile, who, "label buffer"));
  for (uint32_t c0 = 0; c0 < ncand; c0 += chunk) {
    const size_t o = (size_t)c0 * zm->m;
    MSC_TRY(zm_partition_chunk_sums(zm, cand_dev + (uint64_t)c0 * ld, std::min(chunk, ncand - c0), ld,
                                    w_dev ? w_dev + o : nullptr, size_dev ? size_dev + o : nullptr));
  }
  return MSC_OK;
}

// binder_num <= V m (m - 1) / 2 must fit an int64
static int zm_partition_fits(const msc_zmatrix *zm, const char *who) {
  const unsigned __int128 pairs = (unsigned __int128)zm->m * (zm->m - 1) / 2;
  if (zm->nsamples > 0 && pairs * zm->nsamples >= ((unsigned __int128)1 << 63))
    return fail(MSC_EUNSUPPORTED, "%s: m (m - 1) / 2 x nsamples = %u (%u - 1) / 2 x %llu does not fit 63 bits", who, zm->m,
                zm->m, (unsigned long long)zm->nsamples);
  return MSC_OK;
}

// the loss workspaces of one chunk, and T (and V into valid_dev, nullable): the loss of all rows in one cluster
static int zm_partition_total(msc_zmatrix *zm, uint32_t chunk, uint64_t *valid_dev, const char *who) {
  const size_t mpad = (size_t)zm->nt * kZmTile;
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->part_lab, chunk * mpad, who, "label buffer"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->part_w, (size_t)chunk * zm->m, who, "workspace of row sums"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->part_size, (size_t)chunk * zm->m, who, "workspace of cluster sizes"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->part_T, 1, who, "pair total"));
  const hipStream_t s = zm->ctx->stream;
  MSC_HIP(hipMemsetAsync(zm->part_lab, 0, mpad * 4, s));
  if (launch_zm_partition_sums(s, zm->counts, zm->nt, zm->m, zm->nsamples < kZmPartPackedMax, zm->part_lab, 1,
                               zm->part_w, zm->part_size))
    return fail(MSC_EHIP, "k_zm_partition_sums launch failed");
  if (launch_zm_partition_loss(s, zm->counts, zm->part_w, zm->part_size, zm->m, 1, true, zm->part_T, nullptr, nullptr,
                               valid_dev))
    return fail(MSC_EHIP, "k_zm_partition_loss launch failed");
  return MSC_OK;
}

extern "C" int msc_zmatrix_partition_loss(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t ncand, uint64_t ld,
                                          int64_t *binder_num_dev, double *vi_lb_dev, uint64_t *valid_dev) {
  const char *who = "msc_zmatrix_partition_loss";
  MSC_REQUIRE(zm && cand_dev, "null argument");
  MSC_TRY(zm_partition_fits(zm, who));
  MSC_TRY(zm_partition_begin(zm, cand_dev, ncand, ld, who));
  if (!binder_num_dev && !vi_lb_dev && !valid_dev) return MSC_OK;
  const uint32_t chunk = zm_partition_chunk(zm->nt);
  MSC_TRY(zm_partition_total(zm, chunk, valid_dev, who));
  const hipStream_t s = zm->ctx->stream;
  if (!binder_num_dev && !vi_lb_dev) return MSC_OK;
  for (uint32_t c0 = 0; c0 < ncand; c0 += chunk) {
    const uint32_t k = std::min(chunk, ncand - c0);
    MSC_TRY(zm_partition_chunk_sums(zm, cand_dev + (uint64_t)c0 * ld, k, ld, zm->part_w, zm->part_size));
    if (launch_zm_partition_loss(s, zm->counts, zm->part_w, zm->part_size, zm->m, k, false, zm->part_T,
                                 binder_num_dev ? binder_num_dev + c0 : nullptr, vi_lb_dev ? vi_lb_dev + c0 : nullptr,
                                 nullptr))
      return fail(MSC_EHIP, "k_zm_partition_loss launch failed");
  }
  return MSC_OK;
}

// greedy row moves from given starts (kernels_refine.hip)
extern "C" int msc_zmatrix_partition_refine(msc_zmatrix *zm, const int32_t *start_dev, uint32_t nstarts, uint64_t ld,
                                            uint32_t max_sweeps, uint32_t max_clusters, const uint32_t *host_order,
                                            int32_t *labels_dev, int64_t *binder_num_dev, uint32_t *sweeps_dev,
                                            uint64_t *moves_dev) {
  const char *who = "msc_zmatrix_partition_refine";
  MSC_REQUIRE(zm && start_dev, "null argument");
  const uint32_t m = zm->m;
  MSC_REQUIRE(max_clusters >= 1 && max_clusters <= m, "%s: max_clusters = %u outside [1, m = %u]", who, max_clusters, m);
  MSC_TRY(permutation_ok(require_permutation(host_order, m, who)));
  MSC_REQUIRE(zm->nsamples > 0, "%s: no sample has been added", who);
  MSC_REQUIRE(nstarts > 0, "%s: nstarts is 0", who);
  MSC_REQUIRE(ld >= zm->n, "%s: ld = %llu is below n = %llu", who, (unsigned long long)ld, (unsigned long long)zm->n);
  if (m > kZmRefineMaxRows || max_clusters > kZmRefineMaxClusters)
    return fail(MSC_EUNSUPPORTED, "%s: m = %u, max_clusters = %u: at most %u positions and %u clusters", who, m,
                max_clusters, kZmRefineMaxRows, kZmRefineMaxClusters);
  MSC_TRY(zm_partition_fits(zm, who));
  MSC_TRY(zm_partition_begin(zm, start_dev, nstarts, ld, who));
  if (!labels_dev && !binder_num_dev && !sweeps_dev && !moves_dev) return MSC_OK;
  const uint32_t chunk = zm_partition_chunk(zm->nt);
  const uint64_t ldd = ((uint64_t)m + 3u) & ~(uint64_t)3u;
  const uint32_t mpad = zm->nt * kZmTile;
  MSC_TRY(zm_partition_total(zm, chunk, nullptr, who));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->ref_dense, (size_t)m * ldd, who, "dense copy of the counts"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->ref_ids, (size_t)chunk * ldd, who, "cluster ids"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->ref_st, chunk, who, "running totals"));
  MSC_TRY(reserve_or_fail(zm->ctx->stream, zm->ref_binder, chunk, who, "losses of the starts"));
  const hipStream_t s = zm->ctx->stream;
  if (host_order) MSC_HIP(hipMemcpyAsync(zm->order_dev, host_order, (size_t)m * 4, hipMemcpyHostToDevice, s));
  if (launch_zm_finish(s, zm->counts, zm->nt, m, nullptr, false, (float)zm->nsamples, zm->ref_dense, ldd))
    return fail(MSC_EHIP, "k_zm_finish launch failed");
  const bool narrow = zm->nsamples * (uint64_t)m < (1ull << 32);      // s_k <= V (m - 1), V <= nsamples
  std::vector<RefineStart> st_host;
  for (uint32_t c0 = 0; c0 < nstarts; c0 += chunk) {
    const uint32_t k = std::min(chunk, nstarts - c0);
    MSC_TRY(zm_partition_chunk_sums(zm, start_dev + (uint64_t)c0 * ld, k, ld, zm->part_w, zm->part_size));
    if (launch_zm_partition_loss(s, zm->counts, zm->part_w, zm->part_size, m, k, false, zm->part_T, zm->ref_binder, nullptr,
                                 nullptr))
      return fail(MSC_EHIP, "k_zm_partition_loss launch failed");
    if (launch_zm_refine_init(s, zm->part_lab, mpad, m, max_clusters, k, zm->ref_ids, ldd, zm->ref_st))
      return fail(MSC_EHIP, "k_zm_refine_init launch failed");
    for (uint32_t sweep = 0; sweep < max_sweeps; sweep++) {
      bool any = true;
      MSC_TRY(any_start_active(s, sweep, zm->ref_st, k, st_host, &any));
      if (!any) break;
      if (launch_zm_refine_sweep(s, zm->ref_dense, ldd, m, max_clusters, host_order ? zm->order_dev : nullptr, narrow, k,
                                 zm->ref_ids, zm->ref_st))
        return fail(MSC_EHIP, "k_zm_refine_sweep launch failed");
    }
    if (launch_zm_refine_finish(s, zm->ref_ids, ldd, m, max_clusters, k, zm->ref_st, zm->ref_binder,
                                labels_dev ? labels_dev + (uint64_t)c0 * m : nullptr,
                                binder_num_dev ? binder_num_dev + c0 : nullptr, sweeps_dev ? sweeps_dev + c0 : nullptr,
                                moves_dev ? moves_dev + c0 : nullptr))
      return fail(MSC_EHIP, "k_zm_refine_finish launch failed");
  }
  return MSC_OK;
}

extern "C" int msc_zmatrix_reset(msc_zmatrix *zm) {
  MSC_REQUIRE(zm, "null argument");
  MSC_HIP(hipSetDevice(zm->ctx->device));
  const hipStream_t s = zm->ctx->stream;
  MSC_HIP(hipMemsetAsync(zm->counts, 0, zm_count_words(zm->nt) * 4, s));
  MSC_HIP(hipMemsetAsync(zm->batch, 0, (size_t)zm->nt * kZmTile * kZmBatchWords * 4, s));
  MSC_HIP(hipMemsetAsync(zm->bad, 0, (kZmBatchMax + 1) * 4, s));
  zm->staged = 0;
  zm->nsamples = 0;
  return MSC_OK;
}

extern "C" int msc_zmatrix_destroy(msc_zmatrix *zm) {
  if (!zm) return MSC_OK;
  (void)hipSetDevice(zm->ctx->device);
  (void)hipStreamSynchronize(zm->ctx->stream);
  delete zm;
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// single linkage of a dense z-matrix (scipy.cluster.hierarchy.linkage of 1 - Z; kernels_linkage.hip, linkage_host.hpp)
// ---------------------------------------------------------------------------
extern "C" int msc_linkage_single(msc_context *ctx, const float *z_dev, uint64_t ld, uint32_t n, uint32_t flags,
                                  double *host_linkage, uint32_t *host_order) {
  MSC_REQUIRE(ctx && z_dev, "null argument");
  MSC_REQUIRE(flags == 0, "msc_linkage_single: flags = %u (none is defined)", flags);
  MSC_REQUIRE(n >= 2, "msc_linkage_single: n = %u (a linkage needs two points)", n);
  MSC_REQUIRE(ld >= n, "msc_linkage_single: ld = %llu is below n = %u", (unsigned long long)ld, n);
  if (n > linkage::kMaxN)
    return fail(MSC_EUNSUPPORTED, "msc_linkage_single: n = %u is above %u (one workgroup holds the chain's distances in "
                "registers)", n, linkage::kMaxN);
  MSC_TRY(device_error_check(ctx));
  MSC_HIP(hipSetDevice(ctx->device));
  const hipStream_t s = ctx->stream;
  const size_t nvals = 3 * (size_t)(n - 1);
  MSC_TRY(reserve_or_fail(s, ctx->linkage.edges, nvals, "msc_linkage_single", "edge list"));
  if (launch_linkage_prim(s, z_dev, ld, n, ctx->linkage.edges)) return fail(MSC_EHIP, "k_linkage_prim launch failed");
  std::vector<double> edges(nvals);
  MSC_HIP(hipMemcpyAsync(edges.data(), ctx->linkage.edges, nvals * sizeof(double), hipMemcpyDeviceToHost, s));
  MSC_HIP(hipStreamSynchronize(s));
  MSC_TRY(device_error_check(ctx));
  if (host_linkage || host_order) linkage::finish(edges.data(), n, host_linkage, host_order);
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// distances between partitions (kernels_distance.hip)
// ---------------------------------------------------------------------------
// which launches a block of partitions with cluster counts ka[0..na) x kb[0..nb) needs (route_pd_table decides per pair)
static void pd_block_routes(const uint32_t *ka, uint32_t na, const uint32_t *kb, uint32_t nb, bool *lds, bool *global) {
  uint32_t lo_a = kPdBad, hi_a = 0, lo_b = kPdBad, hi_b = 0;
  bool bad = false;
  for (uint32_t i = 0; i < na; i++)
    if (ka[i] == kPdBad) bad = true; else lo_a = std::min(lo_a, ka[i]), hi_a = std::max(hi_a, ka[i]);
  for (uint32_t j = 0; j < nb; j++)
    if (kb[j] == kPdBad) bad = true; else lo_b = std::min(lo_b, kb[j]), hi_b = std::max(hi_b, kb[j]);
  const bool any = hi_a != 0 && hi_b != 0;                  // a pair of two good partitions
  *lds = bad || (any && route_pd_table(lo_a, lo_b) == PdRoute::lds);
  *global = any && route_pd_table(hi_a, hi_b) == PdRoute::global;
}

extern "C" int msc_partition_distances(msc_context *ctx, const int32_t *a_dev, uint64_t lda, uint32_t na,
                                       const int32_t *b_dev, uint64_t ldb, uint32_t nb, uint32_t m, uint32_t flags,
                                       int64_t *pairs_ab_dev, double *nlogn_ab_dev, int64_t *pairs_a_dev,
                                       double *nlogn_a_dev, uint32_t *nclusters_a_dev, int64_t *pairs_b_dev,
                                       double *nlogn_b_dev, uint32_t *nclusters_b_dev) {
  const char *who = "msc_partition_distances";
  MSC_REQUIRE(ctx && a_dev, "%s: null argument", who);
  MSC_REQUIRE(flags == 0, "%s: flags = %u (none is defined)", who, flags);
  const bool mirror = b_dev == nullptr;
  if (mirror) b_dev = a_dev, ldb = lda, nb = na;
  MSC_REQUIRE(na > 0 && nb > 0 && m > 0, "%s: na = %u, nb = %u, m = %u: none may be 0", who, na, nb, m);
  MSC_REQUIRE(lda >= m && ldb >= m, "%s: lda = %llu, ldb = %llu below m = %u", who, (unsigned long long)lda,
              (unsigned long long)ldb, m);
  if (m > kPdMaxRows)
    return fail(MSC_EUNSUPPORTED, "%s: m = %u: at most %u rows (16-bit ids; up to %u clusters a partition)", who, m,
                kPdMaxRows, kPdMaxClusters);
  MSC_TRY(device_error_check(ctx));
  MSC_HIP(hipSetDevice(ctx->device));
  const hipStream_t s = ctx->stream;
  const uint64_t ldi = ((uint64_t)m + 3u) & ~(uint64_t)3u;
  MSC_TRY(reserve_or_fail(s, ctx->pd.ids, 2 * (size_t)kPdChunk * ldi, who, "cluster ids"));
  MSC_TRY(reserve_or_fail(s, ctx->pd.k, 2 * (size_t)kPdChunk, who, "cluster counts"));
  if (ctx->pd.log2_n < m || !ctx->pd.log2) {
    ctx->pd.log2_n = 0;
    MSC_TRY(reserve_or_fail(s, ctx->pd.log2, (size_t)m + 1, who, "table of log2 n"));
    if (launch_pd_log2(s, ctx->pd.log2, m)) return fail(MSC_EHIP, "k_pd_log2 launch failed");
    ctx->pd.log2_n = m;
  }
  uint16_t *ids_a = ctx->pd.ids, *ids_b = ids_a + (size_t)kPdChunk * ldi;
  uint32_t *k_a = ctx->pd.k, *k_b = k_a + kPdChunk;
  // the cluster counts come back to the host, a chunk at a time (one wait each): they say which launches a block needs
  std::vector<uint32_t> ka_host(kPdChunk), kb_host(nb);
  for (uint32_t a0 = 0; a0 < na; a0 += kPdChunk) {
    const uint32_t nac = std::min(kPdChunk, na - a0);
    if (launch_pd_canon(s, a_dev + (uint64_t)a0 * lda, lda, m, nac, ctx->pd.log2, a0, ids_a, ldi, k_a,
                        pairs_a_dev ? pairs_a_dev + a0 : nullptr, nlogn_a_dev ? nlogn_a_dev + a0 : nullptr,
                        nclusters_a_dev ? nclusters_a_dev + a0 : nullptr))
      return fail(MSC_EHIP, "k_pd_canon launch failed");
    MSC_HIP(hipMemcpyAsync(ka_host.data(), k_a, (size_t)nac * 4, hipMemcpyDeviceToHost, s));
    MSC_HIP(hipStreamSynchronize(s));
    for (uint32_t b0 = 0; b0 < nb; b0 += kPdChunk) {
      const uint32_t nbc = std::min(kPdChunk, nb - b0);
      const bool first = a0 == 0;                            // of this chunk of b: its own outputs are written now
      if (mirror && !first && b0 + nbc <= a0) continue;      // (every pair of the block is another block's mirror image)
      if (launch_pd_canon(s, b_dev + (uint64_t)b0 * ldb, ldb, m, nbc, ctx->pd.log2, b0, ids_b, ldi, k_b,
                          first && pairs_b_dev ? pairs_b_dev + b0 : nullptr,
                          first && nlogn_b_dev ? nlogn_b_dev + b0 : nullptr,
                          first && nclusters_b_dev ? nclusters_b_dev + b0 : nullptr))
        return fail(MSC_EHIP, "k_pd_canon launch failed");
      if (first) {
        MSC_HIP(hipMemcpyAsync(kb_host.data() + b0, k_b, (size_t)nbc * 4, hipMemcpyDeviceToHost, s));
        MSC_HIP(hipStreamSynchronize(s));
      }
      if (!pairs_ab_dev && !nlogn_ab_dev) continue;
      if (mirror && b0 + nbc <= a0) continue;
      bool lds = false, global = false;
      pd_block_routes(ka_host.data(), nac, kb_host.data() + b0, nbc, &lds, &global);
      PdPairArgs p;
      p.ids_a = ids_a, p.ids_b = ids_b, p.ldi = ldi, p.k_a = k_a, p.k_b = k_b;
      p.m = m, p.na = nac, p.nb = nbc, p.a0 = a0, p.b0 = b0, p.ldo = nb, p.mirror = mirror ? 1u : 0u;
      p.log2tab = ctx->pd.log2, p.table = nullptr, p.pairs_ab = pairs_ab_dev, p.nlogn_ab = nlogn_ab_dev;
      if (global) {
        if (!ctx->pd.table) {
          const size_t cells = (size_t)kPdSlices * kPdSliceCells;
          MSC_TRY(reserve_or_fail(s, ctx->pd.table, cells, who, "contingency tables"));
          MSC_HIP(hipMemsetAsync(ctx->pd.table, 0, cells * 4, s));
        }
        p.table = ctx->pd.table;
        if (launch_pd_pairs(s, ctx->num_cus, PdRoute::global, p)) return fail(MSC_EHIP, "k_pd_pairs launch failed");
      }
      if (lds && launch_pd_pairs(s, ctx->num_cus, PdRoute::lds, p)) return fail(MSC_EHIP, "k_pd_pairs launch failed");
    }
  }
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// greedy refinement under the exact expected variation of information (kernels_refine_vi.hip)
// ---------------------------------------------------------------------------
extern "C" int msc_vi_table(uint32_t m, int64_t *host_F) {
  MSC_REQUIRE(host_F != nullptr, "msc_vi_table: host_F is null");
  host_F[0] = 0;
  for (uint32_t n = 1; n <= m; n++) host_F[n] = (int64_t)std::rint((double)n * std::log2((double)n) * 16777216.0);
  return MSC_OK;
}

extern "C" int msc_partition_refine_vi(msc_context *ctx, const int32_t *samples_dev, uint64_t lds, uint32_t nsamples,
                                       uint32_t m, const int32_t *start_dev, uint64_t ld, uint32_t nstarts,
                                       uint32_t max_sweeps, uint32_t max_clusters, const uint32_t *host_order,
                                       size_t workspace_bytes, uint32_t flags, int32_t *labels_dev, int64_t *decrease_dev,
                                       uint32_t *sweeps_dev, uint64_t *moves_dev) {
  const char *who = "msc_partition_refine_vi";
  MSC_REQUIRE(ctx && samples_dev && start_dev, "%s: null argument", who);
  MSC_REQUIRE(flags == 0, "%s: flags = %u (none is defined)", who, flags);
  MSC_REQUIRE(nsamples > 0 && nstarts > 0 && m > 0, "%s: nsamples = %u, nstarts = %u, m = %u: none may be 0", who, nsamples,
              nstarts, m);
  MSC_REQUIRE(lds >= m && ld >= m, "%s: lds = %llu, ld = %llu below m = %u", who, (unsigned long long)lds,
              (unsigned long long)ld, m);
  MSC_REQUIRE(max_clusters >= 1 && max_clusters <= m, "%s: max_clusters = %u outside [1, m = %u]", who, max_clusters, m);
  MSC_TRY(permutation_ok(require_permutation(host_order, m, who)));
  if (m > kViMaxRows || nsamples > kViMaxSamples || max_clusters > kViMaxClusters)
    return fail(MSC_EUNSUPPORTED, "%s: m = %u, nsamples = %u, max_clusters = %u: at most %u rows, %u samples and %u clusters",
                who, m, nsamples, max_clusters, kViMaxRows, kViMaxSamples, kViMaxClusters);
  // the table, and the widths of everything made of it: |D| <= 3 S G_max and decrease <= 2 S F(m) stay under 2^62
  if (ctx->vi.G_m != m || ctx->vi.G_host.size() != m) {
    std::vector<int64_t> F((size_t)m + 1);
    MSC_TRY(msc_vi_table(m, F.data()));
    ctx->vi.G_m = 0;
    ctx->vi.G_host.resize(m);
    for (uint32_t n = 0; n < m; n++) ctx->vi.G_host[n] = F[n + 1] - F[n];
  }
  {
    const long double lim = 4611686018427387904.0L;                 // 2^62
    long double fm = 0.0L, gmax = 0.0L;
    for (uint32_t n = 0; n < m; n++) fm += (long double)ctx->vi.G_host[n], gmax = std::max(gmax, (long double)ctx->vi.G_host[n]);
    if (3.0L * nsamples * gmax >= lim || 2.0L * nsamples * fm >= lim)
      return fail(MSC_EUNSUPPORTED, "%s: nsamples = %u, m = %u: a gain or the decrease may pass 62 bits", who, nsamples, m);
  }
  MSC_TRY(device_error_check(ctx));
  MSC_HIP(hipSetDevice(ctx->device));
  if (!labels_dev && !decrease_dev && !sweeps_dev && !moves_dev) return MSC_OK;
  const hipStream_t s = ctx->stream;
  const uint64_t ldi = ((uint64_t)m + 3u) & ~(uint64_t)3u;
  const uint32_t S = nsamples, kcap = round_up(max_clusters, kViCellPad);
  const size_t budget = workspace_bytes ? workspace_bytes : (size_t)2 << 30;
  uint32_t chunk = std::min<uint32_t>(nstarts, 4096);
  uint64_t cells_per_start = 0;
  if (max_sweeps > 0) {
    // the samples: ids, cluster counts, their running sums and the rows' stretch indices.  The host waits once, for the
    // total of the cluster counts: it is what a start's cells, and so the chunk of starts, are sized by
    MSC_TRY(reserve_or_fail(s, ctx->vi.sample_ids, (size_t)S * ldi, who, "ids of the samples"));
    MSC_TRY(reserve_or_fail(s, ctx->vi.L, S, who, "cluster counts of the samples"));
    MSC_TRY(reserve_or_fail(s, ctx->vi.off, (size_t)S + 1, who, "running sums of the cluster counts"));
    MSC_TRY(reserve_or_fail(s, ctx->vi.row, (size_t)m * S, who, "stretch indices of the rows"));
    if (launch_vi_canon(s, samples_dev, lds, m, kViMaxClusters, S, 0, ctx->vi.sample_ids, ldi, ctx->vi.L, nullptr))
      return fail(MSC_EHIP, "k_vi_canon launch failed");
    if (launch_vi_rows(s, ctx->vi.sample_ids, ldi, ctx->vi.L, S, m, ctx->vi.off, ctx->vi.row))
      return fail(MSC_EHIP, "k_vi_offsets / k_vi_transpose launch failed");
    uint32_t stretches = 0;
    MSC_HIP(hipMemcpyAsync(&stretches, ctx->vi.off + S, 4, hipMemcpyDeviceToHost, s));
    MSC_HIP(hipStreamSynchronize(s));
    cells_per_start = (uint64_t)stretches * kcap;
    const uint64_t bytes = cells_per_start * 2u;
    if (bytes > budget)
      return fail(MSC_EUNSUPPORTED, "%s: the contingency cells of one start take %llu bytes (%u stretches of %u cells of 2 "
                  "bytes), workspace_bytes allows %zu", who, (unsigned long long)bytes, stretches, kcap, budget);
    chunk = (uint32_t)std::min<uint64_t>(chunk, budget / bytes);
    MSC_TRY(reserve_or_fail(s, ctx->vi.cells, (size_t)chunk * cells_per_start, who, "contingency cells"));
    if (!ctx->vi.G || ctx->vi.G_m != m) {
      ctx->vi.G_m = 0;
      MSC_TRY(reserve_or_fail(s, ctx->vi.G, m, who, "table of G"));
      MSC_HIP(hipMemcpyAsync(ctx->vi.G, ctx->vi.G_host.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
      MSC_HIP(hipStreamSynchronize(s));
      ctx->vi.G_m = m;
    }
    if (host_order) {
      MSC_TRY(reserve_or_fail(s, ctx->vi.order, m, who, "visiting order"));
      MSC_HIP(hipMemcpyAsync(ctx->vi.order, host_order, (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
  }
  MSC_TRY(reserve_or_fail(s, ctx->vi.ids, (size_t)chunk * ldi, who, "cluster ids"));
  MSC_TRY(reserve_or_fail(s, ctx->vi.st, chunk, who, "running totals"));
  ViSweepArgs p;
  p.row = ctx->vi.row, p.S = S, p.m = m, p.max_clusters = max_clusters, p.kcap = kcap;
  p.order = host_order ? ctx->vi.order.get() : nullptr, p.G = ctx->vi.G, p.ids = ctx->vi.ids, p.ldi = ldi;
  p.cells = ctx->vi.cells, p.cells_per_start = cells_per_start, p.st = ctx->vi.st;
  std::vector<RefineStart> st_host;
  for (uint32_t c0 = 0; c0 < nstarts; c0 += chunk) {
    const uint32_t k = std::min(chunk, nstarts - c0);
    if (launch_vi_canon(s, start_dev + (uint64_t)c0 * ld, ld, m, max_clusters, k, c0, ctx->vi.ids, ldi, nullptr, ctx->vi.st))
      return fail(MSC_EHIP, "k_vi_canon launch failed");
    if (max_sweeps > 0) {
      MSC_HIP(hipMemsetAsync(ctx->vi.cells, 0, (size_t)k * cells_per_start * 2u, s));
      if (launch_vi_count(s, ctx->num_cus, p, k)) return fail(MSC_EHIP, "k_vi_count launch failed");
    }
    for (uint32_t sweep = 0; sweep < max_sweeps; sweep++) {
      bool any = true;
      MSC_TRY(any_start_active(s, sweep, ctx->vi.st, k, st_host, &any));
      if (!any) break;
      if (launch_vi_sweep(s, p, k)) return fail(MSC_EHIP, "k_vi_sweep launch failed");
    }
    if (launch_vi_finish(s, ctx->vi.ids, ldi, m, max_clusters, k, ctx->vi.st,
                         labels_dev ? labels_dev + (uint64_t)c0 * m : nullptr, decrease_dev ? decrease_dev + c0 : nullptr,
                         sweeps_dev ? sweeps_dev + c0 : nullptr, moves_dev ? moves_dev + c0 : nullptr))
      return fail(MSC_EHIP, "k_vi_finish launch failed");
  }
  return MSC_OK;
}
