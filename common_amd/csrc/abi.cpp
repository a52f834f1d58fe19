// abi.cpp -- the core of the extern "C" surface declared in include/microscopes_hip.h: library and context, allocation,
// dataviews, the state with its plan (plan_groups runs the steps of tile_plan.hpp; bind_view), tables and ensure steps,
// the score, accumulate and sweep entries (they launch what the routes of route.hpp return), the reduce and column-bound
// entries, relations and msc_value_op_single.
// The subsystems built on it have a unit each -- blocked.cpp, chains.cpp, hyper.cpp, predict.cpp, summary.cpp -- and reach
// it through abi_internal.hpp.
// Host logic only: argument checking, table bookkeeping and kernel launches.
// There is deliberately no CPU arithmetic path here: every score / update is a
// kernel in kernels_*.hip, and context creation fails without a gfx950 device.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <new>

#include "abi_internal.hpp"
#include "launchers.hpp"
#include "row_range.hpp"
#include "tile_plan.hpp"

namespace msc {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
}
int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

size_t primitive_size(int t) {
  static const size_t sz[MSC_TYPE_NELEMS] = {1, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
  return (t >= 0 && t < MSC_TYPE_NELEMS) ? sz[t] : 0;
}

static bool family_ok(int f) { return f >= MSC_BB && f <= MSC_DM; }

}  // namespace msc

using namespace msc;

// ---------------------------------------------------------------------------
// library / context
// ---------------------------------------------------------------------------
extern "C" int msc_abi_version(void) { return MSC_ABI_VERSION; }
extern "C" const char *msc_last_kernel(int which) { return msc::last_kernel(which); }
extern "C" const char *msc_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *msc_build_info(void) {
  return "microscopes_hip abi " "1" " gfx950 (CDNA4) hipcc " __VERSION__;
}

// ---- device-side errors (device_error.hpp) ----------------------------------------------------------------------------
// One pinned pair of words per device, bound into every kernel translation unit the first time a context is created on
// the device; it lives as long as the library.
static int device_error_word(int device, volatile uint32_t **host_out) {
  static std::mutex mu;
  static uint32_t *words[64] = {};
  MSC_REQUIRE(device >= 0 && device < 64, "device %d: at most 64 devices", device);
  std::lock_guard<std::mutex> lock(mu);
  if (!words[device]) {
    uint32_t *h = nullptr;
    void *d = nullptr;
    MSC_HIP(hipHostMalloc(reinterpret_cast<void **>(&h), 64, hipHostMallocMapped));
    h[0] = h[1] = 0;
    MSC_HIP(hipHostGetDevicePointer(&d, h, 0));
    uint32_t *w = static_cast<uint32_t *>(d);
    if (bind_error_word_score(w) || bind_error_word_sweep(w) || bind_error_word_state(w) || bind_error_word_seq(w) ||
        bind_error_word_query(w) || bind_error_word_refine(w) || bind_error_word_distance(w) ||
        bind_error_word_refine_vi(w))
      return fail(MSC_EHIP, "binding the device error word failed: %s", hipGetErrorString(hipGetLastError()));
    words[device] = h;
  }
  *host_out = words[device];
  return MSC_OK;
}
// what the launching and synchronising entry points call first / last: an error a kernel of an earlier call reported
int msc::device_error_check(msc_context *ctx) {
  volatile uint32_t *w = ctx ? ctx->err_host : nullptr;
  if (!w || w[0] == 0) return MSC_OK;
  std::atomic_thread_fence(std::memory_order_acquire);
  const uint32_t code = w[0], detail = w[1];
  w[0] = 0;
  // (code bits: every kind that was reported since the last check is named; `detail` belongs to the first)
  std::string what;
  auto add = [&](const char *t) { if (!what.empty()) what += "; "; what += t; };
  if (code & 1u) add("a wave-subset barrier of a tile kernel timed out (detail: workgroup): rows of that launch are wrong");
  if (code & 2u) add("msc_entity_op: leave from a group the row is not in / an empty group, or join of an assigned row (detail: group)");
  if (code & 4u) add("msc_relation_slice_scores: a block offset beyond the score row (detail: cell)");
  if (code & 8u) add("msc_sweep_sequential: an order entry >= nrows (visit skipped; detail: entry), or a leave from an empty group or counter (detail: group)");
  if (code & 16u) add("msc_zmatrix_add: a label outside [0, nlabels) (that sample was skipped; detail: row of z)");
  if (code & 32u) add("msc_zmatrix_partition_refine: a start with more than max_clusters clusters (its outputs mean nothing; detail: start of its chunk)");
  if (code & 64u) add("msc_partition_distances: a partition with more than 1024 clusters (every output it takes part in is -1 or NaN; detail: its index in its set)");
  if (code & 128u) add("msc_partition_refine_vi: a sample with more than 1024 clusters or a start with more than max_clusters (its outputs mean nothing; detail: its index)");
  if (code & 256u) add("msc_chains_exchange: rungs that are no permutation within a ladder (it was left as it was; detail: ladder)");
  if (code & 512u) add("msc_chains_sweep_tempered: a chain's temperature is NaN, negative or infinite (the chain made no visit; detail: chain)");
  if (code & ~1023u) add("unknown device-side error");
  return fail(MSC_EDEVICE, "reported by an earlier kernel on device %d: %s [detail of the first: %u]; rebuild the affected state's tables",
              ctx->device, what.c_str(), detail);
}

extern "C" int msc_context_create(int device, void *stream, msc_context **out) {
  MSC_REQUIRE(out != nullptr, "msc_context_create: out is null");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(MSC_ENODEVICE, "no HIP device visible (%s); this library has no CPU path",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  MSC_REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
  hipDeviceProp_t prop;
  MSC_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MSC_ENODEVICE, "device %d is %s; kernels are built for gfx950 only", device,
                prop.gcnArchName);
  MSC_HIP(hipSetDevice(device));
  std::unique_ptr<msc_context> ctx(new (std::nothrow) msc_context());
  if (!ctx) return fail(MSC_ENOMEM, "out of host memory");
  ctx->device = device;
  ctx->stream = static_cast<hipStream_t>(stream);
  ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  MSC_HIP(ctx->mailbox_host.alloc(192 * 1024));   // niw at dim 128: a 66 KB record + a 66 KB hp block
  MSC_HIP(hipHostGetDevicePointer(&ctx->mailbox_dev, ctx->mailbox_host, 0));
  if (ctx->sync_word_host.alloc(16) == hipSuccess) {   // (64 bytes)
    *ctx->sync_word_host = 0;
    if (hipHostGetDevicePointer(&ctx->sync_word_dev, ctx->sync_word_host, 0) != hipSuccess) ctx->sync_word_ok = false;
  } else {
    (void)hipGetLastError();
  }
  MSC_TRY(device_error_word(device, &ctx->err_host));
  *out = ctx.release();
  return MSC_OK;
}

static void vmm_free(msc_context::VmmAlloc &a);

extern "C" int msc_context_destroy(msc_context *ctx) {
  if (!ctx) return MSC_OK;
  (void)hipSetDevice(ctx->device);
  for (auto &a : ctx->vmm) vmm_free(a);
  ctx->vmm.clear();
  if (ctx->record_stream) (void)hipStreamDestroy(ctx->record_stream);
  delete ctx;
  return MSC_OK;
}

extern "C" int msc_context_set_stream(msc_context *ctx, void *stream) {
  MSC_REQUIRE(ctx, "null context");
  ctx->stream = static_cast<hipStream_t>(stream);
  return MSC_OK;
}

extern "C" int msc_context_synchronize(msc_context *ctx) {
  MSC_REQUIRE(ctx, "null context");
  // The per-entity paths (hip::mixture_state: remove, score, add) wait here once per move, for kernels that take a few
  // microseconds: waking up from hipStreamSynchronize costs as much again.  So the stream writes a sequence number
  // into a pinned word when it gets here and the host watches the word; bounded, the stream wait is the fallback.
  if (ctx->sync_word_host && ctx->sync_word_ok) {
    const uint32_t seq = ++ctx->sync_seq;
    if (hipStreamWriteValue32(ctx->stream, ctx->sync_word_dev, seq, 0) == hipSuccess) {
      volatile uint32_t *w = ctx->sync_word_host;
      for (int spin = 0; spin < 400000; spin++)
        if (*w == seq) {
          std::atomic_thread_fence(std::memory_order_acquire);
          return device_error_check(ctx);
        }
    } else {
      (void)hipGetLastError();
      ctx->sync_word_ok = false;
    }
  }
  MSC_HIP(hipStreamSynchronize(ctx->stream));
  return device_error_check(ctx);
}

// One candidate of msc_device_alloc_probed: nbytes of device memory mapped from 32 MiB physical chunks that are created
// one by one (hipMemCreate) and mapped side by side into one reserved VA range.  Measured
// (tools/microbench/placement_stitch.hip, four rounds): such buffers take the C2 store stream at 6.2-7.0 TB/s where
// hipMalloc'ed ones of the same process take it at 5.3-6.2 -- whatever the chunk size (2 / 32 / 256 MiB) and mapping
// order.  Returns false (nothing allocated) when the virtual-memory API is not usable.
static bool vmm_alloc(int device, size_t nbytes, msc_context::VmmAlloc *out) {
  const size_t chunk = 32u << 20;
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0 || chunk % gran != 0) {
    (void)hipGetLastError();
    return false;
  }
  msc_context::VmmAlloc a;
  const size_t n = (std::max<size_t>(nbytes, 1) + chunk - 1) / chunk;
  a.size = n * chunk;
  a.va = nullptr;
  if (hipMemAddressReserve(&a.va, a.size, 2u << 20, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  bool ok = true;
  size_t mapped = 0;
  for (size_t i = 0; i < n && ok; i++) {
    hipMemGenericAllocationHandle_t h;
    if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) { ok = false; break; }
    a.handles.push_back(h);
    if (hipMemMap(static_cast<char *>(a.va) + i * chunk, chunk, 0, h, 0) != hipSuccess) { ok = false; break; }
    mapped = i + 1;
  }
  if (ok) {
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    ok = hipMemSetAccess(a.va, a.size, &acc, 1) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    if (mapped) (void)hipMemUnmap(a.va, mapped * chunk);
    for (auto h : a.handles) (void)hipMemRelease(h);
    (void)hipMemAddressFree(a.va, a.size);
    return false;
  }
  *out = a;
  return true;
}
static void vmm_free(msc_context::VmmAlloc &a) {
  (void)hipMemUnmap(a.va, a.size);
  for (auto h : a.handles) (void)hipMemRelease(h);
  (void)hipMemAddressFree(a.va, a.size);
  a.handles.clear();
  a.va = nullptr;
}

// Large buffers (from 64 MiB on: score matrices) are PLACED: the same store stream runs 5.5 or 7.0 TB/s depending on where
// the driver put the pages (profiles/r02_placement_study.txt), no allocator argument selects that, and buffers mapped
// from separately created 32 MiB chunks land in the upper band more often than hipMalloc'ed ones.  So a candidate is
// mapped from chunks, stream-filled a few times with the score kernels' store pattern, and kept when it takes the stream
// at `accept_gbps` or better; otherwise the next candidate is tried while the rejected ones are still held (released
// first, the driver would hand the same pages back), and the fastest wins.  Three things end the search early:
//   * `max_candidates` (msc_device_alloc: 12);
//   * the candidates held side by side would exceed HALF of what the device had free when the call began (the transient
//     footprint is the caller's memory too: torch's caching allocator, other tenants);
//   * a FLAT box: after `flat_after` candidates whose fill rates lie within 6 % of each other and below the mark there is
//     no fast stretch to find here (the round-3 driver's box: 24 of 24 at 5.40-5.67 TB/s) -- stop, keep the best.
// Per-chunk selection was tried and does not work: a chunk's rate inside a fill follows its position in the launch, not
// the chunk (tools/microbench/placement_chunks.hip, profiles/r03_placement_chunks.txt).  Synchronous (about 1 ms per
// candidate and GB).
static int alloc_placed(msc_context *ctx, size_t nbytes, uint32_t max_candidates, float accept_gbps, uint32_t flat_after,
                        void **out, float *rates_gbps, uint32_t *chosen) {
  struct Cand { void *p; bool vmm; msc_context::VmmAlloc v; };
  std::vector<Cand> bufs;
  std::vector<float> rate;
  auto release = [&](int keep) {
    for (size_t i = 0; i < bufs.size(); i++) {
      if ((int)i == keep) continue;
      if (bufs[i].vmm) vmm_free(bufs[i].v);
      else (void)hipFree(bufs[i].p);
    }
  };
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(MSC_EHIP, "hipEventCreate failed");
  int rc = MSC_OK;
  const int reps = nbytes >= (256u << 20) ? 5 : 8;
  const bool want_vmm = nbytes >= (64u << 20);                      // small buffers: not worth 32 MiB chunks
  size_t free_at_start = 0;
  {
    size_t total_b = 0;
    if (hipMemGetInfo(&free_at_start, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      free_at_start = 0;
    }
  }
  for (uint32_t i = 0; i < max_candidates; i++) {
    if (i > 0) {                                                               // never take the device's last memory for a probe,
      size_t free_b = 0, total_b = 0;                                          // nor more than half of what was free for all of them
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 2 * nbytes + (1ull << 30) ||
          (flat_after != 0 && (size_t)(i + 1) * nbytes > free_at_start / 2)) {
        (void)hipGetLastError();
        break;
      }
      if (flat_after != 0 && i >= flat_after && rate.size() == i) {            // a flat box: nothing to find
        const float hi = *std::max_element(rate.begin(), rate.end()), lo = *std::min_element(rate.begin(), rate.end());
        if (hi > 0.f && (hi - lo) <= 0.06f * hi) break;
      }
    }
    Cand c{nullptr, false, {}};
    if (want_vmm && vmm_alloc(ctx->device, nbytes, &c.v)) {
      c.p = c.v.va;
      c.vmm = true;
    } else if (hipMalloc(&c.p, nbytes ? nbytes : 1) != hipSuccess) {           // out of memory: settle for what there is
      (void)hipGetLastError();
      break;
    }
    bufs.push_back(c);
    void *p = c.p;
    hipError_t e = hipMemsetAsync(p, 0, nbytes ? nbytes : 1, ctx->stream);          // (zero-filled, like every msc_device_alloc)
    if (max_candidates > 1) {
      if (e == hipSuccess && launch_stream_fill(ctx->stream, ctx->num_cus, p, nbytes)) e = hipErrorLaunchFailure;
      if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
      for (int r = 0; r < reps && e == hipSuccess; r++)
        if (launch_stream_fill(ctx->stream, ctx->num_cus, p, nbytes)) e = hipErrorLaunchFailure;
      if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
      if (e == hipSuccess) e = hipEventSynchronize(e1);
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (e != hipSuccess) { rc = fail(MSC_EHIP, "placement probe failed: %s", hipGetErrorString(e)); break; }
      rate.push_back(ms > 0.f ? (float)((double)nbytes * reps / (ms * 1e-3) / 1e9) : 0.f);
      if (rate.back() >= accept_gbps) break;
    } else {
      if (e != hipSuccess) { rc = fail(MSC_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e)); break; }
      rate.push_back(0.f);
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != MSC_OK || bufs.empty() || rate.size() != bufs.size()) {
    (void)hipStreamSynchronize(ctx->stream);
    release(-1);
    return rc != MSC_OK ? rc : fail(MSC_ENOMEM, "allocation of %zu bytes failed", nbytes);
  }
  int best = 0;
  for (size_t i = 1; i < rate.size(); i++)
    if (rate[i] > rate[best]) best = (int)i;
  if (bufs.size() > 1) (void)hipStreamSynchronize(ctx->stream);
  release(best);
  if (bufs[best].vmm) ctx->vmm.push_back(bufs[best].v);
  ctx->last_alloc_rates = rate;
  ctx->last_alloc_chosen = (uint32_t)best;
  // (the stores' mark follows the accept mark when a caller lowers that one -- MSC_ALLOC_ACCEPT_GBPS: the evidence runs of
  // tools/profile_round.sh trace the non-temporal instantiation on boxes without a fast stretch that way)
  ctx->placed.push_back(msc_context::Placed{bufs[best].p, nbytes, max_candidates > 1 && rate[best] >= std::min(kNtFastGbps, accept_gbps)});
  if (rates_gbps)
    for (uint32_t i = 0; i < max_candidates; i++) rates_gbps[i] = i < rate.size() ? rate[i] : 0.f;
  if (chosen) *chosen = (uint32_t)best;
  *out = bufs[best].p;
  return MSC_OK;
}

// device buffers for callers that hold no HIP headers of their own (the assignment vector, score rows, score matrices)
extern "C" int msc_device_alloc(msc_context *ctx, size_t nbytes, void **out) {
  MSC_REQUIRE(ctx && out, "null argument");
  *out = nullptr;
  MSC_HIP(hipSetDevice(ctx->device));
  // MSC_ALLOC_CANDIDATES (default 12; 1 = no probing, 0 = plain hipMalloc) / MSC_ALLOC_ACCEPT_GBPS (default 6650: a
  // candidate that fills at 6.7 TB/s takes the C2 pass at 0.87-0.88 of the HBM roof, one at 6.5 at 0.83-0.87, one at 6.2
  // at 0.80-0.83; when none reaches the mark the best of all is kept, ~1 ms a candidate and GB); after six candidates
  // whose rates all lie within 6 % the box is taken to have no fast stretch.
  // Candidates held side by side walk through physical memory, and where the fast stretches lie differs from box to
  // box: one box offered one within six candidates in ten processes of ten, another none within twelve in one process
  // of twelve (profiles/r03_alloc_distribution.jsonl), the round-3 driver's none within 24
  const Switches sw = read_switches();
  constexpr int flat = 6;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(ctx->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
  if (nbytes >= (64u << 20) && sw.alloc_candidates >= 1 && !capturing)
    return alloc_placed(ctx, nbytes, (uint32_t)std::min(sw.alloc_candidates, 64), sw.alloc_accept_gbps, (uint32_t)std::max(flat, 2), out, nullptr, nullptr);
  void *p = nullptr;
  MSC_HIP(hipMalloc(&p, nbytes ? nbytes : 1));
  const hipError_t e = hipMemsetAsync(p, 0, nbytes ? nbytes : 1, ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return fail(MSC_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
  }
  *out = p;
  return MSC_OK;
}

extern "C" int msc_device_alloc_probed(msc_context *ctx, size_t nbytes, uint32_t candidates, void **out,
                                       float *rates_gbps, uint32_t *chosen) {
  MSC_REQUIRE(ctx && out, "null argument");
  MSC_REQUIRE(candidates >= 1 && candidates <= 64, "candidates %u outside 1..64", candidates);
  *out = nullptr;
  MSC_HIP(hipSetDevice(ctx->device));
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ctx->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(MSC_EINVAL, "msc_device_alloc_probed waits for the device: not on a capturing stream");
  return alloc_placed(ctx, nbytes, candidates, 1e30f, 0u, out, rates_gbps, chosen);     // every candidate is probed, the best kept
}
extern "C" int msc_device_alloc_stats(msc_context *ctx, float *rates_gbps, uint32_t capacity, uint32_t *ntried, uint32_t *chosen) {
  MSC_REQUIRE(ctx, "null context");
  const uint32_t n = (uint32_t)ctx->last_alloc_rates.size();
  if (rates_gbps)
    for (uint32_t i = 0; i < capacity && i < n; i++) rates_gbps[i] = ctx->last_alloc_rates[i];
  if (ntried) *ntried = n;
  if (chosen) *chosen = ctx->last_alloc_chosen;
  return MSC_OK;
}
extern "C" int msc_device_free(msc_context *ctx, void *dev) {
  MSC_REQUIRE(ctx, "null context");
  if (!dev) return MSC_OK;
  MSC_HIP(hipSetDevice(ctx->device));
  MSC_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ctx->placed.size(); i++)
    if (ctx->placed[i].base == dev) {
      ctx->placed.erase(ctx->placed.begin() + i);
      break;
    }
  for (size_t i = 0; i < ctx->vmm.size(); i++)
    if (ctx->vmm[i].va == dev) {                          // a probed buffer mapped from chunks
      vmm_free(ctx->vmm[i]);
      ctx->vmm.erase(ctx->vmm.begin() + i);
      return MSC_OK;
    }
  MSC_HIP(hipFree(dev));
  return MSC_OK;
}
extern "C" int msc_pinned_alloc(msc_context *ctx, size_t nbytes, void **host, void **dev) {
  MSC_REQUIRE(ctx && host && dev, "null argument");
  *host = *dev = nullptr;
  MSC_HIP(hipSetDevice(ctx->device));
  void *h = nullptr, *d = nullptr;
  MSC_HIP(hipHostMalloc(&h, nbytes ? nbytes : 1, hipHostMallocMapped));
  const hipError_t e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(h);
    return fail(MSC_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
  }
  std::memset(h, 0, nbytes ? nbytes : 1);
  *host = h;
  *dev = d;
  return MSC_OK;
}
extern "C" int msc_pinned_free(msc_context *ctx, void *host) {
  MSC_REQUIRE(ctx, "null context");
  if (!host) return MSC_OK;
  MSC_HIP(hipSetDevice(ctx->device));
  MSC_HIP(hipStreamSynchronize(ctx->stream));
  MSC_HIP(hipHostFree(host));
  return MSC_OK;
}
// both copies are ordered on the context's stream and have completed when the call returns
extern "C" int msc_device_upload(msc_context *ctx, void *dst_dev, const void *src_host, size_t nbytes) {
  MSC_REQUIRE(ctx && (nbytes == 0 || (dst_dev && src_host)), "null argument");
  if (nbytes == 0) return MSC_OK;
  MSC_HIP(hipSetDevice(ctx->device));
  MSC_HIP(hipMemcpyAsync(dst_dev, src_host, nbytes, hipMemcpyHostToDevice, ctx->stream));
  MSC_HIP(hipStreamSynchronize(ctx->stream));
  return MSC_OK;
}
extern "C" int msc_device_download(msc_context *ctx, void *dst_host, const void *src_dev, size_t nbytes) {
  MSC_REQUIRE(ctx && (nbytes == 0 || (dst_host && src_dev)), "null argument");
  if (nbytes == 0) return MSC_OK;
  MSC_HIP(hipSetDevice(ctx->device));
  MSC_HIP(hipMemcpyAsync(dst_host, src_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
  MSC_HIP(hipStreamSynchronize(ctx->stream));
  return device_error_check(ctx);
}

// ---------------------------------------------------------------------------
// dataview
// ---------------------------------------------------------------------------
static uint64_t next_view_serial() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}
// The serials of the views that exist.  A state remembers the view it last bound by pointer AND serial and keeps no
// reference to it (the reference's dataviews are borrowed the same way, recarray/_dataview.pxd:24-27); before it looks at
// that view again outside a call that was handed one -- msc_state_set_hp re-plans, msc_sweep_* price kernels by its row
// count -- it asks here whether the view is still there (bound_view_of).  A destroyed view's serial never comes back, so
// a new view at the old address does not pass for it.
static std::mutex g_views_mu;
static std::vector<uint64_t> g_live_views;
static void view_register(uint64_t serial) {
  std::lock_guard<std::mutex> lock(g_views_mu);
  g_live_views.push_back(serial);
}
static void view_unregister(uint64_t serial) {
  std::lock_guard<std::mutex> lock(g_views_mu);
  g_live_views.erase(std::remove(g_live_views.begin(), g_live_views.end(), serial), g_live_views.end());
}
static bool view_alive(uint64_t serial) {
  std::lock_guard<std::mutex> lock(g_views_mu);
  return std::find(g_live_views.begin(), g_live_views.end(), serial) != g_live_views.end();
}
// the view the state last bound, if it still exists and is the one that was bound (msc_dataview_invalidate moves a
// view's serial on); otherwise the binding is dropped: no column pointer of it is dereferenced again, the next call
// that brings a view binds afresh
static const msc_dataview *bound_view_of(msc_state *st) {
  if (st->bound_view == nullptr) return nullptr;
  if (view_alive(st->bound_serial) && st->bound_view->serial == st->bound_serial) return st->bound_view;
  st->bound_view = nullptr;
  st->bound_serial = 0;
  st->bound_cols.clear();
  for (FeatDesc &d : st->desc_host) {
    d.col = nullptr;
    d.mask = nullptr;
    d.col_sentinel = nullptr;
    d.dm_tot = nullptr;
  }
  return nullptr;
}

extern "C" int msc_dataview_from_records(msc_context *ctx, const void *host_records,
                                         const uint8_t *host_mask, uint64_t nrows,
                                         const msc_runtime_type *types, uint32_t ntypes,
                                         const int32_t *col_types, msc_dataview **out) {
  MSC_REQUIRE(ctx && out && types, "null argument");
  MSC_REQUIRE(ntypes > 0, "a dataview needs at least one feature");
  MSC_REQUIRE(nrows == 0 || host_records, "null records");
  *out = nullptr;
  MSC_HIP(hipSetDevice(ctx->device));
  // runtime_type::GetOffsetsAndSize (runtime_type.hpp:123-134)
  std::vector<UnpackFeat> uf(ntypes);
  size_t rowsize = 0, maskrowsize = 0;
  for (uint32_t i = 0; i < ntypes; i++) {
    MSC_REQUIRE(types[i].type >= 0 && types[i].type < MSC_TYPE_NELEMS, "feature %u: bad type %d", i,
                types[i].type);
    MSC_REQUIRE(types[i].count >= 1, "feature %u: count must be >= 1", i);
    const int dst = col_types ? col_types[i] : types[i].type;
    MSC_REQUIRE(dst >= 0 && dst < MSC_TYPE_NELEMS, "feature %u: bad column type %d", i, dst);
    uf[i].offset = (uint32_t)rowsize;
    uf[i].mask_offset = (uint32_t)maskrowsize;
    uf[i].src_type = types[i].type;
    uf[i].dst_type = dst;
    uf[i].count = types[i].count;
    rowsize += primitive_size(types[i].type) * types[i].count;
    maskrowsize += types[i].count;
  }
  std::unique_ptr<msc_dataview> v(new (std::nothrow) msc_dataview());
  if (!v) return fail(MSC_ENOMEM, "out of host memory");
  v->ctx = ctx;
  v->serial = next_view_serial();
  v->nrows = nrows;
  for (uint32_t i = 0; i < ntypes; i++) {
    DevBuf<uint8_t> col, mask;
    MSC_TRY(alloc_zeroed(col, (size_t)nrows * types[i].count * primitive_size(uf[i].dst_type)));
    if (host_mask) MSC_TRY(alloc_zeroed(mask, (size_t)nrows * types[i].count));
    uf[i].dst = col;
    uf[i].dst_mask = mask;
    v->cols.push_back(col);
    v->masks.push_back(mask);
    v->types.push_back(msc_runtime_type{uf[i].dst_type, types[i].count});
    v->owned.push_back(std::move(col));
    if (mask) v->owned.push_back(std::move(mask));
  }
  v->col_max.assign(ntypes, -1);
  v->dm_max.assign(ntypes, std::vector<uint32_t>());
  if (nrows > 0) {
    DevBuf<uint8_t> rec_dev, mask_dev;
    DevBuf<UnpackFeat> uf_dev;
    MSC_TRY(alloc_zeroed(rec_dev, (size_t)nrows * rowsize));
    MSC_TRY(alloc_zeroed(uf_dev, ntypes));
    if (host_mask) MSC_TRY(alloc_zeroed(mask_dev, (size_t)nrows * maskrowsize));
    hipError_t e = hipMemcpyAsync(rec_dev, host_records, (size_t)nrows * rowsize, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && host_mask)
      e = hipMemcpyAsync(mask_dev, host_mask, (size_t)nrows * maskrowsize, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(uf_dev, uf.data(), sizeof(UnpackFeat) * ntypes, hipMemcpyHostToDevice, ctx->stream);
    int rc = e == hipSuccess ? MSC_OK : fail(MSC_EHIP, "upload failed: %s", hipGetErrorString(e));
    if (rc == MSC_OK &&
        launch_unpack(ctx->stream, rec_dev, mask_dev, nrows, (uint32_t)rowsize, (uint32_t)maskrowsize, uf_dev, ntypes))
      rc = fail(MSC_EHIP, "k_unpack launch failed: %s", hipGetErrorString(hipGetLastError()));
    e = hipStreamSynchronize(ctx->stream);              // (also before the staging buffers go on a failure)
    if (rc == MSC_OK && e != hipSuccess) rc = fail(MSC_EHIP, "k_unpack failed: %s", hipGetErrorString(e));
    MSC_TRY(rc);
  }
  view_register(v->serial);
  *out = v.release();
  return MSC_OK;
}

extern "C" int msc_dataview_from_device_columns(msc_context *ctx, uint64_t nrows,
                                                const msc_runtime_type *types, uint32_t ntypes,
                                                void *const *dev_columns, void *const *dev_masks,
                                                msc_dataview **out) {
  MSC_REQUIRE(ctx && out && types && dev_columns, "null argument");
  MSC_REQUIRE(ntypes > 0, "a dataview needs at least one feature");
  *out = nullptr;
  std::unique_ptr<msc_dataview> v(new (std::nothrow) msc_dataview());
  if (!v) return fail(MSC_ENOMEM, "out of host memory");
  v->ctx = ctx;
  v->serial = next_view_serial();
  v->nrows = nrows;
  for (uint32_t i = 0; i < ntypes; i++) {
    MSC_REQUIRE(types[i].type >= 0 && types[i].type < MSC_TYPE_NELEMS, "feature %u: bad type", i);
    MSC_REQUIRE(types[i].count >= 1, "feature %u: count must be >= 1", i);
    MSC_REQUIRE(nrows == 0 || dev_columns[i], "feature %u: null column", i);
    MSC_REQUIRE(reinterpret_cast<uintptr_t>(dev_columns[i]) % primitive_size(types[i].type) == 0,
                "feature %u: column not aligned to its element size (%u bytes)", i, (unsigned)primitive_size(types[i].type));
    v->types.push_back(types[i]);
    v->cols.push_back(dev_columns[i]);
    v->masks.push_back(dev_masks ? dev_masks[i] : nullptr);
  }
  v->col_max.assign(ntypes, -1);
  v->dm_max.assign(ntypes, std::vector<uint32_t>());
  view_register(v->serial);
  *out = v.release();
  return MSC_OK;
}

extern "C" int msc_dataview_destroy(msc_dataview *view) {
  if (!view) return MSC_OK;
  view_unregister(view->serial);                          // (states that had it bound drop the binding: bound_view_of)
  (void)hipSetDevice(view->ctx->device);
  (void)hipStreamSynchronize(view->ctx->stream);
  delete view;
  return MSC_OK;
}

// What the library derives from a view's columns and keeps WITH the view -- a column converted to a model's value type
// (column_as), a masked lookup column with the mask folded in (sentinel_column), bool columns packed four to a byte
// (packed_column), the maxima of count columns and dm row totals that size the exact tables -- is a SNAPSHOT of the
// columns' contents.  A view made by msc_dataview_from_records owns its columns and nothing else can write them; a view
// over the caller's device columns (msc_dataview_from_device_columns) must be told when the caller has rewritten them in
// place (the usual minibatch pattern): this call drops every derived copy and moves the view's serial on, so that every
// state binds -- and derives -- afresh at its next call.  Synchronises the context's stream.
extern "C" int msc_dataview_invalidate(msc_dataview *view) {
  MSC_REQUIRE(view, "null view");
  MSC_HIP(hipSetDevice(view->ctx->device));
  MSC_HIP(hipStreamSynchronize(view->ctx->stream));
  view_unregister(view->serial);
  view->copies.clear();
  view->col_max.assign(view->cols.size(), -1);
  view->dm_max.assign(view->cols.size(), std::vector<uint32_t>());
  view->serial = next_view_serial();
  view_register(view->serial);
  return MSC_OK;
}

extern "C" int msc_dataview_size(const msc_dataview *view, uint64_t *nrows, uint32_t *nfeatures) {
  MSC_REQUIRE(view, "null view");
  if (nrows) *nrows = view->nrows;
  if (nfeatures) *nfeatures = (uint32_t)view->types.size();
  return MSC_OK;
}

extern "C" int msc_dataview_column(const msc_dataview *view, uint32_t feature, void **dev_ptr,
                                   msc_runtime_type *type) {
  MSC_REQUIRE(view, "null view");
  MSC_REQUIRE(feature < view->types.size(), "feature %u out of range", feature);
  if (dev_ptr) *dev_ptr = view->cols[feature];
  if (type) *type = view->types[feature];
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------
extern "C" size_t msc_hp_floats(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB: return 2;
    case MSC_BBNC: return 2;
    case MSC_GP: return 2;
    case MSC_DD: return dim;
    case MSC_NICH: return 4;
    case MSC_NIW: return 2 + (size_t)dim + (size_t)dim * dim;
    case MSC_BNB: return 3;
    case MSC_DM: return dim;
    default: return 0;
  }
}

extern "C" size_t msc_ss_bytes(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB: return 8;
    case MSC_BBNC: return 12;
    case MSC_GP: return 12;
    case MSC_DD: return 4 * (1 + (size_t)dim);
    case MSC_NICH: return 12;
    case MSC_NIW: return 4 * (1 + (size_t)dim + (size_t)dim * dim);
    case MSC_BNB: return 8;
    case MSC_DM: return 4 * ((size_t)dim + 1);
    default: return 4;
  }
}

static void default_hp(int family, uint32_t dim, std::vector<float> &hp) {
  // microscopes/models.pyx:189,211,223,238,264-269
  hp.assign(msc_hp_floats(family, dim), 0.f);
  switch (family) {
    case MSC_BB: hp[0] = 1; hp[1] = 1; break;
    case MSC_BBNC: hp[0] = 1; hp[1] = 1; break;
    case MSC_GP: hp[0] = 1; hp[1] = 1; break;
    case MSC_DD: std::fill(hp.begin(), hp.end(), 1.f); break;
    case MSC_DM: std::fill(hp.begin(), hp.end(), 1.f); break;     // models.pyx:287 (dd's defaults)
    case MSC_BNB: hp[0] = 1; hp[1] = 1; hp[2] = 1; break;          // models.pyx:200
    case MSC_NICH: hp[0] = 0; hp[1] = 1; hp[2] = 1; hp[3] = 1; break;
    case MSC_NIW:
      hp[0] = 1; hp[1] = (float)dim;
      for (uint32_t i = 0; i < dim; i++) hp[2 + dim + (size_t)i * dim + i] = 1.f;
      break;
    default: break;
  }
}

// The view's derived copies (msc_dataview::copies): the one of this kind and key, or null; and a new one.
static const void *view_copy(const msc_dataview *view, msc_dataview::CopyKind kind, const std::vector<uint64_t> &key) {
  for (const msc_dataview::Copy &e : view->copies)
    if (e.kind == kind && e.key == key) return e.buf;
  return nullptr;
}
static void *view_copy_add(const msc_dataview *view, msc_dataview::CopyKind kind, std::vector<uint64_t> key,
                           DevBuf<uint8_t> &&buf) {
  view->copies.push_back(msc_dataview::Copy{kind, std::move(key), std::move(buf)});
  return view->copies.back().buf;
}
static size_t view_copies(const msc_dataview *view, msc_dataview::CopyKind kind) {
  return (size_t)std::count_if(view->copies.begin(), view->copies.end(),
                               [kind](const msc_dataview::Copy &e) { return e.kind == kind; });
}
static std::vector<uint64_t> pointer_key(const void *const *p, size_t n) {
  std::vector<uint64_t> key(n);
  for (size_t i = 0; i < n; i++) key[i] = reinterpret_cast<uintptr_t>(p[i]);
  return key;
}

// the byte column holding the bits of m bool columns (kept by the view: every state that fuses the same columns shares it)
static int packed_column(const msc_dataview *view, const void *const *cols, int m, uint32_t radix, const void **out) {
  std::vector<uint64_t> key = pointer_key(cols, m);
  key.push_back(radix);
  if ((*out = view_copy(view, msc_dataview::kPackedBits, key))) return MSC_OK;
  DevBuf<uint8_t> dst;
  MSC_HIP(dst.alloc(view->nrows, 1));
  if (launch_pack_bits(view->ctx->stream, cols, m, radix, view->nrows, dst)) return fail(MSC_EHIP, "k_pack_bits launch failed");
  *out = view_copy_add(view, msc_dataview::kPackedBits, std::move(key), std::move(dst));
  return MSC_OK;
}

// the float columns `cols` (n2 of them; device, one float a row) as one matrix float [nrows][n2p], n2p = n2 rounded up to
// four and the padding zero: what the role-split kernels' nich waves read a row's second-phase values from (msc::NichPos).
// Kept by the view like the packed bool columns; a copy of those columns (64 MB for C3's sixteen on a million rows).
// A view keeps at most kViewPackCap matrices of either kind (one per distinct column list a state bound it with); a
// plan that would need one more, or whose allocation fails, does without -- the kernels that run the phases one after
// the other need neither (the copies are an optimisation, never a reason for a call to fail).
constexpr size_t kViewPackCap = 8;
static bool nich_x_matrix(const msc_dataview *view, const std::vector<const void *> &cols, const float **out) {
  std::vector<uint64_t> key = pointer_key(cols.data(), cols.size());
  if ((*out = static_cast<const float *>(view_copy(view, msc_dataview::kNichX, key)))) return true;
  if (view_copies(view, msc_dataview::kNichX) >= kViewPackCap) return false;
  const uint32_t n2 = (uint32_t)cols.size(), n2p = (n2 + 3u) & ~3u;
  DevBuf<uint8_t> dst;
  if (dst.alloc((size_t)view->nrows * n2p * sizeof(float), 16) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  DevBuf<const float *> ptrs;
  bool ok = ptrs.alloc(n2) == hipSuccess;
  ok = ok && hipMemcpyAsync(ptrs, cols.data(), sizeof(void *) * n2, hipMemcpyHostToDevice, view->ctx->stream) == hipSuccess;
  ok = ok && launch_pack_nich_x(view->ctx->stream, ptrs, n2, n2p, view->nrows, reinterpret_cast<float *>(dst.get())) == 0;
  ok = (hipStreamSynchronize(view->ctx->stream) == hipSuccess) && ok;      // (`cols` is the caller's, `ptrs` this function's)
  ptrs.reset();
  if (!ok) {
    (void)hipGetLastError();
    return false;
  }
  *out = static_cast<const float *>(view_copy_add(view, msc_dataview::kNichX, std::move(key), std::move(dst)));
  return true;
}

// The lookup index matrix of a plan's first phase as tile_plan.hpp plan_look_idx laid it out (msc::FeatDesc::lk_idx).
// Kept by the view like the x matrix.  false: no matrix (cap reached, or no memory) -- the plan does not take the kernels
// that read one.
static bool look_idx_matrix(const msc_dataview *view, const LookIdxLayout &lay, const uint32_t **out) {
  const std::vector<LookIdxSrc> &src = lay.src;
  std::vector<uint64_t> key = lay.key;
  const uint32_t split = (uint32_t)src.size(), l4 = lay.l4;
  if ((*out = static_cast<const uint32_t *>(view_copy(view, msc_dataview::kLookIdx, key)))) return true;
  if (view_copies(view, msc_dataview::kLookIdx) >= kViewPackCap || split == 0) return false;
  DevBuf<uint8_t> dst;
  if (dst.alloc(((size_t)view->nrows * l4 + 4u) * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  uint32_t *const idx = reinterpret_cast<uint32_t *>(dst.get());
  DevBuf<LookIdxSrc> srcs;
  bool ok = srcs.alloc(split) == hipSuccess;
  ok = ok && hipMemcpyAsync(srcs, src.data(), sizeof(LookIdxSrc) * split, hipMemcpyHostToDevice, view->ctx->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(idx + (size_t)view->nrows * l4, 0, 4u * sizeof(uint32_t), view->ctx->stream) == hipSuccess;
  ok = ok && launch_pack_look_idx(view->ctx->stream, srcs, split, l4, view->nrows, idx) == 0;
  ok = (hipStreamSynchronize(view->ctx->stream) == hipSuccess) && ok;
  srcs.reset();
  if (!ok) {
    (void)hipGetLastError();
    return false;
  }
  *out = static_cast<const uint32_t *>(view_copy_add(view, msc_dataview::kLookIdx, std::move(key), std::move(dst)));
  return true;
}

// The plans of a state (tile_plan.hpp holds the steps and their rules): the steps in order, and between them what needs
// the device -- the bound view's derived copies, the uploads.  st->plan is written whole at the end.
static int plan_groups(msc_state *st) {
  const msc_dataview *const bview = bound_view_of(st);    // (null: no column pointer survives in desc_host either)
  const Switches sw = read_switches();
  TilePlan p;
  std::vector<FeatDesc> &t = st->desc_tile_host, &tf = st->desc_fuse_host;
  // the tile plan: phase order and nich blocks, sentinel copies, groups and lookup runs, leave-one-out stages
  std::vector<uint32_t> nu_bits(st->nfeat, 0u);
  for (uint32_t i = 0; i < st->nfeat; i++)
    if (st->feats[i].family == MSC_NICH) std::memcpy(&nu_bits[i], &st->feats[i].hp[3], 4);
  const PhaseOrder po = plan_phases(st->desc_host, nu_bits, st->nich_info, t);
  p.tile_split = po.split, p.nich_blocks_any = po.nich_blocks_any;
  const std::vector<uint32_t> extra = plan_sentinels(t);
  PlanFacts facts = plan_layout(t, po.split, extra, sw);
  p.loo_staged = plan_loo_stages(t, st->kpad);
  // the score / sweep kernels' plan: runs of bool columns fused (the view packs each run's columns into one), then the
  // accumulate pass's list, then the fused plan's own groups and runs
  const FusedRuns fr = plan_fused_runs(t, po.split, extra, bview != nullptr && !sw.no_bb_fuse);
  MSC_HIP(grow_retained(st->retired, st->fuse_tab, fr.quads.size() * 32 * (size_t)st->kpad));
  std::vector<const void *> packed(fr.quads.size(), nullptr);
  for (size_t q = 0; q < fr.quads.size(); q++) {
    const void *cols[4] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t j = 0; j < fr.quads[q].m; j++) cols[j] = t[fr.member(q, j)].col;
    MSC_TRY(packed_column(bview, cols, (int)fr.quads[q].m, fr.quads[q].radix, &packed[q]));
  }
  std::vector<uint32_t> extra_f;
  plan_fused_list(t, po.split, extra, fr, packed, st->fuse_tab, st->kpad, tf, extra_f, p);
  plan_acc_list(st->desc_host, po.t_src, tf, fr, st->K, st->desc_acc_host);
  if (p.fuse_any) facts = plan_layout(tf, p.fuse_split, extra_f, sw);
  // what the kernels of the three other paths read of the view: the x matrix beside the positions (the nich waves), the
  // lookup index matrix (the lookup waves).  No view, or a view that cannot hold one more copy: the plan takes TILE
  clear_view_reads(tf);
  clear_view_reads(t);
  facts.path = path_for_view(facts.path, bview != nullptr);
  if (stages_nich(facts.path)) {
    std::vector<NichPos> pos;
    std::vector<const void *> xcols;
    plan_nich_pos(tf, p.fuse_split, pos, xcols);
    const float *xm = nullptr;
    if (nich_x_matrix(bview, xcols, &xm)) {
      MSC_HIP(hipMemcpyAsync(st->rn_pos, pos.data(), sizeof(NichPos) * pos.size(), hipMemcpyHostToDevice, st->ctx->stream));
      MSC_HIP(hipStreamSynchronize(st->ctx->stream));           // (`pos` is this function's)
      FeatDesc &h = tf[p.fuse_split];
      h.rn_pack = st->rn_pack, h.rn_pos = st->rn_pos, h.rn_x = xm, h.rn_n2 = (uint32_t)xcols.size(), h.rn_n2p = (uint32_t)pos.size();
    } else facts.path = MSC_PATH_TILE;                         // (no copy: the kernels that stage the nich constants need none)
  }
  if (facts.path == MSC_PATH_TILE_ROLES || facts.path == MSC_PATH_LOOKUPS) {
    LookIdxLayout lay;
    const uint32_t *im = nullptr;
    if (plan_look_idx(tf, p.fuse_split, lay) && look_idx_matrix(bview, lay, &im)) tf[0].lk_idx = im, tf[0].lk_l4 = lay.l4;
    else facts.path = MSC_PATH_TILE;
  }
  // the path, its prices, and what the lane <-> row kernel needs of the plan
  p.tile_path = facts.path;
  p.plan_cost = plan_prices(tf, p.fuse_split, facts.path);
  p.tile_narrow_tail_ok = facts.tail_ok;
  p.tail_masked_nich = facts.tail_masked_nich;
  p.tail_dm = facts.tail_dm;
  p.tail_max_rows = facts.tail_max_rows;
  p.tail_pack_rows = facts.tail_pack_rows;
  st->plan = p;
  return MSC_OK;
}

static void refresh_route_facts(msc_state *st);
static int upload_desc(msc_state *st) {
  MSC_TRY(plan_groups(st));
  refresh_route_facts(st);
  MSC_HIP(hipMemcpyAsync(st->desc_dev, st->desc_host.data(), sizeof(FeatDesc) * st->nfeat,
                         hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipMemcpyAsync(st->desc_tile_dev, st->desc_tile_host.data(), sizeof(FeatDesc) * st->nfeat,
                         hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipMemcpyAsync(st->desc_fuse_dev, st->desc_fuse_host.data(), sizeof(FeatDesc) * st->plan.fuse_nfeat,
                         hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipMemcpyAsync(st->desc_acc_dev, st->desc_acc_host.data(), sizeof(FeatDesc) * st->desc_acc_host.size(),
                         hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipStreamSynchronize(st->ctx->stream));     // (the tile copy is rebuilt by the next call)
  return MSC_OK;
}

extern "C" int msc_state_create(msc_context *ctx, const msc_feature_spec *features,
                                uint32_t nfeatures, uint32_t ngroups, msc_state **out) {
  MSC_REQUIRE(ctx && features && out, "null argument");
  MSC_REQUIRE(nfeatures > 0 && nfeatures <= 65535, "a state needs 1..65535 features (got %u)", nfeatures);
  MSC_REQUIRE(ngroups > 0 && ngroups <= (1u << 20), "ngroups %u out of range", ngroups);
  *out = nullptr;
  MSC_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<msc_state> st(new (std::nothrow) msc_state());
  if (!st) return fail(MSC_ENOMEM, "out of host memory");
  st->ctx = ctx;
  st->nfeat = nfeatures;
  st->K = ngroups;
  st->kpad = round_up(ngroups, kGroupTile);
  const size_t kpad = st->kpad;
  st->feats.resize(nfeatures);
  st->desc_host.resize(nfeatures);
  size_t n_i64 = kpad, n_f64 = 0;
  for (uint32_t f = 0; f < nfeatures; f++) {
    msc_feature_host &h = st->feats[f];
    h.family = features[f].family;
    h.dim = features[f].dim;
    MSC_REQUIRE(family_ok(h.family), "feature %u: unknown family %d", f, h.family);
    if (h.family == MSC_DD && (h.dim == 0 || h.dim > kMaxDDDim))
      return fail(MSC_EUNSUPPORTED, "feature %u: dd dim %u outside 1..%u (DirichletDiscrete<128>)", f,
                  h.dim, kMaxDDDim);
    if (h.family == MSC_DM && (h.dim == 0 || h.dim > kMaxDDDim))
      return fail(MSC_EUNSUPPORTED, "feature %u: dm categories %u outside 1..%u", f, h.dim, kMaxDDDim);
    if (h.family == MSC_NIW && (h.dim == 0 || h.dim > kMaxNiwDim))
      return fail(MSC_EUNSUPPORTED, "feature %u: niw dim %u outside 1..%u", f, h.dim, kMaxNiwDim);
    h.i64_off = n_i64;
    h.i64_len = acc_i64_rows(h.family, h.dim) * kpad;
    n_i64 += h.i64_len;
    h.f64_off = n_f64;
    h.f64_len = h.family == MSC_NIW ? (size_t)ngroups * (h.dim + (size_t)h.dim * h.dim)
                                    : acc_f64_rows(h.family) * kpad;
    n_f64 += h.f64_len;
  }
  st->n_i64 = n_i64;
  st->n_f64 = n_f64;
  st->nich1 = nfeatures == 1 && st->feats[0].family == MSC_NICH;
  for (const msc_feature_host &h : st->feats) st->has_dm |= h.family == MSC_DM, st->n_niw += h.family == MSC_NIW;
  MSC_TRY(alloc_zeroed(st->red_i64, n_i64));
  MSC_TRY(alloc_zeroed(st->red_f64, n_f64));
  MSC_TRY(alloc_zeroed(st->cnt_u32, kpad));
  MSC_TRY(alloc_zeroed(st->logpc, crp_floats(st->kpad)));
  MSC_TRY(alloc_zeroed(st->desc_dev, nfeatures));
  MSC_TRY(alloc_zeroed(st->desc_tile_dev, nfeatures));
  MSC_TRY(alloc_zeroed(st->desc_fuse_dev, nfeatures));
  MSC_TRY(alloc_zeroed(st->nich_info, nfeatures));
  MSC_TRY(alloc_zeroed(st->rn_pos, (size_t)((nfeatures + 3u) & ~3u)));
  {
    size_t nnich = 0;
    for (uint32_t f = 0; f < nfeatures; f++) nnich += features[f].family == MSC_NICH;
    MSC_TRY(alloc_zeroed(st->rn_pack, (1 + kNichPackRows * nnich) * (size_t)kpad));
  }
  MSC_TRY(alloc_zeroed(st->desc_acc_dev, nfeatures));
  MSC_TRY(alloc_zeroed(st->rng_dev, 2));
  MSC_TRY(alloc_zeroed(st->colmax_dev, 1));
  for (uint32_t f = 0; f < nfeatures; f++) {
    msc_feature_host &h = st->feats[f];
    default_hp(h.family, h.dim, h.hp);
    MSC_TRY(alloc_zeroed(h.hp_dev, h.hp.size()));
    MSC_TRY(alloc_zeroed(h.tab, (size_t)(tab_rows(h.family, h.dim) + 4) * kpad));   // +4: stage_table1 copies 4 rows per instruction
    MSC_TRY(alloc_zeroed(h.raw_u32, (size_t)raw_u32_rows(h.family, h.dim) * kpad));
    const size_t nf32 = h.family == MSC_NIW ? (size_t)ngroups * (h.dim + (size_t)h.dim * h.dim)
                                            : (size_t)raw_f32_rows(h.family) * kpad;
    MSC_TRY(alloc_zeroed(h.raw_f32, nf32));
    if (loo_rows(h.family)) MSC_TRY(alloc_zeroed(h.loo64, (size_t)loo_rows(h.family) * kpad));
    if (loo_tab_rows(h.family, h.dim)) MSC_TRY(alloc_zeroed(h.loo_tab, (size_t)loo_tab_rows(h.family, h.dim) * kpad));
    if (h.family == MSC_DM) {
      MSC_TRY(alloc_zeroed(h.dm_meta_dev, 2 * ((size_t)h.dim + 1)));
      h.dm_meta.assign(2 * ((size_t)h.dim + 1), 0u);
    }
    if (h.family == MSC_NIW) {
      if (h.dim <= (uint32_t)kNiwPad) {                    // operands of the f32 MFMA kernel (MSC_SCORE_NIW_F32), dim <= 32 only
        MSC_TRY(alloc_zeroed(h.niw_w, (size_t)ngroups * kNiwPad * kNiwPad));
        MSC_TRY(alloc_zeroed(h.niw_b, (size_t)ngroups * 2 * kNiwPad));
      }
      MSC_TRY(alloc_zeroed(h.niw_w64, (size_t)ngroups * niw_w_stream(h.dim)));
      MSC_TRY(alloc_zeroed(h.niw_mu64, (size_t)ngroups * niw_b_stream(h.dim)));
      MSC_TRY(alloc_zeroed(h.niw_c64, (size_t)ngroups * 8));
    }
    if (!h.hp.empty()) {
      hipError_t e = hipMemcpy(h.hp_dev, h.hp.data(), h.hp.size() * sizeof(float), hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(MSC_EHIP, "hp upload failed: %s", hipGetErrorString(e));
    }
    FeatDesc &d = st->desc_host[f];
    std::memset(&d, 0, sizeof d);
    d.family = h.family;
    d.dim = h.dim;
    d.col_type = value_type_of(h.family);
    d.hp = h.hp_dev;
    d.tab = h.tab;
    d.raw_u32 = h.raw_u32;
    d.raw_f32 = h.raw_f32;
    d.acc_i64 = st->red_i64 + h.i64_off;
    d.acc_f64 = st->red_f64 + h.f64_off;
    d.niw_w = h.niw_w;
    d.niw_b = h.niw_b;
    d.niw_w64 = h.niw_w64;
    d.niw_mu64 = h.niw_mu64;
    d.niw_c64 = h.niw_c64;
    d.vcap = 32;
    d.dm_meta = nullptr;       // set when a column is bound
    d.loo64 = h.loo64;
    d.loo_tab = h.loo_tab;
    d.aux = 0.0;
    for (float a : h.hp) d.aux += h.family == MSC_DD || h.family == MSC_DM ? (double)a : 0.0;
  }
  st->valid.created(nfeatures);       // (raw and additive both all-zero)
  MSC_TRY(upload_desc(st.get()));
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(MSC_EHIP, "state init failed: %s", hipGetErrorString(e));
  *out = st.release();
  return MSC_OK;
}

// the one place that destroys a captured step (msc_sweep_step): whatever the executable holds that no longer stands --
// another key, the kernels or table sizes of an old plan -- the next steps count afresh
static void drop_step_graph(msc_state *st) {
  msc_state::StepGraph &g = st->step_graph;
  if (!g.exec) return;
  (void)hipGraphExecDestroy(g.exec);
  g.exec = nullptr;
  g.seen = 0;
}

extern "C" int msc_state_destroy(msc_state *st) {
  if (!st) return MSC_OK;
  MSC_REQUIRE(st->chain_members == 0, "msc_state_destroy: the state is a member of %u live msc_chains handle(s), whose "
                                      "table holds its buffers; destroy those first (msc_chains_destroy)", st->chain_members);
  (void)hipSetDevice(st->ctx->device);
  (void)hipStreamSynchronize(st->ctx->stream);
  drop_step_graph(st);
  if (st->sm.pair) (void)msc_state_destroy(st->sm.pair);
  delete st;
  return MSC_OK;
}

extern "C" int msc_state_shape(const msc_state *st, uint32_t *nfeatures, uint32_t *ngroups) {
  MSC_REQUIRE(st, "null state");
  if (nfeatures) *nfeatures = st->nfeat;
  if (ngroups) *ngroups = st->K;
  return MSC_OK;
}

// dd / dm: the sum of the feature's alphas (FeatDesc::aux) follows its host hp block, in every host copy of the
// descriptor; whether the family carries one.  The device side is the caller's: msc_state_set_hp uploads, hp_installed
// does not (the kernel wrote it).
bool msc::refresh_alpha_sum(msc_state *st, uint32_t feature) {
  const msc_feature_host &h = st->feats[feature];
  if (h.family != MSC_DD && h.family != MSC_DM) return false;
  double asum = 0;
  for (float a : h.hp) asum += (double)a;
  st->desc_host[feature].aux = asum;
  for (auto *v : {&st->desc_tile_host, &st->desc_fuse_host, &st->desc_acc_host})
    for (FeatDesc &d : *v)
      if (d.hp == h.hp_dev) d.aux = asum;
  return true;
}

extern "C" int msc_state_set_hp(msc_state *st, uint32_t feature, const float *host_hp, size_t nfloats) {
  MSC_REQUIRE(st && host_hp, "null argument");
  MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
  msc_feature_host &h = st->feats[feature];
  MSC_REQUIRE(nfloats == h.hp.size(), "feature %u: hp block has %zu floats, expected %zu", feature,
              nfloats, h.hp.size());
  std::copy(host_hp, host_hp + nfloats, h.hp.begin());
  st->valid.hp_changed(feature);
  if (nfloats) {
    MSC_HIP(hipMemcpyAsync(h.hp_dev, h.hp.data(), nfloats * sizeof(float), hipMemcpyHostToDevice, st->ctx->stream));
    MSC_HIP(hipStreamSynchronize(st->ctx->stream));
  }
  if (refresh_alpha_sum(st, feature)) MSC_TRY(upload_desc(st));
  return MSC_OK;
}

extern "C" int msc_state_get_hp(const msc_state *st, uint32_t feature, float *host_hp, size_t nfloats) {
  MSC_REQUIRE(st && host_hp, "null argument");
  MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
  const msc_feature_host &h = st->feats[feature];
  MSC_REQUIRE(nfloats == h.hp.size(), "feature %u: hp block has %zu floats, expected %zu", feature,
              nfloats, h.hp.size());
  std::copy(h.hp.begin(), h.hp.end(), host_hp);
  return MSC_OK;
}

static int launch_commit_all(msc_state *st) {
  if (launch_commit(st->ctx->stream, st->desc_dev, (int)st->nfeat, st->kpad, st->red_i64, st->cnt_u32))
    return fail(MSC_EHIP, "k_commit launch failed");
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (st->feats[f].family == MSC_NIW &&
        launch_niw_commit(st->ctx->stream, st->desc_dev, f, st->feats[f].dim, st->K, st->kpad, 1))
      return fail(MSC_EHIP, "k_niw_commit launch failed");
  return MSC_OK;
}

int msc::ensure_raw(msc_state *st) {
  if (!st->valid.any_raw_stale()) return MSC_OK;
  MSC_TRY(launch_commit_all(st));
  st->valid.committed();
  return MSC_OK;
}

// refuses a call between msc_sweep_step_begin and msc_state_commit_reduce
int msc::refuse_mid_step(const msc_state *st, const char *entry) {
  MSC_REQUIRE(!st->rng.mid_step(), "%s between msc_sweep_step_begin and msc_state_commit_reduce: the additive tables "
                                   "hold one rank's uncommitted sums", entry);
  return MSC_OK;
}

// u32 rows / f32 rows of one family's packed record, in record order
static void record_layout(int family, uint32_t dim, uint32_t &nu32, uint32_t &nf32) {
  nu32 = raw_u32_rows(family, dim);
  nf32 = raw_f32_rows(family);
}

extern "C" int msc_state_set_ss(msc_state *st, uint32_t feature, uint32_t first_group,
                                uint32_t ngroups, const void *host_records, size_t nbytes) {
  MSC_REQUIRE(st && host_records, "null argument");
  MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
  msc_feature_host &h = st->feats[feature];
  MSC_REQUIRE(ngroups > 0 && first_group <= st->K && ngroups <= st->K - first_group,      // (no 32-bit wrap of the sum)
              "groups [%u,%llu) outside [0,%u)", first_group, (unsigned long long)first_group + ngroups, st->K);
  const size_t rec = msc_ss_bytes(h.family, h.dim);
  MSC_REQUIRE(nbytes == rec * ngroups, "expected %zu bytes of records, got %zu", rec * ngroups, nbytes);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  st->valid.fields_written(feature);
  if (h.family == MSC_NIW) {
    // record = {u32 count, f32 sum_x[d], f32 sum_xxT[d*d]}; device keeps count as a row and the
    // float block group-major
    const size_t nf = h.dim + (size_t)h.dim * h.dim;
    std::vector<uint32_t> cnt(ngroups);
    std::vector<float> blk(nf * ngroups);
    const uint8_t *p = static_cast<const uint8_t *>(host_records);
    for (uint32_t g = 0; g < ngroups; g++) {
      std::memcpy(&cnt[g], p + (size_t)g * rec, 4);
      std::memcpy(&blk[nf * g], p + (size_t)g * rec + 4, 4 * nf);
    }
    MSC_HIP(hipMemcpyAsync(h.raw_u32 + first_group, cnt.data(), 4 * (size_t)ngroups, hipMemcpyHostToDevice, st->ctx->stream));
    MSC_HIP(hipMemcpyAsync(h.raw_f32 + nf * first_group, blk.data(), 4 * nf * ngroups, hipMemcpyHostToDevice, st->ctx->stream));
    MSC_HIP(hipStreamSynchronize(st->ctx->stream));
    return MSC_OK;
  }
  uint32_t nu32, nf32;
  record_layout(h.family, h.dim, nu32, nf32);
  // AoS records -> SoA rows
  std::vector<uint32_t> su((size_t)nu32 * ngroups);
  std::vector<float> sf((size_t)nf32 * ngroups);
  const uint8_t *p = static_cast<const uint8_t *>(host_records);
  for (uint32_t g = 0; g < ngroups; g++) {
    const uint8_t *r = p + (size_t)g * rec;
    for (uint32_t i = 0; i < nu32; i++) std::memcpy(&su[(size_t)i * ngroups + g], r + 4 * i, 4);
    for (uint32_t i = 0; i < nf32; i++) std::memcpy(&sf[(size_t)i * ngroups + g], r + 4 * (nu32 + i), 4);
  }
  for (uint32_t i = 0; i < nu32; i++)
    MSC_HIP(hipMemcpyAsync(h.raw_u32 + (size_t)i * st->kpad + first_group, &su[(size_t)i * ngroups],
                           4 * (size_t)ngroups, hipMemcpyHostToDevice, st->ctx->stream));
  for (uint32_t i = 0; i < nf32; i++)
    MSC_HIP(hipMemcpyAsync(h.raw_f32 + (size_t)i * st->kpad + first_group, &sf[(size_t)i * ngroups],
                           4 * (size_t)ngroups, hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipStreamSynchronize(st->ctx->stream));
  return MSC_OK;
}

extern "C" int msc_state_get_ss(msc_state *st, uint32_t feature, uint32_t first_group,
                                uint32_t ngroups, void *host_records, size_t nbytes) {
  MSC_REQUIRE(st && host_records, "null argument");
  MSC_REQUIRE(feature < st->nfeat, "feature %u out of range", feature);
  msc_feature_host &h = st->feats[feature];
  MSC_REQUIRE(ngroups > 0 && first_group <= st->K && ngroups <= st->K - first_group,      // (no 32-bit wrap of the sum)
              "groups [%u,%llu) outside [0,%u)", first_group, (unsigned long long)first_group + ngroups, st->K);
  const size_t rec = msc_ss_bytes(h.family, h.dim);
  MSC_REQUIRE(nbytes == rec * ngroups, "expected %zu bytes of records, got %zu", rec * ngroups, nbytes);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  if (h.family == MSC_NIW) {
    const size_t nf = h.dim + (size_t)h.dim * h.dim;
    std::vector<uint32_t> cnt(ngroups);
    std::vector<float> blk(nf * ngroups);
    MSC_HIP(hipMemcpyAsync(cnt.data(), h.raw_u32 + first_group, 4 * (size_t)ngroups, hipMemcpyDeviceToHost, st->ctx->stream));
    MSC_HIP(hipMemcpyAsync(blk.data(), h.raw_f32 + nf * first_group, 4 * nf * ngroups, hipMemcpyDeviceToHost, st->ctx->stream));
    MSC_HIP(hipStreamSynchronize(st->ctx->stream));
    uint8_t *p = static_cast<uint8_t *>(host_records);
    for (uint32_t g = 0; g < ngroups; g++) {
      std::memcpy(p + (size_t)g * rec, &cnt[g], 4);
      std::memcpy(p + (size_t)g * rec + 4, &blk[nf * g], 4 * nf);
    }
    return MSC_OK;
  }
  uint32_t nu32, nf32;
  record_layout(h.family, h.dim, nu32, nf32);
  std::vector<uint32_t> su((size_t)nu32 * ngroups);
  std::vector<float> sf((size_t)nf32 * ngroups);
  for (uint32_t i = 0; i < nu32; i++)
    MSC_HIP(hipMemcpyAsync(&su[(size_t)i * ngroups], h.raw_u32 + (size_t)i * st->kpad + first_group,
                           4 * (size_t)ngroups, hipMemcpyDeviceToHost, st->ctx->stream));
  for (uint32_t i = 0; i < nf32; i++)
    MSC_HIP(hipMemcpyAsync(&sf[(size_t)i * ngroups], h.raw_f32 + (size_t)i * st->kpad + first_group,
                           4 * (size_t)ngroups, hipMemcpyDeviceToHost, st->ctx->stream));
  MSC_HIP(hipStreamSynchronize(st->ctx->stream));
  uint8_t *p = static_cast<uint8_t *>(host_records);
  for (uint32_t g = 0; g < ngroups; g++) {
    uint8_t *r = p + (size_t)g * rec;
    for (uint32_t i = 0; i < nu32; i++) std::memcpy(r + 4 * i, &su[(size_t)i * ngroups + g], 4);
    for (uint32_t i = 0; i < nf32; i++) std::memcpy(r + 4 * (nu32 + i), &sf[(size_t)i * ngroups + g], 4);
  }
  return MSC_OK;
}

extern "C" int msc_state_set_alpha(msc_state *st, float alpha) {
  MSC_REQUIRE(st, "null state");
  MSC_REQUIRE(alpha > 0.f, "alpha must be positive (group_manager.hpp:78)");
  st->alpha = alpha;
  st->valid.alpha_changed();
  return MSC_OK;
}

extern "C" int msc_state_get_alpha(const msc_state *st, float *alpha) {
  MSC_REQUIRE(st && alpha, "null argument");
  *alpha = st->alpha;
  return MSC_OK;
}

extern "C" int msc_state_set_group_counts(msc_state *st, const uint32_t *host_counts, uint32_t ngroups) {
  MSC_REQUIRE(st && host_counts, "null argument");
  MSC_REQUIRE(ngroups == st->K, "expected %u counts, got %u", st->K, ngroups);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  MSC_HIP(hipMemcpyAsync(st->cnt_u32, host_counts, 4 * (size_t)ngroups, hipMemcpyHostToDevice, st->ctx->stream));
  MSC_HIP(hipStreamSynchronize(st->ctx->stream));
  st->valid.counts_changed();
  return MSC_OK;
}

extern "C" int msc_state_get_group_counts(msc_state *st, uint32_t *host_counts, uint32_t ngroups) {
  MSC_REQUIRE(st && host_counts, "null argument");
  MSC_REQUIRE(ngroups == st->K, "expected %u counts, got %u", st->K, ngroups);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  MSC_HIP(hipMemcpyAsync(host_counts, st->cnt_u32, 4 * (size_t)ngroups, hipMemcpyDeviceToHost, st->ctx->stream));
  MSC_HIP(hipStreamSynchronize(st->ctx->stream));
  return MSC_OK;
}

// ---------------------------------------------------------------------------
// binding a dataview to the state's features
// ---------------------------------------------------------------------------
// dm: one exact count table per category and one for the row totals, each covering 0..max of what the
// bound column holds (capped at kGpMaxTable); the maxima are found once per view column.
// The column as the model's value type.  The reference converts per value, whatever primitive type the column holds
// (runtime_cast::cast, runtime_type.hpp:145-166 -- its own niw descriptor pairs a float64 numpy dtype with a TYPE_F32[dim]
// model, microscopes/models.pyx:259); here the conversion happens once, when a state first binds the column to a model
// of another value type: a device copy through k_unpack's cast (the column read as one-feature records), kept with
// the view.  make = false: only look the copy up (null when there is none yet).
static int column_as(const msc_dataview *view, uint32_t c, int want, bool make, const void **out) {
  *out = nullptr;
  const msc_runtime_type t = view->types[c];
  if (t.type == want) {
    *out = view->cols[c];
    return MSC_OK;
  }
  std::vector<uint64_t> key{c, (uint64_t)want};
  if ((*out = view_copy(view, msc_dataview::kConverted, key)) || !make) return MSC_OK;
  hipStream_t s = view->ctx->stream;
  DevBuf<uint8_t> dst;
  MSC_HIP(dst.alloc((size_t)view->nrows * t.count * primitive_size(want), 1));
  if (view->nrows > 0) {
    UnpackFeat uf{};
    uf.dst = dst;
    uf.dst_mask = nullptr;                              // (the mask column is per element, whatever the value type)
    uf.offset = 0;
    uf.mask_offset = 0;
    uf.src_type = t.type;
    uf.dst_type = want;
    uf.count = t.count;
    DevBuf<UnpackFeat> uf_dev;
    MSC_HIP(uf_dev.alloc(1));
    hipError_t e = hipMemcpyAsync(uf_dev, &uf, sizeof uf, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && launch_unpack(s, static_cast<const uint8_t *>(view->cols[c]), nullptr, view->nrows,
                                         (uint32_t)(primitive_size(t.type) * t.count), 0, uf_dev, 1))
      e = hipErrorLaunchFailure;
    const hipError_t w = hipStreamSynchronize(s);       // (also before the buffers go on a failure)
    if (e == hipSuccess) e = w;
    if (e != hipSuccess) return fail(MSC_EHIP, "column conversion failed: %s", hipGetErrorString(e));
  }
  *out = view_copy_add(view, msc_dataview::kConverted, std::move(key), std::move(dst));
  return MSC_OK;
}

// A masked lookup column with the mask folded in (FeatDesc::col_sentinel): masked rows hold `sentinel`.  `col` is the
// column as the model's value type (column_as); made once per (column, element type, sentinel), kept with the view.
static int sentinel_column(const msc_dataview *view, uint32_t c, const void *col, bool bytes, uint32_t sentinel, const void **out) {
  *out = nullptr;
  std::vector<uint64_t> key{c, bytes ? 1u : 4u, sentinel};
  if ((*out = view_copy(view, msc_dataview::kSentinel, key))) return MSC_OK;
  DevBuf<uint8_t> dst;
  MSC_HIP(dst.alloc((size_t)view->nrows * (bytes ? 1 : 4), 1));
  if (launch_mask_sentinel(view->ctx->stream, col, static_cast<const uint8_t *>(view->masks[c]), view->nrows, bytes, sentinel, dst))
    return fail(MSC_EHIP, "k_mask_sentinel launch failed");
  *out = view_copy_add(view, msc_dataview::kSentinel, std::move(key), std::move(dst));
  return MSC_OK;
}

// The maxima the plan goes by: the view's own, raised to the whole dataset's where a sharded driver stated them
// (msc_state_set_col_bounds), so that every shard plans -- tables, groups, kernels -- as the whole would
static long long col_max_of(const msc_state *st, uint32_t f, const msc_dataview *view, uint32_t c) {
  const long long own = view->col_max[c];
  return f < st->col_bounds.size() && !st->col_bounds[f].empty() ? std::max(own, (long long)st->col_bounds[f][0]) : own;
}
// (i = dim: the row total's)
static uint32_t dm_max_of(const msc_state *st, uint32_t f, const msc_dataview *view, uint32_t c, uint32_t i) {
  const uint32_t own = view->dm_max[c][i];
  return f < st->col_bounds.size() && !st->col_bounds[f].empty() ? std::max(own, st->col_bounds[f][i]) : own;
}
// how many bounds the state's features take (msc_state_col_bounds / msc_state_set_col_bounds)
static size_t col_bound_count(const msc_state *st, uint32_t f) {
  const int fam = st->feats[f].family;
  return is_count_family(fam) ? 1 : fam == MSC_DM ? (size_t)st->feats[f].dim + 1 : 0;
}
static size_t col_bounds_size(const msc_state *st) {
  size_t n = 0;
  for (uint32_t f = 0; f < st->nfeat; f++) n += col_bound_count(st, f);
  return n;
}

static int bind_dm_column(msc_state *st, uint32_t f, const msc_dataview *view, uint32_t c) {
  msc_feature_host &h = st->feats[f];
  FeatDesc &d = st->desc_host[f];
  const uint32_t nst = h.dim + 1;
  hipStream_t s = st->ctx->stream;
  if (view->dm_max[c].empty()) {
    std::vector<uint32_t> mx(nst, 0u);
    if (view->nrows > 0) {
      DevBuf<uint8_t> tmp, tot;
      MSC_HIP(tmp.alloc(sizeof(uint32_t) * nst));
      MSC_HIP(tot.alloc(sizeof(uint32_t) * view->nrows));
      uint32_t *const tmp32 = reinterpret_cast<uint32_t *>(tmp.get()), *const tot32 = reinterpret_cast<uint32_t *>(tot.get());
      hipError_t e = hipMemsetAsync(tmp32, 0, sizeof(uint32_t) * nst, s);
      int rc = e == hipSuccess ? MSC_OK : fail(MSC_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
      if (rc == MSC_OK && launch_dm_stats(s, static_cast<const uint32_t *>(d.col), view->nrows, h.dim, tmp32, tot32))
        rc = fail(MSC_EHIP, "k_dm_stats launch failed");
      if (rc == MSC_OK && (e = hipMemcpyAsync(mx.data(), tmp32, sizeof(uint32_t) * nst, hipMemcpyDeviceToHost, s)))
        rc = fail(MSC_EHIP, "hipMemcpyAsync: %s", hipGetErrorString(e));
      e = hipStreamSynchronize(s);                      // (also before the buffers go on a failure)
      if (rc == MSC_OK && e != hipSuccess) rc = fail(MSC_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
      MSC_TRY(rc);
      view_copy_add(view, msc_dataview::kDmMax, {c}, std::move(tmp));
      view_copy_add(view, msc_dataview::kDmTot, {c}, std::move(tot));
    }
    view->dm_max[c] = mx;
  }
  d.dm_tot = static_cast<const uint32_t *>(view_copy(view, msc_dataview::kDmTot, {c}));
  std::vector<uint32_t> meta(2 * (size_t)nst);
  uint32_t rows = 0;
  for (uint32_t i = 0; i < nst; i++) {
    const uint32_t vcap = (uint32_t)std::min<unsigned long long>((unsigned long long)dm_max_of(st, f, view, c, i) + 1ull, kGpMaxTable);
    meta[2 * i] = rows;
    meta[2 * i + 1] = vcap;
    rows += 2 * vcap;                                   // (hi, lo) row pairs
  }
  d.dm_rows = rows;
  if (meta != h.dm_meta || d.dm_meta == nullptr) {
    // grow the table buffers, zeroed (rows is even: when the table grows, so does its twin below)
    if (((size_t)rows + 4) * st->kpad > h.tab.size() || h.loo64 == nullptr) {
      MSC_HIP(grow_retained(st->retired, h.tab, ((size_t)rows + 4) * st->kpad));
      MSC_HIP(hipMemset(h.tab, 0, h.tab.size() * sizeof(float)));
      d.tab = h.tab;
      // the leave-one-out twin of the tables ("count v against the group minus v"), one double per entry: read by
      // k_loo_own only, once per row and stage
      MSC_HIP(grow_retained(st->retired, h.loo64, ((size_t)rows / 2 + 1) * st->kpad));
      MSC_HIP(hipMemset(h.loo64, 0, h.loo64.size() * sizeof(double)));
      d.loo64 = h.loo64;
    }
    h.dm_meta = meta;
    MSC_HIP(hipMemcpyAsync(h.dm_meta_dev, h.dm_meta.data(), sizeof(uint32_t) * meta.size(), hipMemcpyHostToDevice, s));
    MSC_HIP(hipStreamSynchronize(s));
    d.dm_meta = h.dm_meta_dev;
    st->valid.derived_dropped(f);
  }
  return MSC_OK;
}

int msc::bind_view(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                   uint64_t nrows) {
  MSC_REQUIRE(view, "null dataview");
  MSC_REQUIRE(view->ctx->device == st->ctx->device, "dataview and state live on different devices");
  MSC_REQUIRE(msc::rows_within(row0, nrows, view->nrows), "rows [%llu,%llu) outside the view (%llu rows)",
              (unsigned long long)row0, (unsigned long long)(row0 + nrows),
              (unsigned long long)view->nrows);
  (void)bound_view_of(st);                                  // (a binding to a view that is gone, or was invalidated, is dropped first)
  bool same = !st->rebind && st->bound_view == view && st->bound_serial == view->serial && st->bound_cols.size() == st->nfeat;
  for (uint32_t f = 0; f < st->nfeat && same; f++) same = st->bound_cols[f] == (cols ? cols[f] : f);
  if (same) {
    for (uint32_t f = 0; f < st->nfeat && same; f++) {
      const void *eff = nullptr;
      if (st->feats[f].family == MSC_NOOP) eff = view->cols[st->bound_cols[f]];
      else MSC_TRY(column_as(view, st->bound_cols[f], value_type_of(st->feats[f].family), false, &eff));
      same = st->desc_host[f].col == eff;
    }
  }
  if (same) return MSC_OK;
  st->bound_cols.resize(st->nfeat);
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const uint32_t c = cols ? cols[f] : f;
    MSC_REQUIRE(c < view->types.size(), "feature %u: column %u outside the view (%zu columns)", f, c,
                view->types.size());
    const msc_feature_host &h = st->feats[f];
    const msc_runtime_type t = view->types[c];
    if (h.family != MSC_NOOP) {
      const uint32_t want_n = h.family == MSC_NIW || h.family == MSC_DM ? h.dim : 1;
      // model::get_runtime_type() fixes the element count (distributions.hpp:398-403, _dataview.pyx:27-44); the element
      // type is converted per value upstream (runtime_cast::cast) and once per column here (column_as)
      MSC_REQUIRE(t.count == want_n, "feature %u: column %u holds %u elements per value but the model wants %u", f, c,
                  t.count, want_n);
    }
    st->bound_cols[f] = c;
    const void *eff = view->cols[c];
    if (h.family != MSC_NOOP) MSC_TRY(column_as(view, c, value_type_of(h.family), true, &eff));
    st->desc_host[f].col = eff;
    st->desc_host[f].mask = static_cast<const uint8_t *>(view->masks[c]);
    st->desc_host[f].col_type = h.family != MSC_NOOP ? value_type_of(h.family) : t.type;
    if (is_count_family(h.family)) {
      // the exact table covers counts 0..max of the bound column (capped): find the max once
      if (view->col_max[c] < 0) {
        uint32_t mx = 0;
        if (view->nrows > 0) {
          MSC_HIP(hipMemsetAsync(st->colmax_dev, 0, 4, st->ctx->stream));
          if (launch_col_max_u32(st->ctx->stream, static_cast<const uint32_t *>(eff), view->nrows, st->colmax_dev))
            return fail(MSC_EHIP, "k_col_max_u32 launch failed");
          MSC_HIP(hipMemcpyAsync(&mx, st->colmax_dev, 4, hipMemcpyDeviceToHost, st->ctx->stream));
          MSC_HIP(hipStreamSynchronize(st->ctx->stream));
        }
        view->col_max[c] = (long long)mx;
      }
      const uint32_t vcap = (uint32_t)std::min<long long>(col_max_of(st, f, view, c) + 1, (long long)kGpMaxTable);
      if (vcap != st->desc_host[f].vcap) {
        st->desc_host[f].vcap = vcap;
        st->valid.derived_dropped(f);
      }
    }
    if (h.family == MSC_DM) MSC_TRY(bind_dm_column(st, f, view, c));
    // a masked column of a lookup family, for the tile kernels: the mask folded in as the index of the family's zero
    // table row, while that row is among those a feature group stages (plan_groups)
    st->desc_host[f].col_sentinel = nullptr;
    if (view->masks[c] != nullptr) {
      uint32_t sentinel = 0;
      bool ok = false, bytes = false;
      switch (h.family) {
        case MSC_BB:
        case MSC_BBNC: sentinel = 2, ok = true, bytes = true; break;
        case MSC_DD: sentinel = h.dim, ok = h.dim + 1 <= 64; break;
        case MSC_GP:
        case MSC_BNB: sentinel = st->desc_host[f].vcap, ok = sentinel + 1 <= 64; break;
        default: break;
      }
      if (ok) MSC_TRY(sentinel_column(view, c, eff, bytes, sentinel, &st->desc_host[f].col_sentinel));
    }
  }
  st->bound_view = view;
  st->bound_serial = view->serial;
  st->rebind = false;
  return upload_desc(st);
}

static uint32_t dm_value_slices(const msc_feature_host &h) {
  uint32_t rows = 1;
  for (size_t i = 1; i < h.dm_meta.size(); i += 2) rows = std::max(rows, h.dm_meta[i]);     // {first_row, vcap} per stage
  return std::min<uint32_t>(64, (rows + 3) / 4);
}

// threads per (feature, group) that share the rows of a count / categorical table in the prepare kernels: ~4 rows each
uint32_t msc::prepare_value_slices(const msc_state *st) {
  uint32_t rows = 1;
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const int fam = st->feats[f].family;
    if (is_count_family(fam)) rows = std::max(rows, st->desc_host[f].vcap);
    else if (fam == MSC_DD) rows = std::max(rows, st->feats[f].dim);
  }
  return std::min<uint32_t>(64, (rows + 3) / 4);
}

int msc::ensure_derived(msc_state *st) {
  MSC_TRY(ensure_raw(st));
  if (!st->valid.any_derived_stale()) return MSC_OK;
  if (launch_prepare(st->ctx->stream, st->desc_dev, st->nfeat, st->kpad, prepare_value_slices(st)))
    return fail(MSC_EHIP, "k_prepare launch failed");
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (st->feats[f].family == MSC_NIW && st->valid.derived_stale(f) &&
        launch_niw_prepare(st->ctx->stream, st->desc_dev, f, st->feats[f].dim, st->K, st->kpad))
      return fail(MSC_EHIP, "k_niw_prepare launch failed");
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (st->feats[f].family == MSC_DM && st->valid.derived_stale(f) && st->desc_host[f].dm_meta != nullptr &&
        launch_dm_prepare(st->ctx->stream, st->desc_dev, (int)f, st->feats[f].dim, st->kpad, dm_value_slices(st->feats[f])))
      return fail(MSC_EHIP, "k_dm_prepare launch failed");
  st->valid.prepared();
  return MSC_OK;
}

int msc::ensure_crp(msc_state *st) {
  MSC_TRY(ensure_raw(st));
  if (!st->valid.crp_stale()) return MSC_OK;
  if (launch_crp_prepare(st->ctx->stream, st->cnt_u32, st->K, st->kpad, st->alpha, st->logpc))
    return fail(MSC_EHIP, "k_crp_prepare launch failed");
  st->valid.crp_prepared();
  return MSC_OK;
}

// the raw tables lifted into the additive ones where those are stale: the features in their order, then the counts
// (niw lifts through its commit kernel run backwards)
int msc::ensure_additive(msc_state *st) {
  MSC_TRY(ensure_raw(st));
  hipStream_t s = st->ctx->stream;
  for (uint32_t f = 0; f < st->nfeat; f++)
    if (st->valid.additive_stale(f)) {
      const int rc = st->feats[f].family == MSC_NIW
                         ? launch_niw_commit(s, st->desc_dev, f, st->feats[f].dim, st->K, st->kpad, 0)
                         : launch_lift(s, st->desc_dev + f, 1, st->kpad, st->red_i64, st->cnt_u32, 0);
      if (rc) return fail(MSC_EHIP, "k_lift launch failed");
    }
  if (st->valid.counts_additive_stale() && launch_lift(s, st->desc_dev, 0, st->kpad, st->red_i64, st->cnt_u32, 1))
    return fail(MSC_EHIP, "k_lift launch failed");
  st->valid.additive_lifted();
  return MSC_OK;
}

// every table current: the reference's fields, the additive sums, the score constants, the CRP terms
int msc::ensure_all_current(msc_state *st) {
  MSC_TRY(ensure_additive(st));
  MSC_TRY(ensure_derived(st));
  return ensure_crp(st);
}

// ---------------------------------------------------------------------------
// hot path
// ---------------------------------------------------------------------------
// scalar families go through one fused kernel (scores summed over features in registers);
// every niw feature then adds its MFMA pass on top.

// the tables of the plan's fused bb runs follow their members' (whatever updated those -- prepare, commit, an entity op):
// rebuilt at the head of every call that scores with the fused plan, one small launch
// ... and so does what the plan's nich blocks go by (NichPlanInfo: is a block's c1 one number per group, how far a value may
// lie before a product of four could overflow) -- the same launch
int msc::refresh_fused_tables(msc_state *st) {
  const bool packed = stages_nich(st->plan.tile_path);
  if (!st->plan.fuse_any && !st->plan.nich_blocks_any && !packed) return MSC_OK;
  if (launch_fuse_tables(st->ctx->stream, st->desc_fuse_dev, (int)st->plan.fuse_split, (st->plan.nich_blocks_any || packed) ? (int)st->plan.fuse_nfeat : (int)st->plan.fuse_split, st->kpad))
    return fail(MSC_EHIP, "k_fuse_tables launch failed");
  return MSC_OK;
}

// what the narrow kernels of a partly filled last tile need (launchers.hpp); the packed-table scratch grows on demand
static int tail_plan(msc_state *st, TailPlan &tp, bool exact = true) {
  tp = TailPlan();
  tp.exact = exact;
  if (!(tp.ok = narrow_tail_fits(st->route))) return MSC_OK;
  MSC_HIP(grow_retained(st->retired, st->tail_pack, (size_t)st->plan.tail_pack_rows * 64));
  tp.masked_nich = st->plan.tail_masked_nich;
  tp.dm = st->plan.tail_dm;
  tp.max_rows = st->plan.tail_max_rows;
  tp.pack_rows = st->plan.tail_pack_rows;
  tp.pack = st->tail_pack;
  return MSC_OK;
}

// (called where a view has just been bound or the plan is made: bind_view and plan_groups leave bound_view current)
static bool gp_beyond_table(const msc_state *st, uint32_t f) {
  if (!st->bound_view || f >= st->bound_cols.size()) return false;
  const uint32_t c = st->bound_cols[f];
  if (is_count_family(st->feats[f].family)) return col_max_of(st, f, st->bound_view, c) >= (long long)kGpMaxTable;
  if (st->feats[f].family == MSC_DM)      // a row goes to the double path when its total is beyond the tables
    return !st->bound_view->dm_max[c].empty() && dm_max_of(st, f, st->bound_view, c, st->feats[f].dim) >= kGpMaxTable;
  return false;
}

// What the routes read of the state (route.hpp RouteFacts), as of this bind or plan: upload_desc is the one place that
// builds it, so a call walks no view metadata.  view_rows is the call's to refresh (route_facts_now).
static void refresh_route_facts(msc_state *st) {
  RouteFacts &rf = st->route;
  rf.K = st->K, rf.kpad = st->kpad, rf.num_cus = st->ctx->num_cus;
  rf.nich1 = st->nich1, rf.has_dm = st->has_dm, rf.n_niw = st->n_niw, rf.nfeat = st->nfeat;
  rf.plan = st->plan;
  rf.feats.resize(st->nfeat);
  for (uint32_t f = 0; f < st->nfeat; f++)
    rf.feats[f] = RouteFeat{st->feats[f].family, st->feats[f].dim, st->desc_host[f].vcap, gp_beyond_table(st, f)};
  rf.niw1_max_groups = sweep_niw1_max_groups(st->feats[0].dim);
  rf.nich1_rows_max_groups = sweep_nich1_rows_max_groups();
}
// The facts as a call routes on them, in this unit and the others.  view_rows: the rows the choice of kernels goes by --
// the bound view's, or those of the whole a sharded driver announced (msc_state_set_sweep_rows), never a call's (route_sweep)
const RouteFacts &msc::route_facts_now(msc_state *st) {
  st->route.view_rows = st->sweep_rows_hint ? st->sweep_rows_hint : st->bound_view ? st->bound_view->nrows : 0;
  return st->route;
}

// does any row's leave-one-out value need the formula paths (dm always; gp / bnb when the column holds counts beyond the table)?
static bool loo_needs_heavy(const msc_state *st) {
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const int fam = st->feats[f].family;
    // (a count family's table covers 0 .. the bound column's maximum unless that exceeds the cap; dm likewise, by row total)
    if ((is_count_family(fam) || fam == MSC_DM) && st->route.feats[f].beyond_table) return true;
  }
  return false;
}

// every row's leave-one-out value (its own group's score, the prior's when crp) into st->own.  The staged kernel (a plan
// with leave-one-out blocks in LDS, plan_groups) pays once the rows nearly fill the chip -- C3, 1M rows: 140 us staged, 196
// gathered; a 131k-row chunk: 0.33 ms against 0.03.  Both give a row the same bits (test_gpu_score.py::
// test_both_leave_one_out_kernels_give_a_row_the_same_bits), so the CALL's rows choose.
int msc::run_loo_own(msc_state *st, uint64_t row0, uint64_t nrows, const int32_t *z, bool crp) {
  const int lds = read_switches().loo_lds;
  const bool staged = st->plan.loo_staged != 0 && (lds < 0 ? nrows >= (uint64_t)kLooRows * kLooThreads * st->ctx->num_cus * 3 / 4 : lds != 0);
  MSC_HIP(grow_retained(st->retired, st->own, nrows));
  if (launch_loo_own(st->ctx->stream, loo_needs_heavy(st), staged, st->desc_tile_dev, (int)st->nfeat, st->K, st->kpad, row0, nrows, z,
                     crp ? st->logpc : nullptr, st->own))
    return fail(MSC_EHIP, "k_loo_own launch failed");
  return MSC_OK;
}

// k_score_nich1's launch shape for a pass of `nrows` x K into `out`: what msc_score_tune remembered for this very
// buffer, else for this size, else the default.  (profiles/r02_placement_study.txt: the shape moves the rate by <= 4 %
// either way; what decides between 5.6 and 7.0 TB/s is where the driver placed the buffer.)
static int nich1_shape_for(msc_context *ctx, const void *out, uint64_t nrows, uint32_t K) {
  // which stores the pass uses (bit 8 of the launch code: plain): what msc_score_tune found for this very buffer; else
  // non-temporal into a buffer this context placed and probed fast, plain into everything else (msc_context::placed)
  int plain = 1;
  for (const msc_context::Placed &p : ctx->placed)
    if (out >= p.base && static_cast<const char *>(out) < static_cast<const char *>(p.base) + p.size) plain = p.nt_fast ? 0 : 1;
  int shape = -1, by_size = -1;
  for (const msc_context::ShapeEntry &e : ctx->nich1_shapes) {
    if (e.nrows != nrows || e.K != K) continue;
    if (e.out == out) {
      shape = e.shape;
      if (e.plain_stores >= 0) plain = e.plain_stores;
      break;
    }
    if (by_size < 0) by_size = e.shape;
  }
  if (shape < 0) shape = by_size < 0 ? 0 : by_size;
  return shape | (plain ? 0x100 : 0);
}

int msc::run_score(msc_state *st, uint64_t row0, uint64_t nrows, const int32_t *z_dev, bool crp,
                   bool niw_f32, float *out_dev, uint64_t ld_out) {
  hipStream_t s = st->ctx->stream;
  const float *prior = crp ? st->logpc : nullptr;
  if (z_dev) MSC_TRY(run_loo_own(st, row0, nrows, z_dev, crp));
  ScoreRoute r = route_score(route_facts_now(st), read_switches(), nrows);
  if (!r.lanes && r.path == MSC_PATH_NICH1) r.shape.nich1 = nich1_shape_for(st->ctx, out_dev, nrows, st->K);
  if (r.lanes) {
    return launch_narrow(s, st->ctx->num_cus, r.lanes, r.table_rows, false, st->desc_dev, (int)st->nfeat, st->K, st->kpad, row0, nrows,
                         z_dev, st->own, prior, out_dev, ld_out, 0, nullptr, nullptr, ZeroSpans());
  }
  bool written = false;
  if (st->n_niw < st->nfeat || crp) {
    const bool nich1 = r.path == MSC_PATH_NICH1;
    TailPlan tail;
    if (!nich1) {
      MSC_TRY(tail_plan(st, tail));
      MSC_TRY(refresh_fused_tables(st));
    }
    MSC_TRY(launch_score(s, st->ctx->num_cus, r.path, tail, r.shape, nich1 ? st->desc_dev : st->desc_fuse_dev, (int)st->plan.fuse_nfeat,
                         (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows, z_dev, st->own, prior, out_dev, ld_out));
    written = true;
    for (uint32_t f = 0; f < st->nfeat; f++)
      if (st->route.feats[f].beyond_table &&
          launch_gp_large_fix(s, st->ctx->num_cus, st->desc_dev, (int)f, st->K, st->kpad, row0, nrows, z_dev, out_dev, ld_out))
        return fail(MSC_EHIP, "k_gp_large_fix launch failed");
  }
  for (uint32_t f = 0; f < st->nfeat; f++) {
    if (st->feats[f].family != MSC_NIW) continue;
    if (z_dev) MSC_HIP(grow_retained(st->retired, st->niw_qown, nrows));   // leave-one-out: the score kernel parks q of the own group here
    if (launch_niw_score(s, st->ctx->num_cus, st->desc_dev, f, st->feats[f].dim, st->K, st->kpad, row0, nrows, z_dev, written,
                         niw_f32, st->niw_qown, out_dev, ld_out))
      return fail(MSC_EHIP, "k_score_niw launch failed: %s", hipGetErrorString(hipGetLastError()));
    written = true;
  }
  return MSC_OK;
}

extern "C" int msc_score_value(msc_state *st, const msc_dataview *view, const uint32_t *cols,
                               uint64_t row0, uint64_t nrows, const int32_t *z_dev, uint32_t flags,
                               float *out_dev, uint64_t ld_out) {
  MSC_REQUIRE(st && (out_dev || nrows == 0), "null argument");    // an empty row range has no output to point at
  MSC_REQUIRE(ld_out >= st->K, "ld_out %llu < ngroups %u", (unsigned long long)ld_out, st->K);
  MSC_REQUIRE((flags & ~(MSC_SCORE_CRP_PRIOR | MSC_SCORE_NIW_F32)) == 0, "unknown flags 0x%x", flags);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  MSC_TRY(ensure_derived(st));
  const bool crp = (flags & MSC_SCORE_CRP_PRIOR) != 0;
  if (crp) MSC_TRY(ensure_crp(st));
  return run_score(st, row0, nrows, z_dev, crp, (flags & MSC_SCORE_NIW_F32) != 0, out_dev, ld_out);
}

// Settle the launch shape of the single-nich scoring pass for passes of this size: every shape of kNich1Shapes, one
// warm-up and six timed launches each into the caller's buffer (every run writes the same values), the fastest is
// remembered per context for (this buffer, nrows, K) and, as the fallback, for (nrows, K).  SYNCHRONOUS (~10 ms): it
// waits on events, so never call it on a capturing stream.  States that do not take the single-nich kernel return
// MSC_OK and remember nothing.
extern "C" int msc_score_tune(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                              uint64_t nrows, float *out_dev, uint64_t ld_out, int *shape_out, float *ms_out) {
  MSC_REQUIRE(st && view && out_dev, "null argument");
  MSC_REQUIRE(ld_out >= st->K, "ld_out %llu < ngroups %u", (unsigned long long)ld_out, st->K);
  if (shape_out) *shape_out = -1;
  if (ms_out) *ms_out = 0.f;
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  const ScoreRoute r = route_score(route_facts_now(st), read_switches(), nrows);
  if (r.lanes || r.path != MSC_PATH_NICH1 || nrows == 0) return MSC_OK;
  MSC_TRY(ensure_derived(st));
  hipStream_t s = st->ctx->stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(MSC_EINVAL, "msc_score_tune waits for the device: not on a capturing stream");
  auto launch = [&](int code) {
    return launch_score(s, st->ctx->num_cus, MSC_PATH_NICH1, TailPlan(), ScoreShape{8, false, LastTile::tiles, code}, st->desc_dev, 1, (int)st->plan.tile_split, st->K, st->kpad, row0,
                        nrows, nullptr, nullptr, nullptr, out_dev, ld_out);
  };
  hipEvent_t e0, e1;
  MSC_HIP(hipEventCreate(&e0));
  MSC_HIP(hipEventCreate(&e1));
  float best = 0.f;
  int shape = -1, rc = MSC_OK;
  for (int cand = 0; cand < kNich1NumShapes && rc == MSC_OK; cand++) {
    if ((rc = launch(cand)) != MSC_OK) break;
    hipError_t e = hipEventRecord(e0, s);
    for (int r = 0; r < 6 && e == hipSuccess; r++) (void)launch(cand);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) { rc = fail(MSC_EHIP, "timing failed: %s", hipGetErrorString(e)); break; }
    if (shape < 0 || ms < best) {
      best = ms;
      shape = cand;
    }
  }
  // ... and, with the winning shape, the stores: non-temporal or plain (which is faster depends on where the buffer lies)
  int plain_stores = 0;
  if (rc == MSC_OK && shape >= 0) {
    float ms_kind[2] = {0.f, 0.f};
    for (int kind = 0; kind < 2 && rc == MSC_OK; kind++) {
      const int code = shape | (kind ? 0x100 : 0);
      if ((rc = launch(code)) != MSC_OK) break;
      hipError_t e = hipEventRecord(e0, s);
      for (int r = 0; r < 6 && e == hipSuccess; r++) (void)launch(code);
      if (e == hipSuccess) e = hipEventRecord(e1, s);
      if (e == hipSuccess) e = hipEventSynchronize(e1);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms_kind[kind], e0, e1);
      if (e != hipSuccess) rc = fail(MSC_EHIP, "timing failed: %s", hipGetErrorString(e));
    }
    plain_stores = ms_kind[1] < ms_kind[0] ? 1 : 0;
    best = ms_kind[plain_stores];
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  MSC_TRY(rc);
  auto &memo = st->ctx->nich1_shapes;
  for (size_t i = 0; i < memo.size();)                      // one entry per (buffer, size); the newest size entry leads
    if (memo[i].out == out_dev && memo[i].nrows == nrows && memo[i].K == st->K) memo.erase(memo.begin() + i);
    else i++;
  memo.insert(memo.begin(), msc_context::ShapeEntry{out_dev, nrows, st->K, shape, plain_stores});
  if (memo.size() > 16) memo.pop_back();
  if (shape_out) *shape_out = shape;
  if (ms_out) *ms_out = best / 6.f;
  return MSC_OK;
}

int msc::commit(msc_state *st) {
  MSC_TRY(launch_commit_all(st));
  st->valid.committed();
  return MSC_OK;
}

static int commit_and_prepare(msc_state *st, bool bump_rng = true) {
  hipStream_t s = st->ctx->stream;
  if (launch_commit_prepare(s, st->desc_dev, (int)st->nfeat, st->K, st->kpad, st->red_i64, st->cnt_u32, st->alpha,
                            st->logpc, bump_rng ? st->rng_dev : nullptr, prepare_value_slices(st)))
    return fail(MSC_EHIP, "k_commit_prepare launch failed");
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const msc_feature_host &h = st->feats[f];
    if (h.family == MSC_NIW && (launch_niw_commit(s, st->desc_dev, f, h.dim, st->K, st->kpad, 1) ||
                                launch_niw_prepare(s, st->desc_dev, f, h.dim, st->K, st->kpad)))
      return fail(MSC_EHIP, "niw commit / prepare launch failed");
    if (h.family == MSC_DM && st->desc_host[f].dm_meta != nullptr &&
        launch_dm_prepare(s, st->desc_dev, (int)f, h.dim, st->kpad, dm_value_slices(h)))
      return fail(MSC_EHIP, "k_dm_prepare launch failed");
  }
  st->valid.committed_and_prepared();
  return MSC_OK;
}

int msc::accumulate_impl(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                         uint64_t nrows, const int32_t *z_dev, uint32_t flags) {
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  hipStream_t s = st->ctx->stream;
  if (flags & MSC_ACC_RESET) {
    if (!(flags & kAccZeroed) && launch_zero64(s, st->red_i64, st->n_i64, st->red_f64, st->n_f64))
      return fail(MSC_EHIP, "k_zero64 launch failed");
    st->valid.additive_lifted();                            // (zeroed: what this call sums into)
  } else {
    MSC_TRY(ensure_additive(st));
  }
  if (nrows > 0) {
    const int rc = launch_accumulate(s, st->ctx->num_cus, st->desc_acc_dev, st->desc_acc_host.data(), (int)st->desc_acc_host.size(),
                                     st->K, st->kpad, row0, nrows, z_dev,
                                     (flags & MSC_ACC_SUBTRACT) ? -1 : 1, st->red_i64);
    if (rc == -2) return fail(MSC_EUNSUPPORTED, "accumulate tables for %u groups exceed LDS", st->K);
    if (rc) return fail(MSC_EHIP, "k_accumulate launch failed: %s", hipGetErrorString(hipGetLastError()));
    for (uint32_t f = 0; f < st->nfeat; f++) {
      if (st->feats[f].family != MSC_NIW) continue;
      MSC_REQUIRE(nrows < (1ull << 32), "niw accumulate takes at most 2^32 - 1 rows per call");
      MSC_HIP(grow_retained(st->retired, st->niw_scratch, 2 * (size_t)st->K + 1 + (size_t)nrows));
      if (launch_niw_accumulate(s, st->ctx->num_cus, st->desc_dev, f, st->K, row0, nrows, z_dev,
                                (flags & MSC_ACC_SUBTRACT) ? -1 : 1, st->niw_scratch, st->feats[f].dim))
        return fail(MSC_EHIP, "niw accumulate launch failed");
    }
  }
  st->valid.accumulated();
  if (flags & kAccThenPrepare) return commit_and_prepare(st);
  if (!(flags & MSC_ACC_NO_COMMIT)) MSC_TRY(commit(st));
  return MSC_OK;
}

extern "C" int msc_accumulate(msc_state *st, const msc_dataview *view, const uint32_t *cols,
                              uint64_t row0, uint64_t nrows, const int32_t *z_dev, uint32_t flags) {
  MSC_REQUIRE(st && (z_dev || nrows == 0), "null argument");
  MSC_REQUIRE((flags & ~(MSC_ACC_RESET | MSC_ACC_SUBTRACT | MSC_ACC_NO_COMMIT)) == 0, "unknown flags 0x%x", flags);
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  return accumulate_impl(st, view, cols, row0, nrows, z_dev, flags);
}

extern "C" int msc_entity_op(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row, uint32_t group,
                             int sign, int32_t *z_dev) {
  MSC_REQUIRE(st && view, "null argument");
  MSC_REQUIRE(sign != 0, "sign must be +1 (join) or -1 (leave)");
  MSC_REQUIRE(group < st->K, "group %u outside [0,%u)", group, st->K);
  MSC_TRY(refuse_mid_step(st, "msc_entity_op"));
  MSC_TRY(device_error_check(st->ctx));
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(bind_view(st, view, cols, row, 1));
  hipStream_t s = st->ctx->stream;
  bool scalar_only = true;
  for (const auto &h : st->feats) scalar_only &= h.family != MSC_NIW && h.family != MSC_DM;
  if (!scalar_only) {
    // general path: the group travels through a one-entry assignment vector of the state's own
    if (!st->one_z) MSC_TRY(alloc_zeroed(st->one_z, 1));
    if (launch_set_i32(s, st->one_z, (int32_t)group)) return fail(MSC_EHIP, "k_set_i32 launch failed");
    MSC_TRY(accumulate_impl(st, view, cols, row, 1, st->one_z, sign < 0 ? (uint32_t)MSC_ACC_SUBTRACT : 0u));
    if (z_dev && launch_set_i32(s, z_dev + row, sign > 0 ? (int32_t)group : -1)) return fail(MSC_EHIP, "k_set_i32 launch failed");
    return MSC_OK;
  }
  // every table current before, every table current after
  MSC_TRY(ensure_all_current(st));
  if (launch_entity_op(s, st->desc_dev, (int)st->nfeat, st->K, st->kpad, row, group, sign > 0 ? 1 : -1, st->red_i64, st->cnt_u32,
                       st->alpha, st->logpc, z_dev ? z_dev + row : nullptr))
    return fail(MSC_EHIP, "k_entity_op launch failed");
  st->valid.kept_current();
  return MSC_OK;
}

extern "C" int msc_score_data(msc_state *st, float *out_dev) {
  MSC_REQUIRE(st && out_dev, "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(ensure_raw(st));
  if (launch_score_data(st->ctx->stream, st->desc_dev, (int)st->nfeat, st->K, st->kpad, out_dev))
    return fail(MSC_EHIP, "k_score_data launch failed");
  if (st->n_niw) {
    MSC_TRY(ensure_derived(st));   // ln det Psi_n comes from the prepare step
    for (uint32_t f = 0; f < st->nfeat; f++)
      if (st->feats[f].family == MSC_NIW &&
          launch_niw_score_data(st->ctx->stream, st->desc_dev, f, st->K, st->kpad, out_dev))
        return fail(MSC_EHIP, "k_niw_score_data launch failed");
  }
  return MSC_OK;
}

// the sampling kernels read (seed, sweep) from the state's device pair and the step ends by incrementing the sweep
// index there, so consecutive sweeps need no host -> device traffic (and replay as a graph, msc_sweep_step)
// `zeroed` non-null = part of a sweep step: the fused kernels also empty the additive tables for the accumulate pass
// that follows (*zeroed says whether one did), and the increment of the sweep index is left to that pass's tail.
int msc::sweep_assign_impl(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                           uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep,
                           bool *zeroed) {
  MSC_TRY(bind_view(st, view, cols, row0, nrows));
  if (nrows == 0) return MSC_OK;
  if (!st->rng.holds(seed, sweep)) {
    if (launch_rng_set(st->ctx->stream, st->rng_dev, seed, sweep)) return fail(MSC_EHIP, "k_rng_set launch failed");
    st->rng.set(seed, sweep);
  }
  MSC_TRY(ensure_derived(st));
  MSC_TRY(ensure_crp(st));
  hipStream_t s = st->ctx->stream;
  const int cus = st->ctx->num_cus;
  ZeroSpans zero;
  if (zeroed) {
    zero.a = reinterpret_cast<unsigned long long *>(st->red_i64.get()); zero.na = st->n_i64;
    zero.b = reinterpret_cast<unsigned long long *>(st->red_f64.get()); zero.nb = st->n_f64;
  }
  const SweepRoute r = route_sweep(route_facts_now(st), read_switches(), nrows);
  bool zeroes = true;                                   // the kernel emptied the additive tables on its way (with `zeroed`)
  switch (r.kind) {                                     // (the launchers report their own failures)
    case SweepKind::niw1:
      MSC_TRY(launch_sweep_niw1(s, cus, st->feats[0].dim, st->desc_dev, st->K, st->kpad, row0, nrows, row_id0, z_dev, st->logpc, st->rng_dev, zero));
      break;
    case SweepKind::nich1_rows:
      MSC_HIP(grow_retained(st->retired, st->rows_table, sweep_nich1_rows_table_floats(st->kpad)));
      MSC_TRY(launch_sweep_nich1_rows(s, cus, st->desc_dev, st->K, st->kpad, row0, nrows, row_id0, z_dev, st->logpc, st->rng_dev, zero, st->rows_table));
      break;
    case SweepKind::nich1:                                // (the single-nich kernel computes the own-group values itself)
      MSC_TRY(launch_sweep_nich1(s, cus, r.transposed, st->desc_dev, st->K, st->kpad, row0, nrows, row_id0, z_dev, st->own, st->logpc, st->rng_dev, zero));
      break;
    case SweepKind::narrow:
      MSC_TRY(run_loo_own(st, row0, nrows, z_dev, true));
      MSC_TRY(launch_narrow(s, cus, r.lanes, r.table_rows, true, st->desc_dev, (int)st->nfeat, st->K, st->kpad, row0, nrows, z_dev,
                            st->own, st->logpc, nullptr, 0, row_id0, z_dev, st->rng_dev, zero));
      break;
    case SweepKind::mixed:
      MSC_TRY(run_loo_own(st, row0, nrows, z_dev, true));
      MSC_TRY(refresh_fused_tables(st));                  // (these walk the fused plan)
      MSC_TRY(launch_sweep_mixed(s, cus, st->has_dm, st->plan.tile_path, r.shape, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows, row_id0, z_dev, st->own, st->logpc, st->rng_dev, zero));
      break;
    case SweepKind::rows:
    case SweepKind::rows_sampler: {
      MSC_TRY(run_loo_own(st, row0, nrows, z_dev, true));
      MSC_TRY(refresh_fused_tables(st));
      TailPlan tail;
      MSC_TRY(tail_plan(st, tail, false));
      if (r.kind == SweepKind::rows) {
        MSC_TRY(launch_sweep_rows(s, cus, tail, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows, row_id0,
                                  z_dev, st->own, st->logpc, st->rng_dev, zero));
        break;
      }
      MSC_HIP(grow_retained(st->retired, st->tail_scores, ((size_t)nrows + 16) * 128));
      MSC_TRY(launch_score_tail(s, cus, tail, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, 0, row0, nrows,
                                z_dev, st->own, st->logpc, st->tail_scores, 128));
      if (launch_sample_rows(s, cus, st->tail_scores, 128, st->K, nrows, row_id0, z_dev, st->rng_dev)) return fail(MSC_EHIP, "k_sample_rows launch failed");
      zeroes = false;                                     // (nothing emptied the additive tables on the way)
      break;
    }
    case SweepKind::roles_tail: {
      MSC_TRY(refresh_fused_tables(st));
      MSC_TRY(run_loo_own(st, row0, nrows, z_dev, true));
      MSC_HIP(grow_retained(st->retired, st->tail_scores, ((size_t)nrows + 16) * r.tail_ld));
      // (the kernel stores at out + row * ld + k: handing it tail_scores - 256 puts group 256 + j at column j; one sum per
      // group: nothing else scores these groups for a draw)
      TailPlan tail;
      MSC_TRY(tail_plan(st, tail, false));
      MSC_TRY(r.tail_pair ? launch_score_pair_tail(s, cus, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows,
                                                   z_dev, st->own, st->logpc, st->tail_scores, r.tail_ld)
                          : launch_score_tail(s, cus, tail, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad,
                                              kGroupTile, row0, nrows, z_dev, st->own, st->logpc, st->tail_scores - kGroupTile, r.tail_ld));
      MSC_TRY(launch_sweep_roles_tail(s, cus, st->plan.tile_path, st->desc_fuse_dev, (int)st->plan.fuse_nfeat, (int)st->plan.fuse_split, st->K, st->kpad, row0, nrows,
                                      row_id0, z_dev, st->own, st->logpc, st->rng_dev, zero, st->tail_scores));
      break;
    }
    case SweepKind::generic: {
      // score a chunk of rows (leave-one-out + prior) into scratch, then sample it (the chunk: route_calls.hpp score_chunk)
      const auto [ld, chunk] = score_chunk(st->K, st->kpad, nrows);
      MSC_HIP(grow_retained(st->retired, st->scratch, chunk * ld));
      for (uint64_t at = 0; at < nrows; at += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, nrows - at);
        MSC_TRY(run_score(st, row0 + at, n, z_dev + at, true, false, st->scratch, ld));
        if (launch_sample_rows(s, cus, st->scratch, ld, st->K, n, row_id0 + at, z_dev + at, st->rng_dev))
          return fail(MSC_EHIP, "k_sample_rows launch failed");
      }
      zeroes = false;
      break;
    }
  }
  if (zeroed) {
    *zeroed = zeroes;
    return MSC_OK;
  }
  if (launch_rng_bump(s, st->rng_dev)) return fail(MSC_EHIP, "k_rng_bump launch failed");
  st->rng.advanced();
  return MSC_OK;
}

extern "C" int msc_sweep_assign(msc_state *st, const msc_dataview *view, const uint32_t *cols,
                                uint64_t row0, uint64_t nrows, uint64_t row_id0, int32_t *z_dev,
                                uint64_t seed, uint64_t sweep) {
  MSC_REQUIRE(st && (z_dev || nrows == 0), "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  return sweep_assign_impl(st, view, cols, row0, nrows, row_id0, z_dev, seed, sweep);
}

// ---------------------------------------------------------------------------
// One whole single-process sweep step: assign, then rebuild the tables from the new assignment
// (msc_sweep_assign + msc_accumulate(RESET), commit included).  On small problems the step is a dozen
// launches of a few microseconds each and the gaps between them are the cost, so its steady state -- same
// view, rows and assignment vector, consecutive sweep indices -- is captured once as a HIP graph and replayed.
// ---------------------------------------------------------------------------
extern "C" int msc_sweep_step(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                              uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep) {
  MSC_REQUIRE(st && view && (z_dev || nrows == 0), "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  hipStream_t s = st->ctx->stream;
  st->valid.step_began();
  auto eager = [&]() -> int {
    st->step_graph.n_eager++;
    bool zeroed = false;
    MSC_TRY(sweep_assign_impl(st, view, cols, row0, nrows, row_id0, z_dev, seed, sweep, &zeroed));
    st->rng.tail_owes();                                // (until the tail has moved the device's pair on)
    MSC_TRY(accumulate_impl(st, view, cols, row0, nrows, z_dev,
                            MSC_ACC_RESET | kAccThenPrepare | (zeroed ? (uint32_t)kAccZeroed : 0u)));
    st->rng.tail_paid();
    return MSC_OK;
  };
  MSC_TRY(bind_view(st, view, cols, row0, nrows));       // (uploads and waits if the binding changed: never inside a capture)
  msc_state::StepGraph &g = st->step_graph;
  // Replay is opt-in: on ROCm 7.2 / MI355X a graph launch of the step's 3-5 kernels measured 4-5 us SLOWER than
  // launching them (27 -> 32 us at N = 10k), and instantiation costs milliseconds (sweep step).
  StepInputs in{read_switches().sweep_graph, g.disabled, g.exec != nullptr};
  if (nrows == 0) return accumulate_impl(st, view, cols, row0, 0, z_dev, MSC_ACC_RESET);   // (no row draws anything)
  StepKey key;
  TableValidity::Snapshot entry;   // (which device tables are current: a captured step must leave them, and the pair, as it found them)
  if (in.graph_on && !in.disabled) {                    // (the rule reads nothing else otherwise: a plain step builds no key)
    key = {view, z_dev, view->serial, row0, nrows, row_id0, st->alpha, std::vector<uint32_t>(st->nfeat)};
    for (uint32_t f = 0; f < st->nfeat; f++) key.cols[f] = cols ? cols[f] : f;
    entry = st->valid.snapshot();
    in.same_key = key == g.key;
    in.seen = g.seen;
    in.holds = st->rng.holds(seed, sweep);
    in.flags_equal = entry == g.flags;
    in.fused = sweep_is_fused(st->route);
  }
  switch (step_action(in)) {                            // (step_rules.hpp)
    case StepAction::eager:
      return eager();
    case StepAction::rekey:
      drop_step_graph(st);
      g.key = std::move(key);
      g.seen = 0;
      [[fallthrough]];
    case StepAction::count:
      g.seen++;
      return eager();
    case StepAction::replay:
      MSC_HIP(hipGraphLaunch(g.exec, s));
      g.n_replayed++;
      st->rng.advanced();
      return MSC_OK;
    case StepAction::capture:
      break;
  }
  // record on the library's own stream (the caller's may be the null stream), replay on the caller's
  msc_context *ctx = st->ctx;
  if (!ctx->record_stream && hipStreamCreateWithFlags(&ctx->record_stream, hipStreamNonBlocking) != hipSuccess)
    ctx->record_stream = nullptr;
  if (!ctx->record_stream || hipStreamBeginCapture(ctx->record_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    g.disabled = true;
    return eager();
  }
  const RngMirror rng_entry = st->rng.snapshot();
  ctx->stream = ctx->record_stream;
  const int rc = eager();
  ctx->stream = s;
  g.n_eager--;                      // (recorded, not run)
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(ctx->record_stream, &graph);
  // (the mirror by validity alone: a recorded step legitimately moves the sweep index on)
  bool ok = rc == MSC_OK && ec == hipSuccess && graph != nullptr && st->valid.snapshot() == entry &&
            st->rng.valid() == rng_entry.valid();
  if (ok && hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    g.exec = nullptr;
    ok = false;
  }
  if (graph) (void)hipGraphDestroy(graph);
  if (!ok) {
    // nothing of the captured step has run: put the host's view of the state back and run the step as it is.  (The
    // mirror whole: a recorded step reports tail_owes and tail_paid alone -- the pair held at entry, so nothing set it,
    // and only msc_sweep_step_begin defers -- so validity and the sweep index are all that can differ.)
    (void)hipGetLastError();
    drop_step_graph(st);
    g.disabled = true;
    st->valid.restore(entry);
    st->rng.restore(rng_entry);
    return eager();
  }
  g.flags = entry;
  MSC_HIP(hipGraphLaunch(g.exec, s));
  g.n_replayed++;
  return MSC_OK;
}

// The row-sharded form of the step: everything up to the exchange.  msc_sweep_assign + msc_accumulate(RESET | NO_COMMIT)
// with the step's fusions (the sweep kernel empties the additive tables; the sweep index moves on in the commit);
// the caller all-reduces msc_state_reduce_buffers and calls msc_state_commit_reduce.
extern "C" int msc_sweep_step_begin(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                    uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep) {
  MSC_REQUIRE(st && view && (z_dev || nrows == 0), "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  if (nrows == 0) return accumulate_impl(st, view, cols, row0, 0, z_dev, MSC_ACC_RESET | MSC_ACC_NO_COMMIT);
  bool zeroed = false;
  MSC_TRY(sweep_assign_impl(st, view, cols, row0, nrows, row_id0, z_dev, seed, sweep, &zeroed));
  st->rng.deferred();                                   // (until the commit has moved the device's pair on)
  return accumulate_impl(st, view, cols, row0, nrows, z_dev,
                         MSC_ACC_RESET | MSC_ACC_NO_COMMIT | (zeroed ? (uint32_t)kAccZeroed : 0u));
}

extern "C" int msc_sweep_step_stats(const msc_state *st, uint64_t *eager_steps, uint64_t *graph_steps) {
  MSC_REQUIRE(st, "null argument");
  if (eager_steps) *eager_steps = st->step_graph.n_eager;
  if (graph_steps) *graph_steps = st->step_graph.n_replayed;
  return MSC_OK;
}

extern "C" int msc_state_reduce_buffers(msc_state *st, void **dev_i64, size_t *n_i64, void **dev_f64,
                                        size_t *n_f64) {
  MSC_REQUIRE(st, "null state");
  if (dev_i64) *dev_i64 = st->red_i64;
  if (n_i64) *n_i64 = st->n_i64;
  if (dev_f64) *dev_f64 = st->red_f64;
  if (n_f64) *n_f64 = st->n_f64;
  return MSC_OK;
}

// the same tables as ONE float64 buffer, for a collective that takes one dtype (counts ride along as doubles: exact
// below 2^53): pack -> all-reduce *pack_dev -> unpack -> msc_state_commit_reduce.  One launch each.
extern "C" int msc_state_reduce_pack(msc_state *st, void **pack_dev, size_t *n_f64) {
  MSC_REQUIRE(st && pack_dev, "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  if (!st->red_pack) MSC_TRY(alloc_zeroed(st->red_pack, st->n_i64 + st->n_f64));
  if (launch_pack64(st->ctx->stream, false, st->red_i64, st->n_i64, st->red_f64, st->n_f64, st->red_pack))
    return fail(MSC_EHIP, "k_pack64 launch failed");
  *pack_dev = st->red_pack;
  if (n_f64) *n_f64 = st->n_i64 + st->n_f64;
  return MSC_OK;
}
extern "C" int msc_state_reduce_unpack(msc_state *st) {
  MSC_REQUIRE(st, "null state");
  st->valid.additive_rewritten();
  MSC_REQUIRE(st->red_pack, "msc_state_reduce_unpack before msc_state_reduce_pack");
  MSC_HIP(hipSetDevice(st->ctx->device));
  if (launch_pack64(st->ctx->stream, true, st->red_i64, st->n_i64, st->red_f64, st->n_f64, st->red_pack))
    return fail(MSC_EHIP, "k_unpack64 launch failed");
  return MSC_OK;
}

// A sweep chooses between the lane <-> row kernel and the tile kernels by ROW COUNT (sweep_rows_pays), and the two sum a
// row's features in different float associations: a shard must choose what the whole would, or a dart may cross a CDF
// step.  By default the count is the bound view's -- right for row ranges of one view.  A driver that gives every rank a
// view of its own shard (common_amd/dist.py ShardedSweep, msc_sweep_step_sharded callers) states the rows of the WHOLE
// here, once; 0 = back to the view's count.
extern "C" int msc_state_set_sweep_rows(msc_state *st, uint64_t global_rows) {
  MSC_REQUIRE(st, "null state");
  // (the hint chooses kernels -- lane <-> row or tile, PAIR mode, the narrow tiling -- for every view the state scores:
  // a captured step holds the old choice, and replaying it would draw other bits than the whole does.  ADVICE r04)
  if (st->sweep_rows_hint != global_rows) drop_step_graph(st);
  st->sweep_rows_hint = global_rows;
  return MSC_OK;
}

// The same for the kernels' TABLES: a count / dm feature's exact tables cover 0 .. the bound view's column maximum, and
// that maximum decides the plan (table sizes, group packing, sentinel columns, lookup or generic kind, the kernel path,
// the narrow and lane <-> row kernels, the generic sweep past kGpMaxTable).  A shard's maxima are not the whole's, so a
// driver that gives every rank a view of its own reads each view's bounds (msc_state_col_bounds), takes the
// elementwise MAX across ranks and installs it on every rank (msc_state_set_col_bounds): every shard then plans as the
// whole does.  The state uses max(view's own, given) everywhere; NULL / 0 restores the view's alone.
extern "C" int msc_state_col_bounds(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint32_t *out, size_t n) {
  MSC_REQUIRE(st && view, "null argument");
  const size_t want = col_bounds_size(st);
  MSC_REQUIRE(n == want, "the state's features take %zu column bounds (got %zu)", want, n);
  MSC_REQUIRE(out || n == 0, "null argument");
  MSC_HIP(hipSetDevice(st->ctx->device));
  MSC_TRY(device_error_check(st->ctx));
  MSC_TRY(bind_view(st, view, cols, 0, 0));              // (finds the maxima the binding needs, once per view)
  size_t k = 0;
  for (uint32_t f = 0; f < st->nfeat; f++) {
    const uint32_t c = st->bound_cols[f];
    if (is_count_family(st->feats[f].family)) out[k++] = (uint32_t)std::max(view->col_max[c], 0ll);
    else if (st->feats[f].family == MSC_DM)
      for (uint32_t i = 0; i <= st->feats[f].dim; i++) out[k++] = view->dm_max[c][i];
  }
  return MSC_OK;
}

extern "C" int msc_state_set_col_bounds(msc_state *st, const uint32_t *bounds, size_t n) {
  MSC_REQUIRE(st, "null state");
  const size_t want = col_bounds_size(st);
  MSC_REQUIRE(n == 0 || n == want, "the state's features take %zu column bounds (got %zu)", want, n);
  MSC_REQUIRE(bounds || n == 0, "null bounds");
  std::vector<std::vector<uint32_t>> nb;
  if (n != 0) {
    nb.resize(st->nfeat);
    for (uint32_t f = 0, k = 0; f < st->nfeat; f++) {
      nb[f].assign(bounds + k, bounds + k + col_bound_count(st, f));
      k += (uint32_t)col_bound_count(st, f);
    }
  }
  if (nb == st->col_bounds) return MSC_OK;
  drop_step_graph(st);   // (a captured step holds the kernels and table sizes of the old plan: ADVICE r04, as for msc_state_set_sweep_rows)
  st->col_bounds = std::move(nb);
  st->rebind = true;
  return MSC_OK;
}

extern "C" int msc_state_commit_reduce(msc_state *st) {
  MSC_REQUIRE(st, "null state");
  MSC_HIP(hipSetDevice(st->ctx->device));
  // (what follows a reduce is the next sweep's scoring: commit and prepare in one launch, as in msc_sweep_step)
  const bool bump = st->rng.mid_step();
  MSC_TRY(commit_and_prepare(st, bump));
  if (bump) st->rng.deferred_paid();
  return MSC_OK;
}

extern "C" int msc_relation_blocks(msc_context *ctx, uint32_t ndim, const uint64_t *shape,
                                   const int32_t *const *z_dev, const uint32_t *ngroups,
                                   const uint32_t *positions_dev, uint64_t ncells, int32_t *z_cell_dev) {
  MSC_REQUIRE(ctx && shape && z_dev && ngroups, "null argument");
  MSC_REQUIRE(ndim >= 1 && ndim <= 8, "a relation has 1..8 dimensions (got %u)", ndim);
  MSC_REQUIRE(z_cell_dev || ncells == 0, "null output");
  unsigned long long total = 1, blocks = 1;
  for (uint32_t d = 0; d < ndim; d++) {
    MSC_REQUIRE(shape[d] > 0 && z_dev[d] && ngroups[d] > 0, "dimension %u: empty shape, null assignment or no groups", d);
    total *= shape[d];
    blocks *= ngroups[d];
    MSC_REQUIRE(blocks <= (1ull << 31) - 1, "more than 2^31 - 1 blocks");
  }
  MSC_REQUIRE(positions_dev || ncells == total, "a dense relation of this shape has %llu cells, not %llu", total,
              (unsigned long long)ncells);
  MSC_HIP(hipSetDevice(ctx->device));
  if (launch_relation_blocks(ctx->stream, ndim, shape, z_dev, ngroups, positions_dev, ncells, z_cell_dev))
    return fail(MSC_EHIP, "k_relation_blocks launch failed");
  return MSC_OK;
}

extern "C" int msc_relation_slice_scores(msc_context *ctx, const float *scores_dev, uint64_t ld, uint32_t ndim,
                                         const uint64_t *shape, uint32_t dim, const uint32_t *seg_dev,
                                         const uint32_t *ids_dev, const int32_t *off_dev, uint32_t ncand,
                                         uint32_t cand_stride, uint64_t nent, float *out_dev, uint64_t ld_out) {
  MSC_REQUIRE(ctx && shape && off_dev, "null argument");
  MSC_REQUIRE(ndim >= 1 && ndim <= 8 && dim < ndim, "dimension %u of a %u-dimensional relation", dim, ndim);
  MSC_REQUIRE((seg_dev == nullptr) == (ids_dev == nullptr), "seg_dev and ids_dev come together (sparse) or not at all (dense)");
  MSC_REQUIRE(nent == 0 || ncand == 0 || (scores_dev && out_dev), "null scores / output");
  MSC_REQUIRE(ld_out >= ncand, "ld_out %llu < candidates %u", (unsigned long long)ld_out, ncand);
  MSC_REQUIRE(ncand == 0 || (uint64_t)(ncand - 1) * cand_stride < ld, "candidate %u x stride %u runs past the score row (%llu)",
              ncand, cand_stride, (unsigned long long)ld);
  for (uint32_t d = 0; d < ndim; d++) MSC_REQUIRE(shape[d] > 0, "dimension %u is empty", d);
  MSC_REQUIRE(seg_dev != nullptr || nent <= shape[dim], "%llu entities on a dimension of %llu", (unsigned long long)nent,
              (unsigned long long)shape[dim]);
  MSC_REQUIRE(nent < (1ull << 31), "too many entities for one launch");
  MSC_HIP(hipSetDevice(ctx->device));
  MSC_TRY(device_error_check(ctx));
  if (launch_relation_slice_scores(ctx->stream, scores_dev, ld, ndim, shape, dim, seg_dev, ids_dev, off_dev, ncand, cand_stride,
                                   nent, out_dev, ld_out))
    return fail(MSC_EHIP, "k_relation_slice_scores launch failed");
  return MSC_OK;
}

extern "C" int msc_value_op_single(msc_context *ctx, int family, uint32_t dim, int op,
                                   const float *host_hp, void *host_ss, const void *host_value,
                                   float *score) {
  MSC_REQUIRE(ctx, "null context");
  MSC_REQUIRE(family_ok(family), "unknown family %d", family);
  MSC_REQUIRE(op >= MSC_OP_ADD && op <= MSC_OP_SCORE_DATA, "unknown op %d", op);
  if (family == MSC_NOOP) {           // models/noop.hpp:13-27: nothing to compute, nothing to launch
    if (score) *score = 0.f;
    return MSC_OK;
  }
  MSC_REQUIRE(host_hp && host_ss, "null hp / suff-stats");
  MSC_REQUIRE(op == MSC_OP_SCORE_DATA || host_value, "null value");
  MSC_REQUIRE(op <= MSC_OP_REMOVE || score, "null score");
  if (family == MSC_DD) MSC_REQUIRE(dim >= 1 && dim <= kMaxDDDim, "dd dim %u outside 1..%u", dim, kMaxDDDim);
  if (family == MSC_NIW) MSC_REQUIRE(dim >= 1 && dim <= kMaxNiwDim, "niw dim %u outside 1..%u", dim, kMaxNiwDim);
  if (family == MSC_DM) MSC_REQUIRE(dim >= 1 && dim <= kMaxDDDim, "dm categories %u outside 1..%u", dim, kMaxDDDim);
  const size_t hp_bytes = msc_hp_floats(family, dim) * sizeof(float), ss_bytes = msc_ss_bytes(family, dim);
  const size_t v_bytes = (family == MSC_BB || family == MSC_BBNC) ? 1 : (family == MSC_NIW || family == MSC_DM) ? 4 * (size_t)dim : 4;
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  MailboxHeader hd;
  hd.family = family; hd.dim = (int32_t)dim; hd.op = op; hd.status = 0; hd.score = 0.f;
  hd.hp_off = 64;
  hd.ss_off = (uint32_t)up16(hd.hp_off + hp_bytes);
  hd.value_off = (uint32_t)up16(hd.ss_off + ss_bytes);
  MSC_REQUIRE(hd.value_off + v_bytes <= ctx->mailbox_host.size(), "record too large for the mailbox");
  if (family == MSC_DD && host_value && op != MSC_OP_SCORE_DATA) {
    int32_t v;
    std::memcpy(&v, host_value, 4);
    MSC_REQUIRE(v >= 0 && (uint32_t)v < dim, "dd value %d outside [0,%u)", v, dim);
  }
  MSC_HIP(hipSetDevice(ctx->device));
  unsigned char *mb = static_cast<unsigned char *>(ctx->mailbox_host);
  std::memcpy(mb, &hd, sizeof hd);
  std::memcpy(mb + hd.hp_off, host_hp, hp_bytes);
  std::memcpy(mb + hd.ss_off, host_ss, ss_bytes);
  if (host_value) std::memcpy(mb + hd.value_off, host_value, v_bytes);
  if (launch_value_op(ctx->stream, ctx->mailbox_dev, dim, family))
    return fail(MSC_EHIP, "k_value_op launch failed: %s", hipGetErrorString(hipGetLastError()));
  // the kernel's last act is status = 1 in this (pinned, host-coherent) mailbox: watching for it costs a PCIe write's
  // latency, waking up from hipStreamSynchronize several microseconds more.  Bounded: the stream wait is the fallback.
  {
    volatile int32_t *flag = &reinterpret_cast<volatile MailboxHeader *>(mb)->status;
    bool seen = false;
    for (int spin = 0; spin < 200000 && !seen; spin++) seen = *flag == 1;
    if (seen) std::atomic_thread_fence(std::memory_order_acquire);
    else MSC_HIP(hipStreamSynchronize(ctx->stream));
  }
  MailboxHeader back;
  std::memcpy(&back, mb, sizeof back);
  if (back.status != 1) return fail(MSC_EHIP, "k_value_op did not complete");
  if (op <= MSC_OP_REMOVE) std::memcpy(host_ss, mb + hd.ss_off, ss_bytes);
  else *score = back.score;
  return MSC_OK;
}
