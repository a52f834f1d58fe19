// dev_buf.hpp -- the one owner of the host library's HIP allocations (device memory, or pinned host memory), the two
// ways a buffer of a state grows, and the one way a table filled on the host goes up (StagedUpload).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <vector>

namespace msc {

struct DeviceMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  void operator()(void *p) const { (void)hipFree(p); }
};
template <unsigned Flags>   // hipHostMalloc's
struct PinnedMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  void operator()(void *p) const { (void)hipHostFree(p); }
};

// A move-only allocation of n elements of T, freed when its owner goes.  It reads as the raw pointer it holds, which is
// what kernel arguments and the kernels' descriptors (FeatDesc) take.
template <typename T, typename Mem = DeviceMem>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(std::move(o.p_)), n_(o.n_) { o.n_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    p_ = std::move(o.p_);
    n_ = o.n_;
    o.n_ = 0;
    return *this;
  }

  operator T *() const { return p_.get(); }
  T *get() const { return p_.get(); }
  size_t size() const { return n_; }   // the n of the allocation (0: none)

  // frees what is held, then allocates room for max(n, min_n) elements; size() is n
  hipError_t alloc(size_t n, size_t min_n = 0) {
    reset();
    void *p = nullptr;
    const hipError_t e = Mem::alloc(&p, std::max(n, min_n) * sizeof(T));
    if (e != hipSuccess) return e;
    p_.reset(static_cast<T *>(p));
    n_ = n;
    return hipSuccess;
  }
  void reset() {
    p_.reset();
    n_ = 0;
  }
  // the allocation alone, for a list that keeps it until its own owner goes
  std::unique_ptr<void, Mem> retire() {
    n_ = 0;
    return std::unique_ptr<void, Mem>(p_.release());
  }

 private:
  std::unique_ptr<T, Mem> p_;
  size_t n_ = 0;
};

template <typename T>
using PinnedBuf = DevBuf<T, PinnedMem<hipHostMallocDefault>>;
template <typename T>
using MappedBuf = DevBuf<T, PinnedMem<hipHostMallocMapped>>;   // pinned and mapped into the device's address space
using Retired = std::vector<std::unique_ptr<void, DeviceMem>>;

// A state's buffer that a captured step graph (msc_sweep_step) may replay: grown to n elements without a wait, and the
// buffer it had goes to `retired`, freed when the state is destroyed -- the graph may still read it.
template <typename T>
hipError_t grow_retained(Retired &retired, DevBuf<T> &buf, size_t n) {
  if (buf.size() >= n) return hipSuccess;
  DevBuf<T> fresh;
  const hipError_t e = fresh.alloc(n);
  if (e != hipSuccess) return e;
  if (buf) retired.push_back(buf.retire());
  buf = std::move(fresh);
  return hipSuccess;
}

// A workspace that only direct calls use (no captured graph reads it): at least n elements; a smaller buffer is freed
// first, after the stream is idle, because an earlier asynchronous call may still read it.
template <typename T>
hipError_t reserve_synced(hipStream_t s, DevBuf<T> &buf, size_t n) {
  if (n <= buf.size() && buf) return hipSuccess;
  const hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  buf.reset();
  return buf.alloc(n, 1);
}

// A table that a call fills on the host and copies to the device on a stream: two pinned areas taken in turn, and an
// event per area recorded behind the copy out of it.  begin() waits for that event before it hands the area out again, so
// no pending copy reads an area that is being written; the device side is ordered by the stream alone.  (Not copyable:
// the areas are not.)
class StagedUpload {
 public:
  ~StagedUpload() {   // (the pinned areas go after this body: no copy reads them then)
    for (Area &a : area_) {
      if (a.pending) (void)hipEventSynchronize(a.copied);
      if (a.copied) (void)hipEventDestroy(a.copied);
    }
  }
  // both areas at least `bytes` now, so that no later begin() of that size allocates
  hipError_t reserve(size_t bytes) {
    const hipError_t e = ready(area_[0], bytes);
    return e != hipSuccess ? e : ready(area_[1], bytes);
  }
  // *host: the area whose turn it is, of at least `bytes`, as the table type the caller fills (the one place a staging
  // area is read as a type).  An area too small is idle once its event has passed, so it is freed and allocated anew.
  template <typename T>
  hipError_t begin(size_t bytes, T **host) {
    const hipError_t e = ready(area_[turn_], bytes);
    *host = reinterpret_cast<T *>(area_[turn_].mem.get());
    return e;
  }
  // the first `bytes` of the area begun to dev, on the stream; the turn passes to the other area
  hipError_t commit(hipStream_t s, void *dev, size_t bytes) {
    Area &a = area_[turn_];
    turn_ ^= 1;
    hipError_t e = hipMemcpyAsync(dev, a.mem.get(), bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(a.copied, s);
    if (e == hipSuccess) a.pending = true;
    return e;
  }

 private:
  struct Area {
    PinnedBuf<unsigned char> mem;
    hipEvent_t copied = nullptr;
    bool pending = false;
  };
  static hipError_t ready(Area &a, size_t bytes) {
    hipError_t e = a.pending ? hipEventSynchronize(a.copied) : hipSuccess;
    if (e != hipSuccess) return e;
    a.pending = false;
    if (!a.copied) e = hipEventCreateWithFlags(&a.copied, hipEventDisableTiming);
    if (e == hipSuccess && (a.mem.size() < bytes || !a.mem)) e = a.mem.alloc(bytes, 1);
    return e;
  }
  Area area_[2];
  int turn_ = 0;
};

}  // namespace msc
