// canon_ids.hpp -- one workgroup turns a partition's int32 labels (any value is a label, only equality is used) into
// 16-bit ids numbered from 0 in the order of each label's first row: an LDS hash table label -> first row, then the rank
// of every first row among the first rows.  The scheme of k_zm_refine_init and k_pd_canon, as a device function
// (kernels_refine_vi.hip uses it; those two kernels keep their own copies).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace msc {

template <uint32_t MAXC>
struct CanonTable {
  static constexpr uint32_t kSlots = 2u * MAXC;             // a power of two
  unsigned long long key[kSlots];                            // the label (zero-extended), all ones = empty
  uint32_t first[kSlots];
  uint16_t rank[kSlots];
  uint32_t cnt, err;
};

__device__ inline uint32_t canon_hash(uint32_t x, uint32_t slots) {
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x & (slots - 1u);
}

// lab: m labels; out: ldi >= m ids (the tail is zeroed).  Returns the number of clusters, the same in every thread, or 0
// when there are more than cap <= MAXC (out is all 0 then).  Every thread of the workgroup of THREADS calls it.
template <uint32_t MAXC, uint32_t THREADS>
__device__ inline uint32_t canon_ids(CanonTable<MAXC> &tab, const int32_t *__restrict__ lab, uint32_t m, uint32_t cap,
                                     uint16_t *__restrict__ out, uint64_t ldi) {
  constexpr uint32_t kSlots = CanonTable<MAXC>::kSlots, kNone = 0xFFFFFFFFu;
  static_assert((kSlots & (kSlots - 1u)) == 0u && MAXC + THREADS < kSlots, "the table cannot fill up before every thread has seen the overflow");
  const uint32_t t = threadIdx.x;
  for (uint32_t q = t; q < kSlots; q += THREADS) tab.key[q] = ~0ull, tab.first[q] = kNone;
  if (t == 0u) tab.cnt = 0u, tab.err = 0u;
  __syncthreads();
  for (uint32_t a = t; a < m; a += THREADS) {
    if (*(volatile uint32_t *)&tab.cnt > cap) break;         // (already too many: do not fill the table)
    const unsigned long long key = (uint32_t)lab[a];
    const uint32_t h = canon_hash((uint32_t)key, kSlots);
    bool placed = false;
    for (uint32_t p = 0; p < kSlots && !placed; p++) {
      const uint32_t slot = (h + p) & (kSlots - 1u);
      const unsigned long long old = atomicCAS(&tab.key[slot], ~0ull, key);
      if (old == ~0ull) atomicAdd(&tab.cnt, 1u);
      if (old == ~0ull || old == key) {
        atomicMin(&tab.first[slot], a);
        placed = true;
      }
    }
    if (!placed) tab.err = 1u;
  }
  __syncthreads();
  const uint32_t count = tab.cnt;
  if (tab.err != 0u || count > cap) {                        // (uniform)
    for (uint64_t a = t; a < ldi; a += THREADS) out[a] = 0;
    return 0u;
  }
  for (uint32_t q = t; q < kSlots; q += THREADS) {
    const uint32_t f = tab.first[q];
    if (f == kNone) continue;
    uint32_t r = 0u;
    for (uint32_t o = 0; o < kSlots; o++) r += tab.first[o] < f ? 1u : 0u;     // (kNone is never below)
    tab.rank[q] = (uint16_t)r;                               // < count <= cap
  }
  __syncthreads();
  for (uint64_t a = t; a < ldi; a += THREADS) {
    uint16_t id = 0;
    if (a < m) {
      const unsigned long long key = (uint32_t)lab[a];
      const uint32_t h = canon_hash((uint32_t)key, kSlots);
      for (uint32_t p = 0; p < kSlots; p++) {                // (it is there: the walk ends at it)
        const uint32_t slot = (h + p) & (kSlots - 1u);
        if (tab.key[slot] == key) {
          id = tab.rank[slot];
          break;
        }
      }
    }
    out[a] = id;
  }
  return count;
}

}  // namespace msc
