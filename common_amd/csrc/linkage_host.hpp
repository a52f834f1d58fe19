// linkage_host.hpp -- single linkage of a dense z-matrix (msc_linkage_single, include/microscopes_hip.h): what the
// kernel (kernels_linkage.hip) and the host share, and everything after the kernel, as plain C++ so that the host compiler
// builds it alone (tests/test_linkage_cpu.py checks it against scipy without a GPU).
//
// scipy's linkage(y, 'single') is
//   1. Prim's chain from node 0.  D[j] = +inf, x = 0; n - 1 times: mark x merged; for every unmerged j in ascending
//      order d = dist(x, j), D[j] = d where D[j] > d, and y = j, cur = D[j] where D[j] < cur; record (x, y, cur); x = y.
//      So y is the lexicographic minimum of (D[j], j) over the unmerged j: among equal distances the lowest index.  A
//      z-matrix holds multiples of 1 / S, ties are the normal case, and this rule decides the tree;
//   2. a stable sort of the n - 1 edges by distance;
//   3. a union-find relabelling in that order: row i = (min(root x, root y), max(..), distance, size), both roots
//      become node n + i;
//   4. leaves_list: the pre-order walk from node 2 n - 2, column 0 before column 1.
// Step 1 runs on the device with dist(x, j) = 1.0f - z[x][j] in float.  Its shape there: `threads` threads, each owning
// `cols` columns in groups of vec = min(cols, 4) neighbours (column(): one 16-byte load a group); a thread forms the
// minimum of its columns, a wave of 64 threads the minimum of its threads, and the workgroup the minimum of the wave
// minima.  Every level compares (key, j) with key = float_key(D[j]), an order-preserving map of the float to an
// unsigned integer, so the minimum of minima is the lexicographic minimum whatever the grouping.  prim_shaped() below is
// that reduction restated on the host, level by level, for every shape the kernel is instantiated at; prim_scan() is
// the chain as step 1 states it.  finish() is steps 2 to 4.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MSC_LK_HD __host__ __device__ inline
#else
#define MSC_LK_HD inline
#endif

namespace msc {
namespace linkage {

constexpr uint32_t kWave = 64;
constexpr uint32_t kMaxThreads = 1024;
constexpr uint32_t kMaxCols = 64;                       // columns a thread: its D in registers, its flags in one 64-bit mask
constexpr uint32_t kMaxN = kMaxThreads * kMaxCols;      // 65536
constexpr uint32_t kNone = 0xFFFFFFFFu;                 // no column; as a key, above every float that is not a NaN

// the launch for n points: n <= 1024 one column a thread and as many waves as hold n; beyond, 1024 threads and the
// lowest power of two of columns that holds n.  threads == 0: n is outside [2, kMaxN]
struct Shape {
  uint32_t threads, cols;
};
MSC_LK_HD Shape shape_for(uint32_t n) {
  if (n < 2 || n > kMaxN) return Shape{0, 0};
  if (n <= kMaxThreads) return Shape{(n + kWave - 1) / kWave * kWave, 1};
  uint32_t c = 2;
  while (c * kMaxThreads < n) c *= 2;
  return Shape{kMaxThreads, c};
}
MSC_LK_HD uint32_t vec_of(uint32_t cols) { return cols < 4 ? cols : 4; }
// the k-th column (k < cols) of thread t: group k / vec, element k % vec; ascending in k
MSC_LK_HD uint32_t column(uint32_t t, uint32_t threads, uint32_t vec, uint32_t k) {
  return vec * (t + threads * (k / vec)) + k % vec;
}
// a < b as floats  <=>  float_key(a) < float_key(b), for every pair that holds no NaN and not both zeros of opposite sign
// (1.0f - z is never -0)
MSC_LK_HD uint32_t float_key(float f) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  std::memcpy(&u, &f, 4);
#endif
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MSC_LK_HD float key_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  std::memcpy(&f, &u, 4);
  return f;
#endif
}

// what one level of the reduction hands to the next.  A thread without a candidate (every D[j] of its unmerged columns
// is +inf or NaN, which finite input never leaves after the first step) offers (kNone, its lowest unmerged column), so
// that the chain always moves to an unmerged point; a thread without unmerged columns offers (kNone, kNone).
struct Cand {
  uint32_t key, j;
};
MSC_LK_HD Cand cand_min(Cand a, Cand b) { return (b.key < a.key || (b.key == a.key && b.j < a.j)) ? b : a; }
// the edge's distance as the chain records it: scipy's cur stays +inf where nothing was below it
MSC_LK_HD double cand_distance(uint32_t key) {
  return key == kNone ? (double)std::numeric_limits<float>::infinity() : (double)key_float(key);
}

// ---- host only from here --------------------------------------------------------------------------------------------

// step 1 as stated: edges[3 i .. 3 i + 2] = (x, y, distance)
inline void prim_scan(const float *z, uint64_t ld, uint32_t n, double *edges) {
  std::vector<float> D(n, std::numeric_limits<float>::infinity());
  std::vector<uint8_t> merged(n, 0);
  uint32_t x = 0, y = 0;
  for (uint32_t i = 0; i + 1 < n; i++) {
    float cur = std::numeric_limits<float>::infinity();
    merged[x] = 1;
    for (uint32_t j = 0; j < n; j++) {
      if (merged[j]) continue;
      const float d = 1.0f - z[(uint64_t)x * ld + j];
      if (D[j] > d) D[j] = d;
      if (D[j] < cur) y = j, cur = D[j];
    }
    edges[3 * (size_t)i] = x, edges[3 * (size_t)i + 1] = y, edges[3 * (size_t)i + 2] = cur;
    x = y;
  }
}

// step 1 in the kernel's shape.  The diagonal is not used and nothing is read outside row x.
inline void prim_shaped(const float *z, uint64_t ld, uint32_t n, Shape s, double *edges) {
  const uint32_t T = s.threads, C = s.cols, V = vec_of(C), nw = T / kWave;
  std::vector<float> D((size_t)T * C, std::numeric_limits<float>::infinity());
  std::vector<uint64_t> unmerged(T, 0);
  for (uint32_t t = 0; t < T; t++)
    for (uint32_t k = 0; k < C; k++)
      if (column(t, T, V, k) < n) unmerged[t] |= 1ull << k;
  std::vector<Cand> wave(nw);
  uint32_t x = 0;
  for (uint32_t i = 0; i + 1 < n; i++) {
    {   // x's owner drops it
      const uint32_t q = x / V, t = q % T, k = (q / T) * V + x % V;
      unmerged[t] &= ~(1ull << k);
    }
    const float *row = z + (uint64_t)x * ld;
    for (uint32_t w = 0; w < nw; w++) {
      Cand wm{kNone, kNone};
      for (uint32_t l = 0; l < kWave; l++) {
        const uint32_t t = w * kWave + l;
        if (!unmerged[t]) continue;                      // (it offers (kNone, kNone), which changes no minimum)
        float best = std::numeric_limits<float>::infinity();
        uint32_t bj = kNone;
        for (uint32_t k = 0; k < C; k++) {
          if (!((unmerged[t] >> k) & 1)) continue;
          const uint32_t j = column(t, T, V, k);
          const float d = 1.0f - row[j];
          float &Dk = D[(size_t)t * C + k];
          if (Dk > d) Dk = d;
          if (Dk < best) best = Dk, bj = j;
        }
        Cand c{kNone, kNone};
        if (bj != kNone)
          c = Cand{float_key(best), bj};
        else
          c.j = column(t, T, V, (uint32_t)__builtin_ctzll(unmerged[t]));
        wm = cand_min(wm, c);
      }
      wave[w] = wm;
    }
    Cand m = wave[0];
    for (uint32_t w = 1; w < nw; w++) m = cand_min(m, wave[w]);
    edges[3 * (size_t)i] = x, edges[3 * (size_t)i + 1] = m.j, edges[3 * (size_t)i + 2] = cand_distance(m.key);
    x = m.j;
  }
}

// steps 2 to 4 from the chain's n - 1 edges: scipy's [n - 1][4] linkage matrix and / or the n leaves in order (either
// may be null).  No recursion: the walk keeps its own stack.
inline void finish(const double *edges, uint32_t n, double *out_linkage, uint32_t *out_order) {
  const uint32_t m = n - 1;
  std::vector<uint32_t> by_distance(m);
  std::iota(by_distance.begin(), by_distance.end(), 0u);
  std::stable_sort(by_distance.begin(), by_distance.end(),
                   [&](uint32_t a, uint32_t b) { return edges[3 * (size_t)a + 2] < edges[3 * (size_t)b + 2]; });
  std::vector<uint32_t> parent(2 * (size_t)n - 1), size(2 * (size_t)n - 1, 1), left(m), right(m);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&](uint32_t a) {
    uint32_t r = a;
    while (parent[r] != r) r = parent[r];
    while (parent[a] != r) {
      const uint32_t next = parent[a];
      parent[a] = r;
      a = next;
    }
    return r;
  };
  for (uint32_t i = 0; i < m; i++) {
    const double *e = edges + 3 * (size_t)by_distance[i];
    const uint32_t a = find((uint32_t)e[0]), b = find((uint32_t)e[1]);
    left[i] = std::min(a, b), right[i] = std::max(a, b);
    parent[a] = parent[b] = n + i;
    size[n + i] = size[a] + size[b];
    if (out_linkage) {
      double *r = out_linkage + 4 * (size_t)i;
      r[0] = left[i], r[1] = right[i], r[2] = e[2], r[3] = size[n + i];
    }
  }
  if (!out_order) return;
  std::vector<uint32_t> stack;
  stack.reserve(n);
  stack.push_back(2 * n - 2);
  uint32_t k = 0;
  while (!stack.empty()) {
    const uint32_t v = stack.back();
    stack.pop_back();
    if (v < n) {
      out_order[k++] = v;
    } else {
      stack.push_back(right[v - n]);
      stack.push_back(left[v - n]);
    }
  }
}

}  // namespace linkage
}  // namespace msc
