// Host build of common_amd/csrc/linkage_host.hpp: Prim's chain in the kernel's reduction shape (or as the plain scan)
// followed by the sort, the relabelling and the leaf walk, driven from ctypes by tests/test_linkage_cpu.py.
// With -DLINKAGE_HOST_MAIN the file is a program of its own: tie-heavy and tie-free matrices through every shape the
// kernel is instantiated at, the shaped chain against the scan, the leaf order checked as a permutation whose walk
// visits every node once.  That is the build to run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "linkage_host.hpp"

using namespace msc::linkage;

extern "C" {

// threads == 0: the scan; otherwise the kernel's shape (threads, cols), which must hold n columns.  Returns 0, or -1
// for a shape that does not.
int linkage_host(const float *z, uint64_t ld, uint32_t n, uint32_t threads, uint32_t cols, double *out_linkage,
                 uint32_t *out_order) {
  if (n < 2) return -1;
  std::vector<double> edges(3 * (size_t)(n - 1));
  if (threads == 0) {
    prim_scan(z, ld, n, edges.data());
  } else {
    if (threads % kWave || threads > kMaxThreads || cols < 1 || cols > kMaxCols || (uint64_t)threads * cols < n) return -1;
    prim_shaped(z, ld, n, Shape{threads, cols}, edges.data());
  }
  finish(edges.data(), n, out_linkage, out_order);
  return 0;
}

// what msc_linkage_single launches for n
void linkage_shape(uint32_t n, uint32_t *threads, uint32_t *cols) {
  const Shape s = shape_for(n);
  *threads = s.threads, *cols = s.cols;
}

}

#ifdef LINKAGE_HOST_MAIN
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}

// Z of S samples of labels below K: multiples of 1 / S (S == 0: distinct real values instead)
static std::vector<float> make_z(uint32_t n, uint64_t ld, uint32_t S, uint32_t K) {
  std::vector<float> z((size_t)n * ld, -7.0f);
  std::vector<uint32_t> lab((size_t)(S ? S : 1) * n);
  for (auto &v : lab) v = next_u32() % K;
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t j = i; j < n; j++) {
      float v;
      if (S == 0) {
        v = (float)(next_u32() >> 8) / 16777216.0f * 3.0f - 1.0f;
      } else {
        uint32_t c = 0;
        for (uint32_t s = 0; s < S; s++) c += lab[(size_t)s * n + i] == lab[(size_t)s * n + j];
        v = (float)c / (float)S;
      }
      z[(size_t)i * ld + j] = z[(size_t)j * ld + i] = v;
    }
  return z;
}

int main() {
  const uint32_t ns[] = {2, 3, 17, 64, 65, 257, 600, 1025, 2049, 4097};
  const uint32_t shapes[][2] = {{64, 1}, {128, 1}, {320, 1}, {640, 1}, {1024, 1}, {1024, 2}, {1024, 4}, {1024, 8},
                                {1024, 16}, {1024, 32}, {1024, 64}};
  int checked = 0;
  for (uint32_t n : ns)
    for (uint32_t S : {0u, 1u, 3u}) {
      const uint64_t ld = n + (n % 3);
      const std::vector<float> z = make_z(n, ld, S, S == 1 ? 4 : 3);
      std::vector<double> want(4 * (size_t)(n - 1)), got(want.size());
      std::vector<uint32_t> want_order(n), got_order(n);
      if (linkage_host(z.data(), ld, n, 0, 0, want.data(), want_order.data())) return 1;
      std::vector<uint8_t> seen(n, 0);
      for (uint32_t v : want_order) {
        if (v >= n || seen[v]) return std::printf("n = %u: the leaf order is no permutation\n", n), 1;
        seen[v] = 1;
      }
      uint32_t t0, c0;
      linkage_shape(n, &t0, &c0);
      for (const auto &sh : shapes) {
        if ((uint64_t)sh[0] * sh[1] < n) continue;
        if (n > 1100 && !(sh[0] == t0 && sh[1] == c0)) continue;   // (the large sizes: the launcher's own shape only)
        if (linkage_host(z.data(), ld, n, sh[0], sh[1], got.data(), got_order.data())) return 1;
        if (got != want || got_order != want_order)
          return std::printf("n = %u S = %u shape (%u, %u): differs from the scan\n", n, S, sh[0], sh[1]), 1;
        checked++;
      }
    }
  std::printf("linkage_host ok: %d (matrix, shape) cases\n", checked);
  return 0;
}
#endif
