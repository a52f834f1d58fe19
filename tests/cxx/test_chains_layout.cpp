// Host test of common_amd/csrc/chains_layout.hpp alone: the carve, and the two composite blocks of the chain ensemble's
// calls against the formulas the offsets were first written as (in full below, none taken from the header), over the
// entry sizes the library has today (64-bit pointers) and over sizes that are no multiple of the alignment.  No device.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chains_layout.hpp"

using namespace msc::layout;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct Part { size_t at, bytes, align; };
// every part starts on its alignment, none overlaps another, they lie in order, and the total ends the last
static void check_parts(const std::vector<Part> &parts, size_t total) {
  for (size_t i = 0; i < parts.size(); i++) {
    CHECK(parts[i].at % parts[i].align == 0);
    for (size_t j = 0; j < i; j++)
      CHECK(parts[j].at + parts[j].bytes <= parts[i].at || parts[i].at + parts[i].bytes <= parts[j].at);
    if (i) CHECK(parts[i - 1].at + parts[i - 1].bytes <= parts[i].at);
  }
  CHECK(total == parts.back().at + parts.back().bytes);
}

static void test_carve() {
  Carve c;
  CHECK(c.end == 0);
  CHECK(c.take(5, 16) == 0 && c.end == 5);
  CHECK(c.take(3, 1) == 5 && c.end == 8);
  CHECK(c.take(0, 16) == 16 && c.end == 16);          // an empty part still lands on its alignment
  CHECK(c.take(7, 16) == 16 && c.end == 23);
  CHECK(c.take(4, 12) == 24 && c.end == 28);          // an alignment that is no power of two
  CHECK(c.take(1, 256) == 256 && c.end == 257);
}

// MargChain [nchains] | 16-aligned MargFeat [nsel] | void * [nfeat]
static void test_marg_block() {
  const size_t chain_sizes[] = {40, 36, 1}, feat_sizes[] = {16, 12}, ptr = 8;   // (40, 16: MargChain, MargFeat)
  for (size_t nchains : {1, 3, 257})
    for (size_t nfeat : {1, 5, 256})
      for (size_t nsel : {(size_t)1, nfeat})
        for (size_t cs : chain_sizes)
          for (size_t fs : feat_sizes) {
            const MargBlock b = marg_block(nchains, nsel, nfeat, cs, fs, ptr);
            const size_t marg_feat_at = (nchains * cs + 15) & ~(size_t)15;      // as first written
            const size_t outs_at = marg_feat_at + nsel * fs;
            CHECK(b.chains == 0);
            CHECK(b.feats == marg_feat_at);
            if (fs % ptr == 0) CHECK(b.outs == outs_at);   // (a MargFeat is a multiple of a pointer: no gap before the pointers)
            CHECK(b.outs >= outs_at && b.outs < outs_at + ptr);
            check_parts({{b.chains, nchains * cs, 16}, {b.feats, nsel * fs, 16}, {b.outs, nfeat * ptr, ptr}}, b.bytes);
          }
}

// up: HpChain [nchains] | SliceTarget [nchains][nt] | SliceCoord [n]; down: values | evals | status, 4 bytes [nchains][n]
static void test_hp_blocks() {
  const size_t sizes[][3] = {{48, 56, 24}, {44, 52, 20}, {1, 1, 1}};            // (48, 56, 24: HpChain, SliceTarget, SliceCoord)
  for (size_t nc : {1, 3, 257})
    for (size_t n : {1, 7})
      for (size_t nt : {1, 3})
        for (const auto &sz : sizes) {
          const HpBlocks b = hp_blocks(nc, nt, n, sz[0], sz[1], sz[2]);
          // as first written, for one buffer of both halves
          const size_t cells = nc * n;
          const size_t o_tgt = align16(nc * sz[0]), o_coord = o_tgt + align16(nc * nt * sz[1]);
          const size_t o_val = o_coord + align16(n * sz[2]), o_ev = o_val + align16(cells * 4);
          const size_t o_stat = o_ev + align16(cells * 4);
          CHECK(b.chains == 0 && b.targets == o_tgt && b.coords == o_coord);
          CHECK(align16(b.up_bytes) == o_val);
          CHECK(b.values == 0 && b.evals == o_ev - o_val && b.status == o_stat - o_val);
          check_parts({{b.chains, nc * sz[0], 16}, {b.targets, nc * nt * sz[1], 16}, {b.coords, n * sz[2], 16}}, b.up_bytes);
          check_parts({{b.values, cells * 4, 16}, {b.evals, cells * 4, 16}, {b.status, cells * 4, 16}}, b.down_bytes);
        }
}

int main() {
  test_carve();
  test_marg_block();
  test_hp_blocks();
  std::printf("chains layout ok\n");
  return 0;
}
