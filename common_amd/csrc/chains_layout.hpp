// chains_layout.hpp -- where the parts of a composite table lie in its block of bytes: the carve that every such block
// is cut by, and the blocks of the chain ensemble's calls (chains.cpp).  Host-only arithmetic on element sizes and counts
// passed in: no device header, no state.
#pragma once

#include <cstddef>

namespace msc::layout {

// Sub-blocks of one block, in the order they are asked for: take() returns the offset of the next, the first multiple of
// `align` (a power of two or not) at or past the end of the one before; `end` is the end of the last, the block's bytes.
struct Carve {
  size_t end = 0;
  size_t take(size_t bytes, size_t align) {
    const size_t at = (end + align - 1) / align * align;
    end = at + bytes;
    return at;
  }
};

constexpr size_t kBlockAlign = 16;   // what a sub-block read with 128-bit loads starts on

// msc_chains_score_marginal / msc_chains_sample_predictive: MargChain [nchains] | MargFeat [nsel] | void * [nfeat], the
// last only in a sampling call (a scoring call uploads the first `outs` bytes)
struct MargBlock {
  size_t chains, feats, outs, bytes;
};
inline MargBlock marg_block(size_t nchains, size_t nsel, size_t nfeat, size_t chain_size, size_t feat_size, size_t ptr_size) {
  Carve c;
  const size_t chains = c.take(nchains * chain_size, kBlockAlign), feats = c.take(nsel * feat_size, kBlockAlign);
  const size_t outs = c.take(nfeat * ptr_size, ptr_size);
  return {chains, feats, outs, c.end};
}

// msc_chains_hp_slice.  Up: HpChain [nchains] | SliceTarget [nchains][ntargets] | SliceCoord [n]; down, a block of its
// own: values | evals | status, each 4 bytes [nchains][n]
struct HpBlocks {
  size_t chains, targets, coords, up_bytes;
  size_t values, evals, status, down_bytes;
};
inline HpBlocks hp_blocks(size_t nchains, size_t ntargets, size_t n, size_t chain_size, size_t target_size, size_t coord_size) {
  Carve up, down;
  const size_t chains = up.take(nchains * chain_size, kBlockAlign);
  const size_t targets = up.take(nchains * ntargets * target_size, kBlockAlign);
  const size_t coords = up.take(n * coord_size, kBlockAlign);
  const size_t cells = nchains * n * 4, values = down.take(cells, kBlockAlign), evals = down.take(cells, kBlockAlign);
  const size_t status = down.take(cells, kBlockAlign);
  return {chains, targets, coords, up.end, values, evals, status, down.end};
}

}  // namespace msc::layout
