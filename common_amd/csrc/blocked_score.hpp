// blocked_score.hpp -- how a row meets the drawn parameter table (blocked_post.hpp lists the slices): the row's value
// codes and the scores of eight slots side by side.  Shared by the assign kernels of the blocked sweep
// (kernels_blocked.hip) and of the split-merge move (kernels_splitmerge.hip): one expression, one order of the sums.
// A row's value of a feature travels as one 32-bit CODE: bb 0 / 1, dd the value clamped into [0, dim), gp / bnb / nich the
// value as a float; kBlkMasked = a masked entry or a noop feature, which adds nothing.
#pragma once

#include "family_math.hpp"
#include "msc_internal.hpp"

namespace msc {

constexpr uint32_t kBlkMasked = 0xffffffffu;   // (as a float a NaN no conversion from uint32 produces)
constexpr int kBlkTile = 8;                    // slots scored side by side
enum { MODE_GLOBAL = 0, MODE_STAGED = 1, MODE_NICH1 = 2 };

MSC_DEV uint32_t blk_code(const BlkFeat &bf, uint64_t vrow) {
  if (bf.kind == MSC_BLK_NOOP || (bf.mask != nullptr && bf.mask[vrow] != 0)) return kBlkMasked;
  switch (bf.kind) {
    case MSC_BLK_SELECT: return static_cast<const uint8_t *>(bf.col)[vrow] != 0 ? 1u : 0u;
    case MSC_BLK_LINEAR: return __float_as_uint((float)static_cast<const uint32_t *>(bf.col)[vrow]);
    case MSC_BLK_GATHER: {
      const int32_t v = static_cast<const int32_t *>(bf.col)[vrow];
      return v < 0 ? 0u : (uint32_t)v >= bf.dim ? bf.dim - 1u : (uint32_t)v;
    }
    default: return __float_as_uint(static_cast<const float *>(bf.col)[vrow]);
  }
}

// the scores of slots k0 .. k0 + 7 for one row (k0 a multiple of eight: the table's rows are kpad floats, so the eight
// operands of a slice are one aligned 32-byte stretch, and slots beyond K read the table's padding).  Both passes call
// this: the same operations in the same order, so pass 2 meets the bits pass 1 summed.
template <int MODE>
MSC_DEV void blk_tile_scores(const BlkFeat *__restrict__ fs, int nfeat, const float *__restrict__ tab, uint32_t kpad,
                             uint32_t k0, const uint32_t *codes, uint32_t cstride, uint64_t vrow, uint32_t code1,
                             float (&s)[kBlkTile]) {
#pragma clang fp contract(off)
  const float *lw = tab + k0;
#pragma unroll
  for (int j = 0; j < kBlkTile; j++) s[j] = lw[j];
  if (MODE == MODE_NICH1) {
    if (code1 != kBlkMasked) {
      const float x = __uint_as_float(code1);
      const float *p = tab + (size_t)kpad + k0;
#pragma unroll
      for (int j = 0; j < kBlkTile; j++) {
        const float d = x - p[kpad + j];
        s[j] += fmaf(p[2 * (size_t)kpad + j] * d, d, p[j]);
      }
    }
  } else {
    for (int f = 0; f < nfeat; f++) {
      const uint32_t kind = fs[f].kind;
      const uint32_t code = MODE == MODE_STAGED ? codes[(size_t)f * cstride] : blk_code(fs[f], vrow);
      if (code == kBlkMasked) continue;
      const float *p = tab + (size_t)fs[f].slice0 * kpad + k0;
      if (kind == MSC_BLK_SELECT) {
#pragma unroll
        for (int j = 0; j < kBlkTile; j++) s[j] += code ? p[kpad + j] : p[j];
      } else if (kind == MSC_BLK_LINEAR) {
        const float x = __uint_as_float(code);
#pragma unroll
        for (int j = 0; j < kBlkTile; j++) s[j] += fmaf(x, p[kpad + j], p[j]);
      } else if (kind == MSC_BLK_GATHER) {
        const float *q = p + (size_t)code * kpad;
#pragma unroll
        for (int j = 0; j < kBlkTile; j++) s[j] += q[j];
      } else {
        const float x = __uint_as_float(code);
#pragma unroll
        for (int j = 0; j < kBlkTile; j++) {
          const float d = x - p[kpad + j];
          s[j] += fmaf(p[2 * (size_t)kpad + j] * d, d, p[j]);
        }
      }
    }
  }
}

}  // namespace msc
