// seq_score.hpp -- score_value of one value against one group, read from a state's prepared tables through its FeatDesc:
// what the sequential sweep (kernels_seq.hip) and the ensemble's row predictive pass (kernels_chains_marginal.hip) share.
#pragma once

#include "family_math.hpp"
#include "msc_internal.hpp"

namespace msc {

// score_value of value v against group k, read from the prepared tables -- the arithmetic of the batched kernels
// (score_block.hpp add_feature; counts beyond the exact table: k_gp_large_fix)
MSC_DEV float seq_feature_score(const FeatDesc &fd, uint32_t v, uint32_t k, uint32_t kpad, double gp_rowc) {
  switch (fd.family) {
    case MSC_BB: return fd.tab[(v != 0 ? kpad : 0u) + k];
    case MSC_DD: {
      const int c = (int)v < 0 ? 0 : ((int)v >= (int)fd.dim ? (int)fd.dim - 1 : (int)v);
      return fd.tab[(size_t)c * kpad + k];
    }
    case MSC_GP:
      if (v < fd.vcap) return fd.tab[(size_t)(GP_T0 + v) * kpad + k];
      return gp_eval_large((double)v, gp_rowc, (double)fd.hp[0] + (double)fd.raw_u32[(size_t)kpad + k],
                           (double)fd.hp[1] + (double)fd.raw_u32[k],
                           (double)fd.tab[(size_t)GP_NSE_HI * kpad + k] + (double)fd.tab[(size_t)GP_NSE_LO * kpad + k]);
    case MSC_BNB:
      if (v < fd.vcap) return fd.tab[(size_t)(GP_T0 + v) * kpad + k];
      return (float)bnb_score(fd.hp, (double)fd.raw_u32[k], (double)fd.raw_u32[(size_t)kpad + k], (double)v);
    case MSC_NICH:
      return nich_eval(__uint_as_float(v), fd.tab[(size_t)NICH_MU_HI * kpad + k], fd.tab[(size_t)NICH_MU_LO * kpad + k],
                       fd.tab[(size_t)NICH_C0 * kpad + k], fd.tab[(size_t)NICH_C1LN2 * kpad + k],
                       fd.tab[(size_t)NICH_C1 * kpad + k], fd.tab[(size_t)NICH_C2 * kpad + k]);
    default: return 0.f;     // noop (models/noop.hpp:17)
  }
}

}  // namespace msc
