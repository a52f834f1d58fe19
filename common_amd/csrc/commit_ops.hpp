// commit_ops.hpp -- additive sums -> the reference's fields for one (feature, group): the body of k_commit, shared with
// the fused commit + prepare kernel of the sweep step (kernels_score.hip k_commit_prepare); and the reference's fields ->
// the score constants of that (feature, group), shared by the prepare kernels and the sequential sweep (kernels_seq.hip)
#pragma once
#include "family_math.hpp"

namespace msc {

MSC_DEV void commit_group(const FeatDesc &fd, uint32_t k, uint32_t kpad) {
  switch (fd.family) {
    case MSC_BBNC:
    case MSC_BB:
      fd.raw_u32[k] = (uint32_t)fd.acc_i64[k];
      fd.raw_u32[kpad + k] = (uint32_t)fd.acc_i64[kpad + k];
      break;
    case MSC_GP:
      fd.raw_u32[k] = (uint32_t)fd.acc_i64[k];
      fd.raw_u32[kpad + k] = (uint32_t)fd.acc_i64[kpad + k];
      fd.raw_f32[k] = (float)fd.acc_f64[k];
      break;
    case MSC_BNB:
      fd.raw_u32[k] = (uint32_t)fd.acc_i64[k];
      fd.raw_u32[kpad + k] = (uint32_t)fd.acc_i64[kpad + k];
      break;
    case MSC_DM:
      for (uint32_t i = 0; i < fd.dim; i++) fd.raw_u32[(size_t)i * kpad + k] = (uint32_t)fd.acc_i64[(size_t)i * kpad + k];
      fd.raw_f32[k] = (float)fd.acc_f64[k];
      break;
    case MSC_DD: {
      long long tot = 0;
      for (uint32_t i = 0; i < fd.dim; i++) {
        const long long c = fd.acc_i64[(size_t)i * kpad + k];
        fd.raw_u32[(size_t)(1 + i) * kpad + k] = (uint32_t)c;
        tot += c;
      }
      fd.raw_u32[k] = (uint32_t)tot;
    } break;
    case MSC_NICH: {
      const long long n = fd.acc_i64[k];
      const double sx = fd.acc_f64[k], sxx = fd.acc_f64[kpad + k];
      double mean = 0, ctv = 0;
      if (n > 0) mean = sx / (double)n;
      if (n > 1) {
        ctv = sxx - (double)n * mean * mean;
        if (ctv < 0) ctv = 0;
      }
      fd.raw_u32[k] = (uint32_t)n;
      fd.raw_f32[k] = (float)mean;
      fd.raw_f32[kpad + k] = (float)ctv;
    } break;
    default: break;
  }
}

// ---------------------------------------------------------------------------
// prepare: one thread per (feature, group slot); pads (k >= K) are prepared from their
// zeroed raw stats so that vector loads of a full tile stay finite.
// ---------------------------------------------------------------------------
// (z, nz): the table rows of the count / categorical families are dealt out over nz threads per (feature, group) --
// a column with counts up to 1000 would otherwise be ~2000 lgamma chains in a row per thread; what a group needs
// once is done by z = 0
MSC_DEV void prepare_group(const FeatDesc &fd, uint32_t k, uint32_t kpad, uint32_t z, uint32_t nz) {
  if (z != 0 && fd.family != MSC_GP && fd.family != MSC_BNB && fd.family != MSC_DD) return;
  switch (fd.family) {
    // (every lookup family keeps one table row of zeros right after its last entry: what a masked value of a column with
    // the mask folded in selects, FeatDesc::col_sentinel)
    case MSC_BB: {
      float s0, s1;
      bb_prepare(fd.hp, fd.raw_u32[k], fd.raw_u32[kpad + k], s0, s1);
      fd.tab[k] = s0;
      fd.tab[kpad + k] = s1;
      fd.tab[2 * (size_t)kpad + k] = 0.f;
      if (fd.loo_tab != nullptr) fd.loo_tab[2 * (size_t)kpad + k] = 0.f;
      if (fd.loo_tab != nullptr) {          // (an entry is only read for a row that is in the group with that value)
        const uint32_t h = fd.raw_u32[k], t = fd.raw_u32[kpad + k];
        fd.loo_tab[k] = t ? (float)bb_loo(fd.hp, h, t, false) : 0.f;
        fd.loo_tab[kpad + k] = h ? (float)bb_loo(fd.hp, h, t, true) : 0.f;
      }
    } break;
    case MSC_BBNC: {
      float s0, s1;
      bbnc_prepare(fd.raw_f32[k], s0, s1);
      fd.tab[k] = s0;
      fd.tab[kpad + k] = s1;
      fd.tab[2 * (size_t)kpad + k] = 0.f;
    } break;
    case MSC_GP: {
      const uint32_t cnt = fd.raw_u32[k], sum = fd.raw_u32[kpad + k];
      if (z == 0) {
        gp_prepare_consts(fd.hp, cnt, sum, fd.tab[(size_t)GP_NSE_HI * kpad + k], fd.tab[(size_t)GP_NSE_LO * kpad + k]);
        fd.tab[(size_t)(GP_T0 + fd.vcap) * kpad + k] = 0.f;
        if (fd.loo_tab != nullptr) fd.loo_tab[(size_t)fd.vcap * kpad + k] = 0.f;
      }
      for (uint32_t v = z; v < fd.vcap; v += nz)
        fd.tab[(size_t)(GP_T0 + v) * kpad + k] = gp_prepare_table(fd.hp, cnt, sum, v);
      if (fd.loo_tab != nullptr)
        for (uint32_t v = z; v < fd.vcap; v += nz)
          fd.loo_tab[(size_t)v * kpad + k] = (cnt >= 1 && sum >= v) ? (float)gp_loo(fd.hp, cnt, sum, v) : 0.f;
    } break;
    case MSC_BNB: {
      const double cnt = fd.raw_u32[k], sum = fd.raw_u32[kpad + k];
      if (z == 0) {
        fd.tab[(size_t)(GP_T0 + fd.vcap) * kpad + k] = 0.f;
        if (fd.loo_tab != nullptr) fd.loo_tab[(size_t)fd.vcap * kpad + k] = 0.f;
      }
      for (uint32_t v = z; v < fd.vcap; v += nz)
        fd.tab[(size_t)(GP_T0 + v) * kpad + k] = (float)bnb_score(fd.hp, cnt, sum, (double)v);
      if (fd.loo_tab != nullptr)
        for (uint32_t v = z; v < fd.vcap; v += nz)
          fd.loo_tab[(size_t)v * kpad + k] = (cnt >= 1.0 && sum >= (double)v) ? (float)bnb_score(fd.hp, cnt - 1.0, sum - (double)v, (double)v) : 0.f;
    } break;
    case MSC_DD: {
      const uint32_t csum = fd.raw_u32[k];
      if (z == 0) {
        fd.tab[(size_t)fd.dim * kpad + k] = 0.f;
        if (fd.loo_tab != nullptr) fd.loo_tab[(size_t)fd.dim * kpad + k] = 0.f;
      }
      for (uint32_t i = z; i < fd.dim; i += nz)
        fd.tab[(size_t)i * kpad + k] =
            dd_prepare_entry(fd.hp[i], fd.raw_u32[(size_t)(1 + i) * kpad + k], fd.aux, csum);
      if (fd.loo_tab != nullptr)
        for (uint32_t i = z; i < fd.dim; i += nz) {
          const uint32_t c = fd.raw_u32[(size_t)(1 + i) * kpad + k];
          fd.loo_tab[(size_t)i * kpad + k] = c ? (float)dd_loo(fd.hp[i], c, fd.aux, csum) : 0.f;
        }
    } break;
    case MSC_NICH: {
      float o[NICH_ROWS];
      nich_prepare(fd.hp, fd.raw_u32[k], fd.raw_f32[k], fd.raw_f32[kpad + k], o);
#pragma unroll
      for (int i = 0; i < NICH_ROWS; i++) fd.tab[(size_t)i * kpad + k] = o[i];
      if (fd.loo64 != nullptr) nich_loo_prepare(fd.hp, fd.raw_u32[k], fd.raw_f32[k], fd.raw_f32[kpad + k], fd.loo64 + (size_t)k * kNlooStride, 1);
    } break;
    default: break;
  }
}

// score_data of one (feature, group) from the reference's fields: the body of k_score_data (kernels_state.hip), shared
// with the ensemble's split-merge kernel (kernels_chains_sm.hip)
MSC_DEV double score_data_group(const FeatDesc &fd, uint32_t k, uint32_t kpad) {
  double s = 0;
  switch (fd.family) {
    case MSC_BB: s = bb_score_data(fd.hp, fd.raw_u32[k], fd.raw_u32[kpad + k]); break;
    case MSC_BBNC: s = bbnc_score_data(fd.hp, fd.raw_u32[k], fd.raw_u32[kpad + k], fd.raw_f32[k]); break;
    case MSC_GP: s = gp_score_data(fd.hp, fd.raw_u32[k], fd.raw_u32[kpad + k], (double)fd.raw_f32[k]); break;
    case MSC_DD: s = dd_score_data(fd.hp, fd.dim, fd.raw_u32 + kpad + k, kpad, fd.raw_u32[k]); break;
    case MSC_NICH: s = nich_score_data(fd.hp, fd.raw_u32[k], fd.raw_f32[k], fd.raw_f32[kpad + k]); break;
    case MSC_BNB: s = bnb_score_data(fd.hp, fd.raw_u32[k], fd.raw_u32[kpad + k]); break;
    case MSC_DM: s = dm_score_data(fd.hp, fd.dim, fd.raw_u32 + k, kpad, (double)fd.raw_f32[k]); break;
    default: break;
  }
  return s;
}

}  // namespace msc
