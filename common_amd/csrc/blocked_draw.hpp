// blocked_draw.hpp -- one body, two kernels: the per-thread work of the blocked sampler's draw
// kernels as device functions, called by k_blocked_sticks / k_blocked_draw (kernels_blocked.hip), which deal them out over
// a grid, and by k_sm_chains (kernels_chains_sm.hip), where one workgroup makes a pair state's draws between two barriers.
// blocked_post.hpp has the arithmetic and the streams; here is only where a slot's suff-stats are read and its slices
// written.
#pragma once

#include "blocked_post.hpp"
#include "family_math.hpp"
#include "msc_internal.hpp"

namespace msc {

// the stick fraction of slot k: log V_k and log(1 - V_k), V_k ~ Beta(1 + n_k, alpha + n_after) (the last slot's is 1)
MSC_DEV void blk_stick_slot(double n_k, double n_after, double alpha, uint64_t key, uint32_t k, uint64_t sweep, bool last,
                            double *log_v, double *log_1mv) {
  double a, b;
  blocked::stick_post(n_k, n_after, alpha, &a, &b);
  pred::Stream s(key, k, sweep, blocked::kStickTag);
  blocked::draw_stick(s, a, b, last, log_v, log_1mv);
}

// slot k's parameters of feature bf from their conjugate posterior, stored as the float slices the assign kernels read
MSC_DEV void blk_draw_slot(const BlkFeat &bf, uint32_t k, uint32_t kpad, uint64_t key, uint64_t sweep, float *__restrict__ tab) {
  float *out = tab + (size_t)bf.slice0 * kpad + k;
  const float *hp = bf.hp;
  const uint32_t *u = bf.raw_u32;
  switch (bf.family) {
    case MSC_BB: {
      double a, b;
      blocked::bb_post(hp, (double)u[k], (double)u[kpad + k], &a, &b);
      pred::Stream s(key, k, sweep, bf.tag);
      blocked::draw_bb(s, a, b, out, kpad);
      break;
    }
    case MSC_GP: {
      double shape, rate;
      blocked::gp_post(hp, (double)u[k], (double)u[kpad + k], &shape, &rate);
      pred::Stream s(key, k, sweep, bf.tag);
      blocked::draw_gp(s, shape, rate, out, kpad);
      break;
    }
    case MSC_BNB: {
      double a, b;
      blocked::bnb_post(hp, (double)u[k], (double)u[kpad + k], &a, &b);
      pred::Stream s(key, k, sweep, bf.tag);
      blocked::draw_bnb(s, a, b, (double)hp[2], out, kpad);
      break;
    }
    case MSC_NICH: {
      double mu_n, kappa_n, sigmasq_n, nu_n;
      blocked::nich_post(hp, (double)u[k], (double)bf.raw_f32[k], (double)bf.raw_f32[kpad + k], &mu_n, &kappa_n,
                         &sigmasq_n, &nu_n);
      pred::Stream s(key, k, sweep, bf.tag);
      blocked::draw_nich(s, mu_n, kappa_n, sigmasq_n, nu_n, out, kpad);
      break;
    }
    case MSC_DD:   // raw rows {count_sum, counts[dim]}
      blocked::draw_dd(key, k, sweep, bf.tag, bf.dim, hp, u + (size_t)kpad + k, kpad, out, kpad);
      break;
    default: break;
  }
}

}  // namespace msc
