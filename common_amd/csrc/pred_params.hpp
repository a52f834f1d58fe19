// pred_params.hpp -- a group's posterior predictive parameters from its raw sufficient statistics and hp, in double: the
// formulas of the host sampler (include/microscopes_amd/hip_models.hpp detail::sampler), one function a family.
// k_pred_prepare (kernels_pred.hip) stores what they return for k_pred_sample; the ensemble's draw (kernels_chains_pred.hip)
// evaluates them for the one (chain, group) of its row.  Both read the same expressions, so the same tables give the same
// doubles: what makes msc_chains_sample_predictive's entries msc_sample_predictive's, bit for bit.
// u / f: the feature's raw u32 / f32 tables (rows of kpad, msc_internal.hpp), k the group.
#pragma once

#include "family_math.hpp"

namespace msc {
namespace predpar {

// bb: P(v = 0)
MSC_DEV double bb_p0(const float *hp, const uint32_t *u, uint32_t kpad, uint32_t k) {
  const double h = u[k], t = u[kpad + k], a = hp[0], b = hp[1];
  return (b + t) / (a + b + h + t);
}

// gp: the Gamma shape of the rate and its scale
struct Gp { double shape, scale; };
MSC_DEV Gp gp(const float *hp, const uint32_t *u, uint32_t kpad, uint32_t k) {
  const double n = u[k], s = u[kpad + k];
  Gp p;
  p.shape = (double)hp[0] + s;
  p.scale = 1.0 / ((double)hp[1] + n);
  return p;
}

// bnb: the Beta's two parameters and r
struct Bnb { double a, b, r; };
MSC_DEV Bnb bnb(const float *hp, const uint32_t *u, uint32_t kpad, uint32_t k) {
  const double n = u[k], s = u[kpad + k], r = hp[2];
  Bnb p;
  p.a = (double)hp[0] + r * n;
  p.b = (double)hp[1] + s;
  p.r = r;
  return p;
}

// dd: category i's weight; the cumulative weights are their running sum from 0.0 in ascending i
MSC_DEV double dd_weight(const float *hp, const uint32_t *u, uint32_t kpad, uint32_t k, uint32_t i) {
  return (double)hp[i] + (double)u[(size_t)(1 + i) * kpad + k];
}

// nich: the Student-t's location, scale and degrees of freedom
struct Nich { double mu, scale, nu; };
MSC_DEV Nich nich(const float *hp, const uint32_t *u, const float *f, uint32_t kpad, uint32_t k) {
  const double n = u[k], mean = f[k], ctv = f[kpad + k];
  const double mu = hp[0], kappa = hp[1], sigmasq = hp[2], nu = hp[3];
  const double kn = kappa + n, nun = nu + n, dm = mu - mean;
  const double sigsq = (nu * sigmasq + ctv + n * kappa * dm * dm / kn) / nun;
  Nich p;
  p.mu = (kappa * mu + n * mean) / kn;
  p.scale = sqrt(sigsq * (kn + 1.0) / kn);
  p.nu = nun;
  return p;
}

}  // namespace predpar
}  // namespace msc
