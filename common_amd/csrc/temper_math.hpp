// temper_math.hpp -- what msc_chains_exchange / msc_chains_anneal_weights (kernels_temper.hip) fix that needs no device:
// the data log-likelihood of a chain from its joint row, the log ratio of a swap between two temperatures, the rule by
// which it is accepted, which rung pairs an exchange proposes, the ladder's walk, the annealing increment, and the checks
// of the calls' shapes; and of the sweep at a temperature (msc_chains_sweep_tempered, kernels_seq.hip) which temperatures a
// chain can be swept at and how a score partial goes onto a slot's score.  Host only: no HIP header, nothing else of the library but joint_math.hpp (the row's layout) --
// tests/cxx/temper_math_host.cpp builds it with the host compiler; the kernels and the entry points call the same functions.
//
// The tempered target of a chain at temperature beta is pi_beta(z) ~ p(z | alpha) p(X | z, hp)^beta.  With L_c = log p(X |
// z_c, hp) the swap of the temperatures of chains a and b is accepted with probability min(1, exp(r)),
//   r = (beta_a - beta_b) (L_b - L_a),
// and a step of annealed importance sampling from beta_from to beta_to multiplies a chain's weight by exp((beta_to -
// beta_from) L_c).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "joint_math.hpp"

// one rounding per operation in the functions below, on the device as on the host: nothing is fused
#if defined(__clang__)
#define MSC_TEMPER_EXACT _Pragma("clang fp contract(off)")
#else
#define MSC_TEMPER_EXACT
#endif

namespace msc {
namespace temper {

// L_c = ((d_0 + d_1) + ...) + d_{F-1} of a joint row, in double in that written order (0 with no feature): the
// features' entries [2, 2 + F) exactly as msc_chains_score_joint wrote them, one rounding per addition
MSC_JOINT_HD double chain_loglik(const double *row, uint32_t nfeat) {
  MSC_TEMPER_EXACT
  if (nfeat == 0) return 0.0;
  double l = row[joint::kJointData];
  for (uint32_t f = 1; f < nfeat; f++) l = l + row[joint::kJointData + f];
  return l;
}

// r of the swap between the chain at beta_a with likelihood la and the one at beta_b with lb: antisymmetric in the two
// chains' likelihoods and in their temperatures; the floats are widened first, so the difference is exact
MSC_JOINT_HD double swap_log_ratio(float beta_a, float beta_b, double la, double lb) {
  MSC_TEMPER_EXACT
  return ((double)beta_a - (double)beta_b) * (lb - la);
}

// log(u) < r, u uniform on [0, 1) (u == 0: log_u = -inf, below every finite r).  A non-finite r -- a NaN likelihood, inf -
// inf of two -inf ones, 0 * inf of equal temperatures -- rejects: a swap is never decided by a number that is none.
MSC_JOINT_HD bool swap_accepts(double log_u, double r) { return __builtin_isfinite(r) && log_u < r; }

// the neighbouring pairs (j, j + 1), j < nrungs - 1, an exchange of this parity proposes: j % 2 == parity % 2.  Disjoint,
// so their swaps do not touch each other; both parities in turn cover every pair.
MSC_JOINT_HD bool pair_active(uint32_t j, uint64_t parity) { return (j & 1u) == (uint32_t)(parity & 1u); }
MSC_JOINT_HD uint32_t ladder_pairs(uint32_t nrungs) { return nrungs > 0 ? nrungs - 1 : 0; }

// the chain of a ladder that holds rung j (its index within the ladder), nrungs when none does
MSC_JOINT_HD uint32_t rung_holder(const int32_t *rung, uint32_t nrungs, uint32_t j) {
  for (uint32_t i = 0; i < nrungs; i++)
    if (rung[i] == (int32_t)j) return i;
  return nrungs;
}

// every rung 0 .. nrungs - 1 held exactly once
MSC_JOINT_HD bool ladder_is_permutation(const int32_t *rung, uint32_t nrungs) {
  for (uint32_t j = 0; j < nrungs; j++) {
    uint32_t held = 0;
    for (uint32_t i = 0; i < nrungs; i++) held += rung[i] == (int32_t)j;
    if (held != 1) return false;
  }
  return true;
}

// One exchange of one ladder: its chains' joint rows at joint + i * ld_joint, temperatures beta[i] and rungs rung[i], i <
// nrungs; proposed / accepted: the ladder's nrungs - 1 counters, added to.  u01(j): the uniform of the pair (j, j + 1).
// Accepted swaps exchange the two chains' entries of beta and of rung -- the temperatures move, the states stay.  false,
// with nothing changed, when the rungs are no permutation.  One walker per ladder (a thread of k_chains_exchange): the
// holders are found by search, nrungs^2 steps, a ladder being a few dozen rungs.
template <class Uniform>
MSC_JOINT_HD bool exchange_ladder(const double *joint, uint64_t ld_joint, uint32_t nfeat, uint32_t nrungs, float *beta,
                                  int32_t *rung, uint64_t parity, Uniform u01, uint32_t *proposed, uint32_t *accepted) {
  if (!ladder_is_permutation(rung, nrungs)) return false;
  for (uint32_t j = 0; j + 1 < nrungs; j++) {
    if (!pair_active(j, parity)) continue;
    const uint32_t a = rung_holder(rung, nrungs, j), b = rung_holder(rung, nrungs, j + 1);
    const double la = chain_loglik(joint + (size_t)a * ld_joint, nfeat), lb = chain_loglik(joint + (size_t)b * ld_joint, nfeat);
    const double r = swap_log_ratio(beta[a], beta[b], la, lb);
    proposed[j] += 1u;
    if (!swap_accepts(std::log((double)u01(j)), r)) continue;
    accepted[j] += 1u;
    const float tb = beta[a];
    beta[a] = beta[b];
    beta[b] = tb;
    rung[a] = (int32_t)(j + 1);
    rung[b] = (int32_t)j;
  }
  return true;
}

// logw += (beta_to - beta_from) L.  Equal temperatures leave the weight untouched (false): 0 * an infinite L is no
// number, and a step that moves no temperature weighs nothing.
MSC_JOINT_HD bool anneal_step(float beta_from, float beta_to, double l, double *logw) {
  MSC_TEMPER_EXACT
  if (beta_to == beta_from) return false;
  *logw = *logw + ((double)beta_to - (double)beta_from) * l;
  return true;
}

// ---- the sweep at a temperature (msc_chains_sweep_tempered, k_sweep_seq_chains_tempered in kernels_seq.hip) ----
// A temperature a chain can be swept at: finite and >= 0 (-0.0f is 0; beta > 1 sharpens towards the MAP).  NaN, a negative
// or an infinite beta is none: its chain makes no visit and is reported (MSC_DEVERR_TEMPER_BETA).
MSC_JOINT_HD bool beta_ok(float beta) { return beta >= 0.f && __builtin_isfinite(beta); }

// One score partial of a slot -- the features' sum of one scoring slice -- going onto the slot's score sk at temperature
// beta: sk + beta * partial with ONE rounding, where the untempered sweep has sk + partial.  At beta = 1 the product is
// exact, so the bits are that add's; beta is not factored out of the slices' sum, which would round once more and
// elsewhere.  The caller adds no partial at beta == 0 (0 * -inf is no number).
MSC_JOINT_HD float tempered_add(float beta, float partial, float sk) { return __builtin_fmaf(beta, partial, sk); }

// ---- the calls' shape checks: ok, or the message of the first one that fails ----
inline joint::JointCheck check_exchange(const char *who, bool have_all, uint32_t nrungs, uint32_t nchains, uint64_t ld_joint,
                                        uint32_t nfeat) {
  if (!have_all) return joint::joint_fail("%s: null argument", who, 0, 0);
  if (nrungs == 0) return joint::joint_fail("%s: nrungs is 0", who, 0, 0);
  if (nchains % nrungs != 0)
    return joint::joint_fail("%s: %llu chains are no whole number of ladders of %llu rungs", who, nchains, nrungs);
  if (ld_joint < joint::joint_row(nfeat))
    return joint::joint_fail("%s: ld_joint %llu < nfeatures + 3 = %llu", who, ld_joint, joint::joint_row(nfeat));
  return joint::JointCheck();
}
inline joint::JointCheck check_anneal_weights(const char *who, bool have_all, uint64_t ld_joint, uint32_t nfeat) {
  if (!have_all) return joint::joint_fail("%s: null argument", who, 0, 0);
  if (ld_joint < joint::joint_row(nfeat))
    return joint::joint_fail("%s: ld_joint %llu < nfeatures + 3 = %llu", who, ld_joint, joint::joint_row(nfeat));
  return joint::JointCheck();
}

}  // namespace temper
}  // namespace msc
