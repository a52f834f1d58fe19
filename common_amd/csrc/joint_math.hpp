// joint_math.hpp -- what msc_score_joint / msc_chains_score_joint / msc_chains_keep_best (kernels_joint.hip) fix that
// needs no device: the order in which a row's total is added, the rule by which a sample replaces the best one kept, and
// the checks of the calls' shapes.  Host only: no HIP header, nothing else of the library -- tests/cxx/joint_math_host.cpp
// builds it with the host compiler; the kernels and the entry points call the same functions.
//
// A row of a joint score is nfeatures + 3 doubles:
//   [0]      the total  (((a + d_0) + d_1) + ... + d_{F-1}) + p, added in double in that written order (joint_total)
//   [1]      a = score_assignment(alpha) of the group counts
//   [2 + f]  d_f = the sum over the counted slots of score_data(hp_f, group)
//   [2 + F]  p = the sum of the hyper-priors given, in entry order (0 when none is given)
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define MSC_JOINT_HD __host__ __device__ inline
#else
#define MSC_JOINT_HD inline
#endif

namespace msc {
namespace joint {

constexpr uint32_t kJointTotal = 0, kJointAssign = 1, kJointData = 2;
MSC_JOINT_HD uint64_t joint_row(uint32_t nfeat) { return (uint64_t)nfeat + 3; }
MSC_JOINT_HD uint32_t joint_prior_at(uint32_t nfeat) { return nfeat + 2; }

// the total of a row from its parts as they lie in the row: a, then the features in index order, then p.  One rounding
// per addition, nothing fused or reassociated: a caller who downloads the parts and adds them in this order in double
// gets the bits of row[0].
MSC_JOINT_HD double joint_total(const double *row, uint32_t nfeat) {
  double t = row[kJointAssign];
  for (uint32_t f = 0; f < nfeat; f++) t = t + row[kJointData + f];
  return t + row[joint_prior_at(nfeat)];
}

// Does a sample of total `joint` replace a best of `best`?  Strictly greater only: a tie keeps the earlier sample (so
// the first of equal maxima is the one kept, and -0.0 against 0.0 either way is a tie), a NaN never wins, and a NaN or
// -inf that is the best so far loses only to something that compares greater -- which nothing does against a NaN, so a
// tracker starts from -inf, never from NaN.
MSC_JOINT_HD bool keep_best_wins(double joint, double best) { return joint > best; }

// ---- the calls' shape checks: ok, or the message of the first one that fails ----
struct JointCheck {
  bool ok = true;
  char message[192] = "";
};
inline JointCheck joint_fail(const char *fmt, const char *who, unsigned long long a, unsigned long long b) {
  JointCheck c;
  c.ok = false;
  std::snprintf(c.message, sizeof c.message, fmt, who, a, b);
  return c;
}

// msc_score_joint / msc_chains_score_joint: an output, coordinates when n says there are some, rows that hold a row of
// the score, a mask stride that is 0 (one mask for all chains) or holds ngroups bytes
inline JointCheck check_score_joint(const char *who, bool have_out, bool have_coords, uint32_t n, uint32_t nfeat,
                                    uint64_t ld_out, bool have_slots, uint64_t ld_slots, uint32_t ngroups) {
  if (!have_out) return joint_fail("%s: null output", who, 0, 0);
  if (n > 0 && !have_coords) return joint_fail("%s: %llu coordinates but a null list", who, n, 0);
  if (ld_out < joint_row(nfeat))
    return joint_fail("%s: ld_out %llu < nfeatures + 3 = %llu", who, ld_out, joint_row(nfeat));
  if (have_slots && ld_slots != 0 && ld_slots < ngroups)
    return joint_fail("%s: ld_slots %llu is neither 0 (one mask for all chains) nor >= ngroups %llu", who, ld_slots, ngroups);
  return JointCheck();
}

// msc_chains_keep_best: every array, a joint row that holds its total, z and best_z rows that hold nrows entries
inline JointCheck check_keep_best(const char *who, bool have_all, uint64_t ld_joint, uint64_t nrows, uint64_t ld_z,
                                  uint64_t ld_best) {
  if (!have_all) return joint_fail("%s: null argument", who, 0, 0);
  if (ld_joint < 1) return joint_fail("%s: ld_joint %llu < 1", who, ld_joint, 0);
  if (ld_z < nrows) return joint_fail("%s: ld_z %llu < nrows %llu", who, ld_z, nrows);
  if (ld_best < nrows) return joint_fail("%s: ld_best %llu < nrows %llu", who, ld_best, nrows);
  return JointCheck();
}

}  // namespace joint
}  // namespace msc
