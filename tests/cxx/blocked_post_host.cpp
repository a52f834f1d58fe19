// Host build of common_amd/csrc/blocked_post.hpp for tests/test_blocked_cpu.py: the posterior parameters and the
// parameter draws of the blocked Gibbs sampler, driven from ctypes.  Draw i of a batch reads the stream of
// (seed ^ kKey, slot = i, sweep = 0, feature = 0), as slot i of a device draw with that seed does.
#include <cstdint>
#include <vector>

#include "blocked_post.hpp"

using namespace msc;
using namespace msc::blocked;

enum { F_BB = 0, F_GP = 1, F_DD = 2, F_NICH = 3, F_BNB = 7 };   // msc_family

extern "C" {

uint64_t blk_key() { return kKey; }
double blk_truncation_bound(double nrows, uint32_t K, double alpha) { return truncation_bound(nrows, K, alpha); }

// posterior parameters of one slot: su = the record's uint32 fields, sf its float fields, out = up to four doubles
// (bb a, b; gp shape, rate; bnb a, b; nich mu', kappa', sigmasq', nu'; dd: dim concentrations)
void blk_post(int family, uint32_t dim, const float *hp, const uint32_t *su, const float *sf, double *out) {
  switch (family) {
    case F_BB: bb_post(hp, su[0], su[1], &out[0], &out[1]); break;
    case F_GP: gp_post(hp, su[0], su[1], &out[0], &out[1]); break;
    case F_BNB: bnb_post(hp, su[0], su[1], &out[0], &out[1]); break;
    case F_NICH: nich_post(hp, su[0], sf[0], sf[1], &out[0], &out[1], &out[2], &out[3]); break;
    case F_DD:
      for (uint32_t i = 0; i < dim; i++) out[i] = (double)hp[i] + (double)su[1 + i];
      break;
    default: break;
  }
}

// n draws of one slot's slices from (hp, suff-stats): out = float[n][nslices]
void blk_draw(int family, uint32_t dim, const float *hp, const uint32_t *su, const float *sf, uint64_t n, uint64_t seed,
              float *out) {
  const uint64_t key = seed ^ kKey;
  double p[4];
  if (family != F_DD) blk_post(family, dim, hp, su, sf, p);
  for (uint64_t i = 0; i < n; i++) {
    pred::Stream s(key, i, 0, 0);
    switch (family) {
      case F_BB: draw_bb(s, p[0], p[1], out + 2 * i, 1); break;
      case F_GP: draw_gp(s, p[0], p[1], out + 2 * i, 1); break;
      case F_BNB: draw_bnb(s, p[0], p[1], (double)hp[2], out + 2 * i, 1); break;
      case F_NICH: draw_nich(s, p[0], p[1], p[2], p[3], out + 3 * i, 1); break;
      case F_DD: draw_dd(key, i, 0, 0, dim, hp, su + 1, 1, out + (size_t)dim * i, 1); break;
      default: break;
    }
  }
}

// the stick weights of K slots with the counts cnt, as k_blocked_sticks forms them: log_v, log_w = double[K]
void blk_sticks(const uint32_t *cnt, uint32_t K, double alpha, uint64_t seed, uint64_t sweep, double *log_v, double *log_w) {
  const uint64_t key = seed ^ kKey;
  std::vector<double> after(K, 0.0), l1(K, 0.0);
  double run = 0.0;
  for (uint32_t k = K; k-- > 0;) { after[k] = run; run += (double)cnt[k]; }
  for (uint32_t k = 0; k < K; k++) {
    double a, b;
    stick_post((double)cnt[k], after[k], alpha, &a, &b);
    pred::Stream s(key, k, sweep, kStickTag);
    draw_stick(s, a, b, k + 1 == K, &log_v[k], &l1[k]);
  }
  run = 0.0;
  for (uint32_t k = 0; k < K; k++) { log_w[k] = (double)fin(log_v[k] + run); run += l1[k]; }
}
}
