// kernels_slice.hip -- gfx950 kernels of slice sampling (msc_hp_slice / msc_theta_slice, include/microscopes_hip.h):
//   k_hp_slice     one workgroup per target (a feature's chain of hp coordinates, or the CRP alpha): the whole update
//                  loop of every coordinate runs here, each evaluation of the target one pass of the workgroup over the
//                  feature's counted groups (staged in LDS once) and a fixed-order reduction
//   k_hp_slice_chains  the same body on a grid of (targets, chains): the step of every chain of an ensemble in one launch
//   k_theta_slice  one lane per (bbnc feature, counted slot): the slot's p, an O(1) target with ln B(alpha, beta) hoisted
// The update is Neal (2003), "Slice sampling", Fig. 3 (stepping out, at most m = 64 steps) and Fig. 5 (shrinkage), with
// every proposal rounded to float32 (what the tables hold) before the target is evaluated there, and the uniforms taken
// from Philox4x32-10 blocks of a counter of the update's own (the layout is in the header).  tests/slice_helpers.py
// restates the algorithm on the host, operation by operation.  No atomics on values and every sum in a fixed order: two
// calls on the same tables give the same bits, and so do the ranks of a sharded sweep.
#include <algorithm>

#include "family_math.hpp"
#include "launchers.hpp"
#include "pred_samplers.hpp"

namespace msc {

constexpr int kSliceThreads = 256;
constexpr int kSliceWaves = kSliceThreads / kWave;
constexpr uint32_t kSliceCap = 4096;    // counted slots staged in LDS, 3 words each (48 KiB); the rest are read in place
constexpr int kSliceStepOut = 64;       // m: at most m - 1 steps out, shared between the two ends
constexpr uint32_t kSliceShrink = 256;  // rejected proposals before an update keeps its value and counts as stalled

// the uniforms of one update: u_b from Philox4x32-10 block b of counter (c0, c1, c2, b), words 0 and 1, built as
// pred_samplers.hpp builds its two-word uniforms (in (0, 1))
struct SliceUniforms {
  uint32_t k0, k1, c0, c1, c2;
  MSC_DEV double u(uint32_t b) const {
    const uint32_t key[2] = {k0, k1}, ctr[4] = {c0, c1, c2, b};
    uint32_t o[4];
    pred::philox4x32_10(key, ctr, o);
    return ((double)(o[0] >> 5) * 67108864.0 + (double)(o[1] >> 6) + 0.5) * (1.0 / 9007199254740992.0);
  }
};

// One slice update of x0 with width w.  G: in_support(float) and operator()(float) -> the target at a point of its
// support.  The target is evaluated only inside its support (outside it is -inf); `evals` counts the evaluations, the
// one at x0 included.  status: kSliceOk, kSliceNonFinite (the target at x0 is not finite: x0 kept) or kSliceStalled (256
// proposals rejected, which takes an interval floating point has collapsed: x0 kept).
template <class G>
MSC_DEV float slice_update(G &g, float x0, double w, const SliceUniforms &r, uint32_t &evals, uint32_t &status) {
#pragma clang fp contract(off)   // the host twin does this arithmetic operation by operation
  // Written as one loop with ONE evaluation of the target (x0, then the left end, the right end, the proposals), which
  // k_hp_slice inlines as a pass of the workgroup: four call sites would be four copies of every family's score_data.
  uint32_t n = 0, j = 0;
  int phase = 0, J = 0, Kr = 0;              // 0: x0, 1: stepping out left, 2: right, 3: shrinking
  const double xd = (double)x0;
  double y = 0.0, L = 0.0, R = 0.0, z = xd;
  float x = x0;
  status = kSliceStalled;
  for (;;) {
    const float f = (float)z;                // the target is evaluated at float points only, inside its support only
    double gz = -INFINITY;
    if (g.in_support(f)) {
      n++;
      gz = g(f);
    }
    if (phase == 0) {
      if (!(fabs(gz) < INFINITY)) {          // (NaN included)
        status = kSliceNonFinite;
        break;
      }
      y = gz + log(r.u(0));
      L = xd - w * r.u(1);
      R = L + w;
      J = (int)floor((double)kSliceStepOut * r.u(2));
      Kr = kSliceStepOut - 1 - J;
      phase = 1;
    } else if (phase == 1) {
      if (y < gz) {
        L -= w;
        J--;
      } else {
        phase = 2;
      }
    } else if (phase == 2) {
      if (y < gz) {
        R += w;
        Kr--;
      } else {
        phase = 3;
      }
    } else {
      if (y < gz) {
        x = f;
        status = kSliceOk;
        break;
      }
      if ((double)f < xd) L = (double)f;
      else R = (double)f;
      j++;
    }
    if (phase == 1 && J == 0) phase = 2;
    if (phase == 2 && Kr == 0) phase = 3;
    if (phase == 1) z = L;
    else if (phase == 2) z = R;
    else if (j < kSliceShrink) z = L + r.u(3 + j) * (R - L);
    else break;                              // stalled: x0 kept
  }
  evals = n;
  return x;
}

// The target of one coordinate of k_hp_slice, evaluated by the whole workgroup: every thread holds the same values, so
// every thread takes the same branches and meets the same barriers.
struct HpSliceTarget {
  int family;                 // or kHpCluster
  uint32_t coord;
  bool positive;              // support x > 0 (else every finite x)
  float c0, c1, c2, c3;       // the feature's hp block as the chain has left it (scalars: an array indexed by a
                              // coordinate would live in scratch)
  uint32_t prior;
  double pa, pb, partner;
  // feature: slots [0, nst) staged (rows of kSliceCap words), the counted ones of [spill, K) read in place
  const uint32_t *su;
  const float *sf;
  uint32_t nst, spill, K, kpad;
  const uint32_t *raw_u32;
  const float *raw_f32;
  const uint32_t *cnt;
  const uint8_t *slots;
  double (*wred)[kSliceWaves];   // [2][waves] LDS, used alternately
  uint32_t parity;
  // alpha: the constant parts of score_assignment
  double occ, lg, nn;

  MSC_DEV float cur(uint32_t i) const { return i == 0 ? c0 : i == 1 ? c1 : i == 2 ? c2 : c3; }
  MSC_DEV void set(uint32_t i, float v) {
    c0 = i == 0 ? v : c0;
    c1 = i == 1 ? v : c1;
    c2 = i == 2 ? v : c2;
    c3 = i == 3 ? v : c3;
  }

  MSC_DEV bool in_support(float x) const { return positive ? (x > 0.f && x < INFINITY) : fabsf(x) < INFINITY; }

  // this thread's part of the sum over the counted slots, in slot order
  template <int F>
  MSC_DEV double pass(const float (&h)[4]) const {
    double acc = 0.0;
    const uint32_t ntot = nst + (K - spill);
    for (uint32_t i = threadIdx.x; i < ntot; i += kSliceThreads) {
      const bool staged = i < nst;
      const uint32_t k = staged ? i : spill + (i - nst);
      if (!staged && !(slots ? slots[k] != 0 : cnt[k] != 0u)) continue;
      acc += hp_eval(F, 0, h, h, staged ? su : raw_u32, staged ? sf : raw_f32, k, staged ? kSliceCap : kpad);
    }
    return acc;
  }

  MSC_DEV double likelihood(float x) {
    if (family == kHpCluster)                       // score_assignment(x), as k_crp_grid_score writes it
      return occ * log((double)x) + lg + lgamma((double)x) - lgamma(nn + (double)x);
    const float h[4] = {coord == 0 ? x : c0, coord == 1 ? x : c1, coord == 2 ? x : c2, coord == 3 ? x : c3};
    double acc = 0.0;
    switch (family) {                             // (one pass per family: the register budget is the largest one's)
      case MSC_BB: acc = pass<MSC_BB>(h); break;
      case MSC_BBNC: acc = pass<MSC_BBNC>(h); break;
      case MSC_GP: acc = pass<MSC_GP>(h); break;
      case MSC_BNB: acc = pass<MSC_BNB>(h); break;
      default: acc = pass<MSC_NICH>(h); break;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    double *buf = wred[parity];
    parity ^= 1u;
    if ((threadIdx.x & (kWave - 1)) == 0) buf[threadIdx.x / kWave] = acc;
    __syncthreads();
    return (buf[0] + buf[1]) + (buf[2] + buf[3]);
  }

  MSC_DEV double operator()(float x) { return likelihood(x) + slice_log_prior(prior, (double)x, pa, pb, partner); }
};
static_assert(kSliceWaves == 4, "HpSliceTarget::likelihood adds four wave partials");

// One target, one workgroup: the body of k_hp_slice and k_hp_slice_chains (one body, two kernels: a chain of the ensemble
// does the arithmetic of a single msc_hp_slice call on its state, in the same order).  Entry e of the target: Philox
// counter (T.target, e, sweep, b), key `key`.  alpha_out: null, or where the alpha target leaves the installed alpha.
MSC_DEV void hp_slice_target(const SliceTarget &T, const SliceCoord *__restrict__ coords, uint32_t K, uint32_t kpad,
                             const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ slots, uint64_t key,
                             uint32_t sweep_lo, float *__restrict__ values, uint32_t *__restrict__ evals,
                             uint32_t *__restrict__ status, float *alpha_out) {
  __shared__ uint32_t tab[3 * kSliceCap];
  __shared__ double wred[2][kSliceWaves];
  __shared__ double lg_s[kSliceThreads];
  __shared__ unsigned long long nn_s[kSliceThreads];
  __shared__ uint32_t occ_s[kSliceThreads];
  __shared__ uint32_t wcnt[kSliceWaves];
  __shared__ uint32_t spill_at;
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  HpSliceTarget g;
  g.family = T.family;
  g.wred = wred;
  g.parity = 0;
  g.K = K;
  g.kpad = kpad;
  g.cnt = cnt;
  g.slots = slots;
  g.raw_u32 = T.raw_u32;
  g.raw_f32 = T.raw_f32;
  g.su = tab;
  g.sf = reinterpret_cast<const float *>(tab + (size_t)T.nu32 * kSliceCap);
  g.nst = 0;
  g.spill = K;
  g.occ = g.lg = g.nn = 0.0;
  g.c0 = g.c1 = g.c2 = g.c3 = 0.f;
  if (T.family == kHpCluster) {
    // the group counts' part of score_assignment: strided partials, then a fixed LDS tree (k_crp_grid_score's order)
    double l = 0.0;
    unsigned long long n = 0;
    uint32_t o = 0;
    for (uint32_t k = threadIdx.x; k < K; k += kSliceThreads) {
      const uint32_t c = cnt[k];
      if (c) {
        l += lgamma((double)c);
        n += c;
        o++;
      }
    }
    lg_s[threadIdx.x] = l;
    nn_s[threadIdx.x] = n;
    occ_s[threadIdx.x] = o;
    for (uint32_t w = kSliceThreads / 2; w > 0; w >>= 1) {
      __syncthreads();
      if (threadIdx.x < w) {
        lg_s[threadIdx.x] += lg_s[threadIdx.x + w];
        nn_s[threadIdx.x] += nn_s[threadIdx.x + w];
        occ_s[threadIdx.x] += occ_s[threadIdx.x + w];
      }
    }
    __syncthreads();
    g.occ = (double)occ_s[0];
    g.lg = lg_s[0];
    g.nn = (double)nn_s[0];
    g.c0 = T.alpha;
  } else {
    // stage the counted slots' raw fields, in index order: the first kSliceCap of them in LDS, the rest read in place
    if (threadIdx.x == 0) spill_at = K;
    uint32_t base = 0;
    const uint32_t rows = T.nu32 + T.nf32;
    for (uint32_t c0 = 0; c0 < K; c0 += kSliceThreads) {
      const uint32_t k = c0 + threadIdx.x;
      const bool counted = k < K && (slots ? slots[k] != 0 : cnt[k] != 0u);
      const uint64_t b = __ballot(counted);
      if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
      __syncthreads();
      uint32_t pos = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      for (uint32_t w = 0; w < wave; w++) pos += wcnt[w];
      if (counted) {
        if (pos < kSliceCap) {
          for (uint32_t r = 0; r < rows; r++)
            tab[r * kSliceCap + pos] = r < T.nu32 ? T.raw_u32[(size_t)r * kpad + k]
                                                  : __float_as_uint(T.raw_f32[(size_t)(r - T.nu32) * kpad + k]);
        } else if (pos == kSliceCap) {
          spill_at = k;                               // the first counted slot that did not fit
        }
      }
      for (uint32_t w = 0; w < kSliceWaves; w++) base += wcnt[w];
      __syncthreads();
    }
    g.nst = min(base, kSliceCap);
    g.spill = spill_at;
    for (uint32_t i = 0; i < T.hpf; i++) g.set(i, T.hp[i]);
  }
  for (uint32_t e = 0; e < T.n; e++) {
    const SliceCoord C = coords[T.first + e];
    g.coord = C.coord;
    g.positive = !(T.family == MSC_NICH && C.coord == 0);   // nich mu: any real
    g.prior = C.prior;
    g.pa = (double)C.prior_a;
    g.pb = (double)C.prior_b;
    g.partner = (double)g.cur(C.partner);
    const SliceUniforms r{(uint32_t)key, (uint32_t)(key >> 32), T.target, e, sweep_lo};
    uint32_t ev, stt;
    const float x = slice_update(g, g.cur(C.coord), (double)C.width, r, ev, stt);
    g.set(C.coord, x);
    if (threadIdx.x == 0) {
      values[T.first + e] = x;
      evals[T.first + e] = ev;
      status[T.first + e] = stt;
    }
  }
  if (T.hp != nullptr && threadIdx.x < T.hpf) T.hp[threadIdx.x] = g.cur(threadIdx.x);
  if (alpha_out != nullptr && T.family == kHpCluster && threadIdx.x == 0) *alpha_out = g.c0;
}

// grid (targets), block kSliceThreads: the targets of one state
__global__ __launch_bounds__(kSliceThreads) void k_hp_slice(const SliceTarget *__restrict__ targets,
                                                            const SliceCoord *__restrict__ coords, uint32_t K,
                                                            uint32_t kpad, const uint32_t *__restrict__ cnt,
                                                            const uint8_t *__restrict__ slots, uint64_t key,
                                                            uint32_t sweep_lo, float *__restrict__ values,
                                                            uint32_t *__restrict__ evals, uint32_t *__restrict__ status) {
  hp_slice_target(targets[blockIdx.x], coords, K, kpad, cnt, slots, key, sweep_lo, values, evals, status, nullptr);
}

// grid (targets, chains), block kSliceThreads: workgroup (t, c) takes target t of chain c from targets[c][t] and what is
// per chain (counts, mask, key) from chains[c]; the coordinates are the ensemble's, the outputs [nchains][n]
__global__ __launch_bounds__(kSliceThreads) void k_hp_slice_chains(const SliceTarget *__restrict__ targets, HpChain *chains,
                                                                   const SliceCoord *__restrict__ coords, uint32_t n,
                                                                   uint32_t K, uint32_t kpad, uint32_t sweep_lo,
                                                                   float *__restrict__ values, uint32_t *__restrict__ evals,
                                                                   uint32_t *__restrict__ status) {
  const uint32_t c = blockIdx.y;
  HpChain &H = chains[c];
  const size_t at = (size_t)c * n;
  hp_slice_target(targets[(size_t)c * gridDim.x + blockIdx.x], coords, K, kpad, H.cnt, H.slots, H.key, sweep_lo, values + at,
                  evals + at, status + at, &H.alpha);
}

// the target of one bbnc slot: bbnc_score_data(hp, heads, tails, p) on (0, 1)
struct ThetaSliceTarget {
  float h[2];
  double lbeta;
  uint32_t heads, tails;
  MSC_DEV bool in_support(float p) const { return p > 0.f && p < 1.f; }
  MSC_DEV double operator()(float p) const { return bbnc_score_data_lb(h, heads, tails, p, lbeta); }
};

// grid (slot blocks, jobs), block 256: lane <-> slot.  Per (job, block): the evaluations its lanes took, and the first
// slot whose target at the current p is not finite (0xffffffff: none).
__global__ __launch_bounds__(256) void k_theta_slice(const ThetaJob *__restrict__ jobs, uint32_t K, uint32_t kpad,
                                                     const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ slots,
                                                     uint64_t key, uint32_t sweep_lo,
                                                     unsigned long long *__restrict__ evals_part,
                                                     uint32_t *__restrict__ bad_part) {
  __shared__ unsigned long long ev_s[256 / kWave];
  __shared__ uint32_t bad_s[256 / kWave];
  const ThetaJob &J = jobs[blockIdx.y];
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  unsigned long long ev = 0;
  uint32_t bad = 0xffffffffu;
  if (k < K && (slots ? slots[k] != 0 : cnt[k] != 0u)) {
    ThetaSliceTarget g;
    g.h[0] = J.hp[0];
    g.h[1] = J.hp[1];
    g.lbeta = bbnc_lbeta(g.h);
    g.heads = J.raw_u32[k];
    g.tails = J.raw_u32[kpad + k];
    const SliceUniforms r{(uint32_t)key, (uint32_t)(key >> 32), k, 0x80000000u | J.feature, sweep_lo};
    uint32_t e, stt;
    const float p = slice_update(g, J.raw_f32[k], (double)J.width, r, e, stt);
    ev = e;
    if (stt == kSliceNonFinite) bad = k;
    else J.raw_f32[k] = p;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    ev += __shfl_xor(ev, off);
    bad = min(bad, (uint32_t)__shfl_xor((int)bad, off));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    ev_s[threadIdx.x / kWave] = ev;
    bad_s[threadIdx.x / kWave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    uint32_t b = 0xffffffffu;
    for (int w = 0; w < 256 / kWave; w++) {
      t += ev_s[w];
      b = min(b, bad_s[w]);
    }
    evals_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    bad_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = b;
  }
}

int launch_hp_slice(hipStream_t stream, const SliceTarget *targets_dev, uint32_t ntargets, const SliceCoord *coords_dev,
                    uint32_t K, uint32_t kpad, const uint32_t *cnt, const uint8_t *slots, uint64_t key, uint64_t sweep,
                    float *values, uint32_t *evals, uint32_t *status) {
  hipLaunchKernelGGL(k_hp_slice, dim3(ntargets), dim3(kSliceThreads), 0, stream, targets_dev, coords_dev, K, kpad, cnt,
                     slots, key, (uint32_t)sweep, values, evals, status);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_hp_slice_chains(hipStream_t stream, const SliceTarget *targets_dev, uint32_t ntargets, HpChain *chains_dev,
                           uint32_t nchains, const SliceCoord *coords_dev, uint32_t n, uint32_t K, uint32_t kpad,
                           uint64_t sweep, float *values, uint32_t *evals, uint32_t *status) {
  for (uint32_t c0 = 0; c0 < nchains; c0 += kMaxGridYZ) {          // (a grid's y extent ends at 65535)
    const uint32_t nc = std::min(kMaxGridYZ, nchains - c0);
    const size_t at = (size_t)c0 * n;
    hipLaunchKernelGGL(k_hp_slice_chains, dim3(ntargets, nc), dim3(kSliceThreads), 0, stream,
                       targets_dev + (size_t)c0 * ntargets, chains_dev + c0, coords_dev, n, K, kpad, (uint32_t)sweep,
                       values + at, evals + at, status + at);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_theta_slice(hipStream_t stream, const ThetaJob *jobs_dev, uint32_t njobs, uint32_t K, uint32_t kpad,
                       const uint32_t *cnt, const uint8_t *slots, uint64_t key, uint64_t sweep,
                       unsigned long long *evals_part, uint32_t *bad_part) {
  hipLaunchKernelGGL(k_theta_slice, dim3(theta_slice_blocks(K), njobs), dim3(256), 0, stream, jobs_dev, K, kpad, cnt,
                     slots, key, (uint32_t)sweep, evals_part, bad_part);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
