// kernels_pred.hip -- gfx950 kernels of posterior predictive sampling (msc_sample_predictive, include/microscopes_hip.h):
//   k_pred_prepare      one thread per (feature, group): raw suff-stats + hp -> the group's predictive parameters, in double
//                       (the formulas: pred_params.hpp, shared with the ensemble's draw)
//   k_pred_prepare_niw  one wave per niw group: mu', the lower Cholesky factor of the predictive scale, dof -- the factor is
//                       the inverse of the whitening matrix k_niw_prepare already made (no second factorisation)
//   k_pred_sample       one lane per row, the scalar features looped: every output column store is coalesced; <false>
//                       copies observed entries and makes the one-uniform draws, <true> the rejection families' draws
//   k_pred_sample_niw   one lane per row for one niw feature: d normals through LDS, L z, sqrt(dof / chi2); the rows are
//                       stored through LDS, coalesced
// The formulas are the host sampler's (include/microscopes_amd/hip_models.hpp detail::sampler), the variates those of
// pred_samplers.hpp, whose header comment also fixes the Philox counter of every draw.
#include "family_math.hpp"
#include "launchers.hpp"
#include "pred_params.hpp"
#include "pred_samplers.hpp"

namespace msc {

constexpr int kPredNiwLanes = 64;       // rows of a k_pred_sample_niw workgroup; its z vectors are [dim][65] doubles of LDS

MSC_DEV size_t pred_tri(uint32_t i, uint32_t j) { return (size_t)i * (i + 1u) / 2u + j; }

__global__ __launch_bounds__(256) void k_pred_prepare(const PredFeat *__restrict__ pfs, uint32_t K, uint32_t kpad) {
  const PredFeat &pf = pfs[blockIdx.y];
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K || pf.family == MSC_NIW) return;
  const float *hp = pf.hp;
  const uint32_t *u = pf.raw_u32;
  double *par = pf.par + (size_t)k * pf.stride;
  switch (pf.family) {
    case MSC_BB: par[0] = predpar::bb_p0(hp, u, kpad, k); break;                       // P(v = 0)
    case MSC_BBNC: par[0] = 1.0 - (double)pf.raw_f32[k]; break;
    case MSC_GP: {
      const predpar::Gp p = predpar::gp(hp, u, kpad, k);
      par[0] = p.shape;                                           // Gamma shape of the rate
      par[1] = p.scale;                                           // and its scale
      break;
    }
    case MSC_BNB: {
      const predpar::Bnb p = predpar::bnb(hp, u, kpad, k);
      par[0] = p.a;
      par[1] = p.b;
      par[2] = p.r;
      break;
    }
    case MSC_DD: {
      double c = 0.0;
      for (uint32_t i = 0; i < pf.dim; i++) {
        c += predpar::dd_weight(hp, u, kpad, k, i);
        par[i] = c;                                               // cumulative weights; par[dim - 1] is the total
      }
      break;
    }
    case MSC_NICH: {
      const predpar::Nich p = predpar::nich(hp, u, pf.raw_f32, kpad, k);
      par[0] = p.mu;
      par[1] = p.scale;
      par[2] = p.nu;
      break;
    }
    default: break;
  }
}

// group k of a niw feature: par = {mu'[d], L packed lower triangle (tri(i, j)), dof}.  k_niw_prepare stored
// W = chol(Psi')^-1 sqrt(kn / (kn + 1)); the predictive scale Sigma = Psi' (kn + 1) / (kn dof) has the factor
// W^-1 / sqrt(dof): lane c solves W y = e_c for column c.
__global__ __launch_bounds__(64) void k_pred_prepare_niw(const PredFeat *__restrict__ pfs, uint32_t i_feat, uint32_t K) {
  const PredFeat &pf = pfs[i_feat];
  const uint32_t k = blockIdx.x, d = pf.dim, t = threadIdx.x;
  if (k >= K) return;
  const float *hp = pf.hp;
  const double kappa = hp[0], nu = hp[1];
  const double n = pf.raw_u32[k], kn = kappa + n, dof = nu + n - (double)d + 1.0;
  const float *sx = pf.raw_f32 + (size_t)k * (d + (size_t)d * d);
  const double *W = pf.niw_w64 + (size_t)k * niw_w_stream(d);
  double *par = pf.par + (size_t)k * pf.stride, *L = par + d;
  for (uint32_t i = t; i < d; i += 64) par[i] = (kappa * (double)hp[2 + i] + (double)sx[i]) / kn;
  const double rs = 1.0 / sqrt(dof);
  for (uint32_t c = t; c < d; c += 64) {
    L[pred_tri(c, c)] = 1.0 / W[niw_w_index(c, c)];
    for (uint32_t i = c + 1; i < d; i++) {
      double s = 0.0;
      for (uint32_t m = c; m < i; m++) s += W[niw_w_index(i, m)] * L[pred_tri(m, c)];
      L[pred_tri(i, c)] = -s / W[niw_w_index(i, i)];
    }
    for (uint32_t i = c; i < d; i++) L[pred_tri(i, c)] *= rs;
  }
  if (t == 0) par[d + pred_tri(d, 0)] = dof;                     // (tri(d, 0) = the triangle's size)
}

// the group of row r, or -1 when it is skipped
MSC_DEV int32_t pred_group(const int32_t *z, uint64_t r, uint32_t K) {
  const int32_t g = z[r];
  return (g < 0 || (uint32_t)g >= K) ? -1 : g;
}

// a family whose draw runs a rejection loop (Gamma, Poisson, Student-t): drawn by k_pred_sample<true>
MSC_DEV bool pred_heavy(int family) { return family == MSC_GP || family == MSC_BNB || family == MSC_NICH; }

// HEAVY = false: z_out, the copies of observed entries, and the one-uniform draws (bb, bbnc, dd) -- the memory-bound part,
// few registers; HEAVY = true: the draws of the rejection families only (their generators inlined, many registers)
template <bool HEAVY>
__global__ __launch_bounds__(256) void k_pred_sample(const PredFeat *__restrict__ pfs, uint32_t npf, uint32_t K,
                                                     uint64_t row0, uint64_t nrows, uint64_t row_id0,
                                                     const int32_t *__restrict__ z, int32_t *__restrict__ z_out,
                                                     uint32_t masked_only, uint64_t seed, uint64_t sweep) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const int32_t g = pred_group(z, r, K);
  if (g < 0) return;
  if (!HEAVY && z_out) z_out[r] = g;
  const uint64_t vrow = row0 + r, grow = row_id0 + r;
  for (uint32_t i = 0; i < npf; i++) {
    const PredFeat &pf = pfs[i];
    if (pf.family == MSC_NIW) continue;                            // (k_pred_sample_niw)
    if (masked_only && !(pf.mask != nullptr && pf.mask[vrow] != 0)) {
      if (HEAVY) continue;
      switch (pf.family) {                                         // observed: the view's value, as the model reads it
        case MSC_BB:
        case MSC_BBNC: static_cast<uint8_t *>(pf.out)[r] = static_cast<const uint8_t *>(pf.col)[vrow] != 0; break;
        case MSC_NICH: static_cast<float *>(pf.out)[r] = static_cast<const float *>(pf.col)[vrow]; break;
        default: static_cast<uint32_t *>(pf.out)[r] = static_cast<const uint32_t *>(pf.col)[vrow]; break;
      }
      continue;
    }
    if (pred_heavy(pf.family) != HEAVY) continue;
    const double *par = pf.par + (size_t)g * pf.stride;
    pred::Stream s(seed, grow, sweep, pf.feature);
    if (!HEAVY) {
      if (pf.family == MSC_DD) {
        const double t = s.u24() * par[pf.dim - 1];
        int32_t v = (int32_t)pf.dim - 1;
        for (uint32_t j = 0; j + 1 < pf.dim; j++)
          if (t < par[j]) { v = (int32_t)j; break; }
        static_cast<int32_t *>(pf.out)[r] = v;
      } else {
        static_cast<uint8_t *>(pf.out)[r] = s.u24() >= par[0] ? 1 : 0;   // bb, bbnc
      }
      continue;
    }
    switch (pf.family) {
      case MSC_GP: static_cast<uint32_t *>(pf.out)[r] = pred::poisson(s, pred::gamma1(s, par[0]) * par[1]); break;
      case MSC_BNB: {
        const double p = fmax(pred::beta(s, par[0], par[1]), 1e-300);  // (a Beta draw that underflowed: no 1/0)
        const double rate = pred::gamma1(s, par[2]) * (1.0 - p) / p;   // failures before the r-th success
        static_cast<uint32_t *>(pf.out)[r] = pred::poisson(s, rate);
        break;
      }
      default: static_cast<float *>(pf.out)[r] = (float)(par[0] + par[1] * pred::student_t(s, par[2])); break;
    }
  }
}

// One lane per row of one niw feature.  The normals of lane l sit in LDS column l of [dim][kPredNiwStride] doubles;
// x = mu' + w L z is formed from the last element to the first, each element written over the normal of its own index
// (element i needs z_0 .. z_i only), and the workgroup's 64 rows of dim floats -- one contiguous stretch of out -- are
// then stored element by element across the lanes: coalesced, where a lane storing its own row would stride by dim * 4.
constexpr uint32_t kPredNiwStride = kPredNiwLanes + 1;   // (an odd stride: the store phase's reads hit distinct banks)
__global__ __launch_bounds__(kPredNiwLanes) void k_pred_sample_niw(const PredFeat *__restrict__ pfs, uint32_t i_feat,
                                                                   uint32_t K, uint64_t row0, uint64_t nrows,
                                                                   uint64_t row_id0, const int32_t *__restrict__ z,
                                                                   uint32_t masked_only, uint64_t seed, uint64_t sweep) {
  extern __shared__ double zs[];                                   // [dim][kPredNiwStride], then act[kPredNiwLanes]
  const PredFeat &pf = pfs[i_feat];
  const uint32_t d = pf.dim, lane = threadIdx.x;
  uint32_t *act = reinterpret_cast<uint32_t *>(zs + (size_t)d * kPredNiwStride);   // does the row get stored
  const uint64_t rb = (uint64_t)blockIdx.x * kPredNiwLanes, r = rb + lane;
  const int32_t g = r < nrows ? pred_group(z, r, K) : -1;
  act[lane] = g >= 0;
  if (g >= 0) {
    const uint64_t vrow = row0 + r;
    bool draw = true;
    if (masked_only) {
      bool any = false;
      if (pf.mask != nullptr)
        for (uint32_t i = 0; i < d; i++) any |= pf.mask[(size_t)vrow * d + i] != 0;
      draw = any;
    }
    if (!draw) {                                                   // observed whole: copied
      const float *col = static_cast<const float *>(pf.col) + (size_t)vrow * d;
      for (uint32_t i = 0; i < d; i++) zs[(size_t)i * kPredNiwStride + lane] = (double)col[i];
    } else {
      pred::Stream s(seed, row_id0 + r, sweep, pf.feature);
      for (uint32_t i = 0; i < d; i++) zs[(size_t)i * kPredNiwStride + lane] = s.normal();
      const double *par = pf.par + (size_t)g * pf.stride, *L = par + d;
      const double dof = par[d + pred_tri(d, 0)];
      const double w = sqrt(dof / pred::chi2(s, dof));
      for (uint32_t i = d; i-- > 0;) {
        double x = 0.0;
        const double *Li = L + pred_tri(i, 0);
        for (uint32_t k = 0; k <= i; k++) x += Li[k] * zs[(size_t)k * kPredNiwStride + lane];
        zs[(size_t)i * kPredNiwStride + lane] = (double)(float)(par[i] + x * w);
      }
    }
  }
  __syncthreads();
  const uint64_t nb = nrows - rb < (uint64_t)kPredNiwLanes ? nrows - rb : (uint64_t)kPredNiwLanes;
  float *out = static_cast<float *>(pf.out) + (size_t)rb * d;
  for (uint64_t e = lane; e < nb * d; e += kPredNiwLanes) {
    const uint32_t row = (uint32_t)(e / d), i = (uint32_t)(e - (uint64_t)row * d);
    if (act[row]) out[e] = (float)zs[(size_t)i * kPredNiwStride + row];
  }
}

int launch_pred_prepare(hipStream_t stream, const PredFeat *pfs_dev, const std::vector<PredFeat> &pfs, uint32_t K,
                        uint32_t kpad) {
  if (pfs.empty()) return 0;
  hipLaunchKernelGGL(k_pred_prepare, dim3((K + 255) / 256, (uint32_t)pfs.size()), dim3(256), 0, stream, pfs_dev, K, kpad);
  for (uint32_t i = 0; i < pfs.size(); i++)
    if (pfs[i].family == MSC_NIW)
      hipLaunchKernelGGL(k_pred_prepare_niw, dim3(K), dim3(64), 0, stream, pfs_dev, i, K);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_sample(hipStream_t stream, const PredFeat *pfs_dev, const std::vector<PredFeat> &pfs, uint32_t K,
                       uint64_t row0, uint64_t nrows, uint64_t row_id0, const int32_t *z, int32_t *z_out,
                       bool masked_only, uint64_t seed, uint64_t sweep) {
  if (nrows == 0) return 0;
  bool light = z_out != nullptr, heavy = false;
  for (const PredFeat &pf : pfs) {
    light |= pf.family != MSC_NIW;
    heavy |= pf.family == MSC_GP || pf.family == MSC_BNB || pf.family == MSC_NICH;
  }
  const dim3 grid((uint32_t)((nrows + 255) / 256));
  if (light)
    hipLaunchKernelGGL(k_pred_sample<false>, grid, dim3(256), 0, stream, pfs_dev, (uint32_t)pfs.size(), K, row0, nrows,
                       row_id0, z, z_out, masked_only ? 1u : 0u, seed, sweep);
  if (heavy)
    hipLaunchKernelGGL(k_pred_sample<true>, grid, dim3(256), 0, stream, pfs_dev, (uint32_t)pfs.size(), K, row0, nrows,
                       row_id0, z, z_out, masked_only ? 1u : 0u, seed, sweep);
  for (uint32_t i = 0; i < pfs.size(); i++)
    if (pfs[i].family == MSC_NIW) {
      const size_t lds = (size_t)pfs[i].dim * kPredNiwStride * sizeof(double) + kPredNiwLanes * sizeof(uint32_t);
      if (lds > 64 * 1024 &&                                        // (dim 128: 65 KiB)
          hipFuncSetAttribute(reinterpret_cast<const void *>(k_pred_sample_niw),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
      hipLaunchKernelGGL(k_pred_sample_niw, dim3((uint32_t)((nrows + kPredNiwLanes - 1) / kPredNiwLanes)),
                         dim3(kPredNiwLanes), lds, stream, pfs_dev, i, K, row0, nrows, row_id0, z,
                         masked_only ? 1u : 0u, seed, sweep);
    }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace msc
