// kernels_blocked_niw.hip -- gfx950 kernels of the blocked Gibbs sampler for a state of one Normal-Inverse-Wishart
// feature of dim <= 32 (msc_blocked_*, route_calls.hpp BlockedKernel::niw1): the exact sampler of the Dirichlet-process
// Gaussian mixture.  The stick weights are k_blocked_sticks' (kernels_blocked.hip), unchanged.
//   k_blocked_draw_niw      one 64-thread workgroup a slot: blocked_niw.hpp's draw_niw over two packed triangles in LDS
//                           -- posterior, Cholesky, L^-1, then one thread a matrix row: its normals and chi-square from
//                           the row's own stream and its row of V = T L^-1 -- then mu, V mu and the slice
//                           c = -(d / 2) ln 2 pi + sum ln V_ii.  Stored in double: mean[K][d], whiten[K][d (d + 1) / 2]
//                           (what msc_blocked_niw_params hands out) and, from the same doubles, V and V mu in the operand
//                           layout of the f64 matrix kernels (msc_internal.hpp niw_w_index / niw_b_index).
//   k_blocked_assign_niw<NB>  NB = 16-blocks of the dimension (1, 2).  A wave owns 64 rows as four blocks of 16; lane
//                           (c = lane & 15, kk = lane >> 4) holds feature 4 s + kk of row c of each block.  Per slot:
//                           acc = -(V mu), then V x on v_mfma_f64_16x16x4_f64 over the NB (NB + 1) / 2 chunks of the
//                           triangle (kernels_niw.hip k_score_niw64's contraction); D[i = kk + 4 reg][j = c], so
//                           q = |V x - V mu|^2 is a sum over a lane's registers and over the four lanes of a row;
//                           s = log pi_k + c_k - q / 2 in double.  Then k_blocked_assign's draw, per row: pass 1 an online
//                           max and sum of exp, pass 2 the same scores again (same code, same bits) and the CDF walk to
//                           u S.  No LDS, any K, nothing of size rows x K leaves the registers.  The four lanes of a
//                           row carry the same sums; lane row 0 stores.  A row's arithmetic depends on its own column of
//                           the matrix instruction alone: a sub-range draws what the whole draws.
#include "blocked_niw.hpp"
#include "family_math.hpp"
#include "launchers.hpp"
#include "score_block.hpp"

namespace msc {

// ---- the draw ----------------------------------------------------------------------------------------------------------
struct DevSync {
  __host__ __device__ void operator()() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

__global__ __launch_bounds__(64) void k_blocked_draw_niw(const BlkFeat *__restrict__ fs, uint32_t K, uint32_t kpad,
                                                          uint64_t key, uint64_t sweep, float *__restrict__ tab,
                                                          double *__restrict__ mean_out, double *__restrict__ whiten_out,
                                                          double *__restrict__ w64, double *__restrict__ mu64) {
  constexpr uint32_t D = blocked::kNiwMaxDim, NT = D * (D + 1) / 2;
  __shared__ double A[NT], Li[NT], mun[D], z[D], vmu[D], mean[D];
  const BlkFeat bf = fs[0];
  const uint32_t d = bf.dim, k = blockIdx.x, t = threadIdx.x;
  if (k >= K || d == 0 || d > D) return;           // (uniform over the workgroup)
  const float *sx = bf.raw_f32 + (size_t)k * (d + (size_t)d * d);
  float c = 0.f;
  blocked::draw_niw(d, bf.hp, (double)bf.raw_u32[k], sx, sx + d, key, k, sweep, bf.tag, A, Li, mun, z, vmu, mean, &c, t, 64u,
                    DevSync());
  if (t == 0) tab[(size_t)bf.slice0 * kpad + k] = c;
  const uint32_t nt = (uint32_t)blocked::ntri(d);
  for (uint32_t i = t; i < d; i += 64) mean_out[(size_t)k * d + i] = mean[i];
  for (uint32_t i = t; i < nt; i += 64) whiten_out[(size_t)k * nt + i] = A[i];
  // the operand stream: every slot of every chunk (zeros above the diagonal and beyond dim), as k_niw_prepare writes W
  const uint32_t nb = niw_blocks(d);
  double *W = w64 + (size_t)k * niw_w_stream(d);
  for (uint32_t b = 0; b < nb; b++)
    for (uint32_t s4 = 0; s4 <= b; s4++) {
      double *chunk = W + (size_t)(b * (b + 1u) / 2u + s4) * 256u;
      for (uint32_t slot = t; slot < 256u; slot += 64) {
        const uint32_t lane = slot >> 2, e = slot & 3u, i = 16u * b + (lane & 15u), j = 16u * s4 + 4u * e + (lane >> 4);
        chunk[slot] = (i < d && j <= i) ? A[blocked::tri(i, j)] : 0.0;
      }
    }
  double *B = mu64 + (size_t)k * niw_b_stream(d);
  for (uint32_t slot = t; slot < nb * 256u; slot += 64) {
    const uint32_t b = slot >> 8, lane = (slot >> 2) & 63u, r = slot & 3u, i = 16u * b + 4u * r + (lane >> 4);
    B[slot] = i < d ? vmu[i] : 0.0;
  }
}

// ---- the assignment ----------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// v + v[lane ^ 16], then that + its [lane ^ 32]: every lane of a row ends with the same bits (each step adds the same two
// numbers on both sides)
MSC_DEV double blk_niw_row_sum(double v) {
  u32x2 a = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(v), (unsigned)__double2loint(v), false, false);
  u32x2 b = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(v), (unsigned)__double2hiint(v), false, false);
  const double s = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
  a = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(s), (unsigned)__double2loint(s), false, false);
  b = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(s), (unsigned)__double2hiint(s), false, false);
  return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

constexpr int kBlkNiwJB = 4;                       // 16-row blocks a wave carries

// the scores of slot k for the wave's rows: s[jb] = log pi_k + c_k - |V_k x - V_k mu_k|^2 / 2 (a masked row: log pi_k)
template <int NB>
MSC_DEV void blk_niw_scores(const double *__restrict__ w64, const double *__restrict__ mu64, const float *__restrict__ logw,
                            const float *__restrict__ cs, uint32_t k, int lane, const float (&xf)[kBlkNiwJB][4 * NB],
                            const bool (&msk)[kBlkNiwJB], double (&s)[kBlkNiwJB]) {
  constexpr int JB = kBlkNiwJB, NCH = NB * (NB + 1) / 2;
  const double *Wk = w64 + (size_t)k * (NCH * 256) + lane * 4;
  const double *Bk = mu64 + (size_t)k * (NB * 256) + lane * 4;
  double qp[JB];
#pragma unroll
  for (int jb = 0; jb < JB; jb++) qp[jb] = 0.0;
#pragma unroll
  for (int b = 0; b < NB; b++) {
    const double2 b01 = *reinterpret_cast<const double2 *>(Bk + b * 256), b23 = *reinterpret_cast<const double2 *>(Bk + b * 256 + 2);
    f64x4 acc[JB];
#pragma unroll
    for (int jb = 0; jb < JB; jb++) acc[jb] = f64x4{-b01.x, -b01.y, -b23.x, -b23.y};   // V x - V mu
#pragma unroll
    for (int s4 = 0; s4 <= b; s4++) {
      const double *wc = Wk + (b * (b + 1) / 2 + s4) * 256;
      const double2 a01 = *reinterpret_cast<const double2 *>(wc), a23 = *reinterpret_cast<const double2 *>(wc + 2);
      const double a[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
      for (int e = 0; e < 4; e++)
#pragma unroll
        for (int jb = 0; jb < JB; jb++)
          acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], (double)xf[jb][4 * s4 + e], acc[jb], 0, 0, 0);
    }
#pragma unroll
    for (int jb = 0; jb < JB; jb++)
#pragma unroll
      for (int i = 0; i < 4; i++) qp[jb] = fma(acc[jb][i], acc[jb][i], qp[jb]);
  }
  const double lw = (double)logw[k], base = lw + (double)cs[k];
#pragma unroll
  for (int jb = 0; jb < JB; jb++) {
    const double q = blk_niw_row_sum(qp[jb]);      // over the four lanes c, c + 16, c + 32, c + 48
    s[jb] = msk[jb] ? lw : fma(-0.5, q, base);
  }
}

template <int NB>
__global__ __launch_bounds__(256) void k_blocked_assign_niw(const BlkFeat *__restrict__ fs, const float *__restrict__ tab,
                                                             const double *__restrict__ w64, const double *__restrict__ mu64,
                                                             uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows,
                                                             uint64_t row_id0, int32_t *__restrict__ z, uint64_t seed,
                                                             uint64_t sweep) {
  static_assert(NB == 1 || NB == 2, "dim <= 32");
  constexpr int JB = kBlkNiwJB, NS = 4 * NB;
  const BlkFeat bf = fs[0];
  const uint32_t d = bf.dim;
  const int lane = threadIdx.x & 63, c = lane & 15, kk = lane >> 4;
  const uint64_t rb = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (16 * JB);      // the wave's first row
  if (rb >= nrows) return;                         // (wave-uniform)
  const float *X = static_cast<const float *>(bf.col);
  const float *logw = tab, *cs = tab + (size_t)bf.slice0 * kpad;
  float xf[JB][NS];              // this lane's feature of every step, for its row of each block
  bool live[JB], msk[JB];
#pragma unroll
  for (int jb = 0; jb < JB; jb++) {
    const uint64_t r = rb + 16 * jb + c;
    live[jb] = r < nrows;
    const uint64_t vrow = row0 + (live[jb] ? r : 0);   // (a lane without a row scores row0's values and stores nothing)
    const float *xp = X + vrow * d;
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const bool has = (uint32_t)(4 * s + kk) < d;
      const float v = xp[has ? 4 * s + kk : 0];
      xf[jb][s] = has ? v : 0.0f;
    }
    msk[jb] = false;
    if (bf.mask != nullptr)
      for (uint32_t e = 0; e < d; e++) msk[jb] |= bf.mask[vrow * d + e] != 0;
  }
  // pass 1: online max (double: the scores are) and sum of exp (the max is kept finite)
  double m[JB];
  float S[JB];
#pragma unroll
  for (int jb = 0; jb < JB; jb++) m[jb] = -INFINITY, S[jb] = 0.f;
  for (uint32_t k = 0; k < K; k++) {
    double s[JB];
    blk_niw_scores<NB>(w64, mu64, logw, cs, k, lane, xf, msk, s);
#pragma unroll
    for (int jb = 0; jb < JB; jb++) {
      const double tm = fmax(fmax(m[jb], s[jb]), -1.0e300);
      S[jb] = S[jb] * __expf((float)(m[jb] - tm)) + __expf((float)(s[jb] - tm));   // (m = -inf at the first slot: exp gives 0)
      m[jb] = tm;
    }
  }
  // pass 2: the first slot whose running sum reaches u S = the number of slots whose running sum stays below it
  float t[JB], acc[JB];
  uint32_t pick[JB], last[JB];
#pragma unroll
  for (int jb = 0; jb < JB; jb++) {
    t[jb] = philox_uniform01(seed, sweep, row_id0 + rb + 16 * jb + c) * S[jb];
    acc[jb] = 0.f, pick[jb] = 0, last[jb] = 0;
  }
  for (uint32_t k = 0; k < K; k++) {
    double s[JB];
    blk_niw_scores<NB>(w64, mu64, logw, cs, k, lane, xf, msk, s);
    bool done = true;
#pragma unroll
    for (int jb = 0; jb < JB; jb++) {
      const float e = __expf((float)(s[jb] - m[jb]));
      acc[jb] += e;
      pick[jb] += acc[jb] < t[jb] ? 1u : 0u;
      last[jb] = e > 0.f ? k : last[jb];
      done = done && !(acc[jb] < t[jb]);
    }
    if (__all(done)) break;                        // (wave-uniform: every row of the wave has its slot)
  }
#pragma unroll
  for (int jb = 0; jb < JB; jb++) {
    // rounding left the last sum short of u S (pass 1 summed in another order): the last slot that added anything
    // (such a lane never let the loop end early, so `last` saw every slot)
    const uint32_t p = pick[jb] >= K ? last[jb] : pick[jb];
    if (live[jb] && kk == 0) z[rb + 16 * jb + c] = (int32_t)p;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int launch_blocked_draw_niw(hipStream_t stream, const BlkFeat *fs_dev, uint32_t K, uint32_t kpad, const uint32_t *cnt,
                            float alpha, uint64_t seed, uint64_t sweep, double *work, float *tab, double *mean,
                            double *whiten, double *w64, double *mu64) {
  // the stick weights and the (empty) per-thread draw as for every other state, then the slots' matrices
  if (launch_blocked_draw(stream, fs_dev, 0, K, kpad, cnt, alpha, seed, sweep, work, tab)) return MSC_EHIP;
  hipLaunchKernelGGL(k_blocked_draw_niw, dim3(K), dim3(64), 0, stream, fs_dev, K, kpad, seed ^ blocked::kKey, sweep, tab, mean,
                     whiten, w64, mu64);
  return launch_status("k_blocked_draw_niw");
}

int launch_blocked_assign_niw(hipStream_t stream, uint32_t dim, const BlkFeat *fs_dev, const float *tab, const double *w64,
                              const double *mu64, uint32_t K, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                              int32_t *z, uint64_t seed, uint64_t sweep) {
  if (nrows == 0) return 0;
  const dim3 grid((unsigned)((nrows + 64 * kBlkNiwJB - 1) / (64 * kBlkNiwJB)));
  if (niw_blocks(dim) == 1)
    hipLaunchKernelGGL((k_blocked_assign_niw<1>), (note_kernel(1, "k_blocked_assign_niw<1>"), grid), dim3(256), 0, stream,
                       fs_dev, tab, w64, mu64, K, kpad, row0, nrows, row_id0, z, seed, sweep);
  else
    hipLaunchKernelGGL((k_blocked_assign_niw<2>), (note_kernel(1, "k_blocked_assign_niw<2>"), grid), dim3(256), 0, stream,
                       fs_dev, tab, w64, mu64, K, kpad, row0, nrows, row_id0, z, seed, sweep);
  return launch_status("k_blocked_assign_niw");
}

}  // namespace msc
