// kernels_splitmerge.hip -- gfx950 kernels of the split-merge Metropolis-Hastings move (msc_split_merge,
// include/microscopes_hip.h; splitmerge_math.hpp has the streams and the arithmetic).  One proposal is a fixed chain of
// launches; a void or rejected proposal turns the later ones into no-ops through the device-side descriptor (SmProp):
//   k_sm_anchors      one workgroup: the ordered pair of anchors, their groups, the kind, the lowest empty slot
//   k_sm_coins        lane <-> row: the set S and the initial pair labels (-1 outside S, 0 / 1 at the anchors, a coin else)
//   k_sm_assign       lane <-> row, the restricted two-slot pass: a lane reads its row's z and leaves if the row is not in
//                     S; the others score pair slots 0 and 1 with blk_tile_scores (blocked_score.hpp: the slots' slices
//                     are wave-uniform operands, the first two of an aligned eight-slot stretch), form the two-way
//                     log-softmax with one exp and one log, and
//                       <MODE, false>  a launch pass: redraw the label of every free row
//                       <MODE, true>   the final pass: a split draws the final labels, a merge takes [z = z_j]; either
//                                      way log P(label | theta*) of the free rows is summed in double -- lanes by
//                                      shuffles, waves in wave order -- into the workgroup's partial
//                     MODEs as k_blocked_assign's (nich1, staged, global): the same order of a row's terms in all three
//   k_sm_merge_slots  additive tables of the pair state: slot 2 = slot 0 + slot 1 (the union S, for score_data)
//   k_sm_decide       one workgroup: the partials added in block order by one thread, log A in double, the dart, the
//                     log row and the counters
//   k_sm_relabel      lane <-> row: an accepted proposal moves its label-1 rows; the group-size table follows
// The coins kernel and the assign kernels also empty the pair state's additive tables for the accumulate pass that
// follows each of them.
#include "blocked_score.hpp"
#include "launchers.hpp"
#include "splitmerge_math.hpp"

namespace msc {

MSC_DEV void sm_zero_spans(const ZeroSpans &zs) {
  const size_t n = zs.na + zs.nb;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i < zs.na) zs.a[i] = 0ull;
    else zs.b[i - zs.na] = 0ull;
  }
}

__global__ __launch_bounds__(256) void k_sm_anchors(const int32_t *__restrict__ z, uint64_t nrows,
                                                     const uint32_t *__restrict__ cnt, uint32_t K, uint64_t key,
                                                     uint64_t sweep, SmProp *__restrict__ prop) {
  __shared__ uint32_t lowest;
  if (threadIdx.x == 0) lowest = K;
  __syncthreads();
  uint32_t mine = K;
  for (uint32_t k = threadIdx.x; k < K; k += blockDim.x)
    if (cnt[k] == 0) { mine = k; break; }
  if (mine < K) atomicMin(&lowest, mine);
  __syncthreads();
  if (threadIdx.x != 0) return;
  SmProp p;
  p.gi = p.gj = p.target = -1;
  p.kind = sm::kVoid;
  p.i = p.j = 0;
  p.accepted = 0;
  p.pad = 0;
  if (nrows >= 2) {
    sm::anchors(key, sweep, nrows, &p.i, &p.j);
    const int32_t gi = z[p.i], gj = z[p.j];
    if (gi >= 0 && (uint32_t)gi < K && gj >= 0 && (uint32_t)gj < K) {
      p.gi = gi;
      p.gj = gj;
      if (gi != gj) {
        p.kind = sm::kMerge;
        p.target = gi;
      } else if (lowest < K) {
        p.kind = sm::kSplit;
        p.target = (int32_t)lowest;
      }
    }
  }
  *prop = p;
}

__global__ __launch_bounds__(256) void k_sm_coins(const int32_t *__restrict__ z, uint64_t nrows, uint64_t row_id0,
                                                   const SmProp *__restrict__ prop, uint64_t key, uint64_t sweep,
                                                   int32_t *__restrict__ ell, ZeroSpans zero) {
  sm_zero_spans(zero);
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const SmProp p = *prop;
  int32_t lab = -1;
  if (p.kind != sm::kVoid) {
    const int32_t zr = z[r];
    if (zr == p.gi || zr == p.gj)
      lab = r == p.i ? 0 : r == p.j ? 1 : sm::uniform01(key, sweep, row_id0 + r) >= 0.5f ? 1 : 0;
  }
  ell[r] = lab;
}

template <int MODE, bool FINAL>
__global__ __launch_bounds__(256) void k_sm_assign(const BlkFeat *__restrict__ fs, int nfeat,
                                                    const float *__restrict__ tab, uint32_t kpad, uint64_t row0,
                                                    uint64_t nrows, uint64_t row_id0, const int32_t *__restrict__ z,
                                                    int32_t *__restrict__ ell, const SmProp *__restrict__ prop,
                                                    uint64_t key, uint64_t sweep, double *__restrict__ part,
                                                    ZeroSpans zero) {
  extern __shared__ uint32_t sm_lds[];             // MODE_STAGED: [nfeat][blockDim.x] codes (read as single dwords)
  __shared__ double wsum[4];                       // the waves' sums (at most four waves a workgroup)
  const uint32_t B = blockDim.x;
  const uint64_t r = (uint64_t)blockIdx.x * B + threadIdx.x;
  const SmProp p = *prop;
  bool in = r < nrows && p.kind != sm::kVoid;
  int32_t zr = -1;
  if (in) {
    zr = z[r];
    in = zr == p.gi || zr == p.gj;
  }
  double lq = 0.0;
  if (in) {
    const uint64_t vrow = row0 + r;
    uint32_t code1 = kBlkMasked;
    if (MODE == MODE_STAGED) {
      for (int f = 0; f < nfeat; f++) sm_lds[(size_t)f * B + threadIdx.x] = blk_code(fs[f], vrow);
      // (every lane reads back its own column only: no barrier)
    } else if (MODE == MODE_NICH1) {
      code1 = blk_code(fs[0], vrow);
    }
    float s[kBlkTile];
    blk_tile_scores<MODE>(fs, nfeat, tab, kpad, 0, sm_lds + threadIdx.x, B, vrow, code1, s);
    float lp0, lp1, p0;
    sm::two_way(s[0], s[1], &lp0, &lp1, &p0);
    const bool free_row = r != p.i && r != p.j;
    int32_t lab;
    if (FINAL && p.kind == sm::kMerge) lab = zr == p.gj ? 1 : 0;
    else if (!free_row) lab = r == p.j ? 1 : 0;
    else lab = sm::uniform01(key, sweep, row_id0 + r) < p0 ? 0 : 1;
    ell[r] = lab;
    if (FINAL && free_row) lq = (double)(lab ? lp1 : lp0);
  }
  if (FINAL) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lq += __shfl_down(lq, off, 64);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) wsum[wave] = lq;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (uint32_t w = 0; w < (B + 63u) / 64u; w++) t += wsum[w];
      part[blockIdx.x] = t;
    }
  }
  sm_zero_spans(zero);
}

__global__ __launch_bounds__(256) void k_sm_merge_slots(long long *__restrict__ i64, uint32_t rows_i,
                                                         double *__restrict__ f64, uint32_t rows_f, uint32_t kpad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < rows_i) {
    long long *a = i64 + (size_t)t * kpad;
    a[2] = a[0] + a[1];
  } else if (t - rows_i < rows_f) {
    double *a = f64 + (size_t)(t - rows_i) * kpad;
    a[2] = a[0] + a[1];
  }
}

constexpr uint32_t kSmChunk = 256;
__global__ __launch_bounds__(256) void k_sm_decide(SmProp *__restrict__ prop, const double *__restrict__ part,
                                                    uint32_t nparts, const float *__restrict__ sd, uint32_t nfeat,
                                                    const uint32_t *__restrict__ pair_cnt, float alpha, uint64_t key,
                                                    uint64_t sweep, double *__restrict__ log_row,
                                                    unsigned long long *__restrict__ counters) {
  __shared__ double sh[kSmChunk];
  __shared__ double tot[4];                        // log q, sd(0), sd(1), sd(S)
  const uint32_t t = threadIdx.x;
  const SmProp p = *prop;
  if (t < 4) tot[t] = 0.0;
  __syncthreads();
  if (p.kind != sm::kVoid) {
    // the workgroups' partials in block order, the features' score_data in feature order: staged by all, added by one
    for (uint32_t c0 = 0; c0 < nparts; c0 += kSmChunk) {
      const uint32_t n = nparts - c0 < kSmChunk ? nparts - c0 : kSmChunk;
      if (t < n) sh[t] = part[c0 + t];
      __syncthreads();
      if (t == 0) {
        double run = tot[0];
        for (uint32_t i = 0; i < n; i++) run += sh[i];
        tot[0] = run;
      }
      __syncthreads();
    }
    for (uint32_t slot = 0; slot < 3; slot++) {
      for (uint32_t c0 = 0; c0 < nfeat; c0 += kSmChunk) {
        const uint32_t n = nfeat - c0 < kSmChunk ? nfeat - c0 : kSmChunk;
        if (t < n) sh[t] = (double)sd[(size_t)(c0 + t) * 3 + slot];
        __syncthreads();
        if (t == 0) {
          double run = tot[1 + slot];
          for (uint32_t i = 0; i < n; i++) run += sh[i];
          tot[1 + slot] = run;
        }
        __syncthreads();
      }
    }
  }
  if (t != 0) return;
  double n0 = 0.0, n1 = 0.0, logq = 0.0, logA = 0.0;
  uint32_t accepted = 0;
  if (p.kind != sm::kVoid) {
    n0 = (double)pair_cnt[0];
    n1 = (double)pair_cnt[1];
    logq = tot[0];
    logA = sm::log_accept(p.kind, log((double)alpha), n0, n1, tot[1], tot[2], tot[3], logq);
    const double u = (double)sm::uniform01(key, sweep, sm::kDartAccept);
    accepted = log(u) < logA ? 1u : 0u;            // (u = 0: log gives -inf, accepted whenever log A is not NaN)
  }
  prop->accepted = accepted;
  if (log_row) {
    log_row[0] = (double)p.i;
    log_row[1] = (double)p.j;
    log_row[2] = (double)p.kind;
    log_row[3] = n0;
    log_row[4] = n1;
    log_row[5] = logq;
    log_row[6] = logA;
    log_row[7] = (double)accepted;
  }
  if (counters) {
    if (p.kind == sm::kVoid) counters[4] += 1ull;
    else {
      counters[2 * p.kind] += 1ull;
      counters[2 * p.kind + 1] += accepted;
    }
  }
}

__global__ __launch_bounds__(256) void k_sm_relabel(uint64_t nrows, int32_t *__restrict__ z,
                                                     const int32_t *__restrict__ ell, const SmProp *__restrict__ prop,
                                                     const uint32_t *__restrict__ pair_cnt, uint32_t *__restrict__ cnt) {
  const SmProp p = *prop;
  if (!p.accepted) return;
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nrows && ell[r] == 1) z[r] = p.target;
  if (r == 0) {
    const uint32_t n1 = pair_cnt[1];
    cnt[p.kind == sm::kSplit ? p.gi : p.gj] -= n1;
    cnt[p.target] += n1;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static dim3 sm_row_grid(uint64_t nrows, uint32_t block) { return dim3((unsigned)std::max<uint64_t>(1, (nrows + block - 1) / block)); }

int launch_sm_begin(hipStream_t stream, const int32_t *z, uint64_t nrows, uint64_t row_id0, const uint32_t *cnt, uint32_t K,
                    uint64_t seed, uint64_t sweep, SmProp *prop, int32_t *ell, ZeroSpans zero) {
  hipLaunchKernelGGL(k_sm_anchors, dim3(1), dim3(256), 0, stream, z, nrows, cnt, K, sm::stream_key(seed, sm::kStreamProposal),
                     sweep, prop);
  hipLaunchKernelGGL(k_sm_coins, sm_row_grid(nrows, 256), dim3(256), 0, stream, z, nrows, row_id0, prop,
                     sm::stream_key(seed, sm::kStreamCoin), sweep, ell, zero);
  return launch_status("k_sm_coins");
}

template <int MODE>
static void sm_assign_mode(hipStream_t stream, bool final, dim3 grid, uint32_t block, size_t lds, const BlkFeat *fs, int nfeat,
                           const float *tab, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0, const int32_t *z,
                           int32_t *ell, const SmProp *prop, uint64_t key, uint64_t sweep, double *part, ZeroSpans zero) {
  if (final)
    hipLaunchKernelGGL((k_sm_assign<MODE, true>), grid, dim3(block), lds, stream, fs, nfeat, tab, kpad, row0, nrows, row_id0, z,
                       ell, prop, key, sweep, part, zero);
  else
    hipLaunchKernelGGL((k_sm_assign<MODE, false>), grid, dim3(block), lds, stream, fs, nfeat, tab, kpad, row0, nrows, row_id0, z,
                       ell, prop, key, sweep, part, zero);
}

uint32_t sm_assign_blocks(uint64_t nrows, uint32_t block) { return sm_row_grid(nrows, block).x; }

int launch_sm_assign(hipStream_t stream, BlockedKernel kernel, uint32_t block, bool final, uint32_t pass, const BlkFeat *fs_dev,
                     int nfeat, const float *tab, uint32_t kpad, uint64_t row0, uint64_t nrows, uint64_t row_id0,
                     const int32_t *z, int32_t *ell, const SmProp *prop, uint64_t seed, uint64_t sweep, double *part,
                     ZeroSpans zero) {
  const dim3 grid = sm_row_grid(nrows, block);
  const uint64_t key = sm::stream_key(seed, sm::kStreamPass0 + pass);
  switch (kernel) {
    case BlockedKernel::nich1:
      note_kernel(1, "k_sm_assign<2, %s>", tf(final));
      sm_assign_mode<MODE_NICH1>(stream, final, grid, block, 0, fs_dev, nfeat, tab, kpad, row0, nrows, row_id0, z, ell, prop,
                                 key, sweep, part, zero);
      break;
    case BlockedKernel::staged:
      note_kernel(1, "k_sm_assign<1, %s>", tf(final));
      sm_assign_mode<MODE_STAGED>(stream, final, grid, block, (size_t)nfeat * block * sizeof(uint32_t), fs_dev, nfeat,
                                  tab, kpad, row0, nrows, row_id0, z, ell, prop, key, sweep, part, zero);
      break;
    case BlockedKernel::global:
      note_kernel(1, "k_sm_assign<0, %s>", tf(final));
      sm_assign_mode<MODE_GLOBAL>(stream, final, grid, block, 0, fs_dev, nfeat, tab, kpad, row0, nrows, row_id0, z, ell, prop,
                                  key, sweep, part, zero);
      break;
    case BlockedKernel::niw1:                      // (route_splitmerge refuses every niw state)
      return fail(MSC_EHIP, "k_sm_assign: no route sends a niw state here");
  }
  return launch_status("k_sm_assign");
}

int launch_sm_merge_slots(hipStream_t stream, long long *i64, uint32_t rows_i, double *f64, uint32_t rows_f, uint32_t kpad) {
  hipLaunchKernelGGL(k_sm_merge_slots, dim3((rows_i + rows_f + 255) / 256), dim3(256), 0, stream, i64, rows_i, f64, rows_f, kpad);
  return launch_status("k_sm_merge_slots");
}

int launch_sm_decide(hipStream_t stream, SmProp *prop, const double *part, uint32_t nparts, const float *sd, uint32_t nfeat,
                     const uint32_t *pair_cnt, float alpha, uint64_t seed, uint64_t sweep, double *log_row,
                     unsigned long long *counters) {
  hipLaunchKernelGGL(k_sm_decide, dim3(1), dim3(256), 0, stream, prop, part, nparts, sd, nfeat, pair_cnt, alpha,
                     sm::stream_key(seed, sm::kStreamProposal), sweep, log_row, counters);
  return launch_status("k_sm_decide");
}

int launch_sm_relabel(hipStream_t stream, uint64_t nrows, int32_t *z, const int32_t *ell, const SmProp *prop,
                      const uint32_t *pair_cnt, uint32_t *cnt) {
  hipLaunchKernelGGL(k_sm_relabel, sm_row_grid(nrows, 256), dim3(256), 0, stream, nrows, z, ell, prop, pair_cnt, cnt);
  return launch_status("k_sm_relabel");
}

}  // namespace msc
