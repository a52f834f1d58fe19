// msc_internal.hpp -- host-side objects behind include/microscopes_hip.h and the
// plain-old-data descriptors shared with the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/microscopes_hip.h"
#include "dev_buf.hpp"
#include "feat_desc.hpp"
#include "route.hpp"
#include "step_rules.hpp"
#include "table_validity.hpp"

namespace msc {

constexpr int kWave = 64;          // gfx950 wavefront
constexpr unsigned kMaxDDDim = 128;
constexpr float kNtFastGbps = 6650.f;    // probe fill rate from which a placed buffer takes non-temporal stores (msc_context::placed)

// ---- error plumbing --------------------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define MSC_HIP(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return ::msc::fail(MSC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                         __FILE__, __LINE__);                                            \
  } while (0)

#define MSC_REQUIRE(cond, ...)                                    \
  do {                                                            \
    if (!(cond)) return ::msc::fail(MSC_EINVAL, __VA_ARGS__);     \
  } while (0)

#define MSC_TRY(expr)                \
  do {                               \
    int _s = (expr);                 \
    if (_s != MSC_OK) return _s;     \
  } while (0)

inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// the CRP table (msc_state::logpc; kernels_score.hip crp_prepare_block): float offsets of the low halves
__host__ __device__ inline size_t crp_lo_cnt(uint32_t kpad) { return 2 * (size_t)kpad + 4; }     // lo of log(cnt)
__host__ __device__ inline size_t crp_lo_cntm1(uint32_t kpad) { return 3 * (size_t)kpad + 4; }   // lo of log(cnt - 1)
inline size_t crp_floats(uint32_t kpad) { return 4 * (size_t)kpad + 4; }

// One grid of hyper-parameter points as the kernels of kernels_hp.hip read it (msc_hp_grid_*): a feature's grid, or the
// CRP concentration's (family kHpCluster, one float per point, no tables).  The score kernel writes per (group block,
// point) partial sums at part_off, the reduce kernel their fixed-order sum at out_off; the draw kernel reads those,
// writes prior + likelihood to scores_out (nullable) and the chosen block into hp_dst (+ its alpha sum into aux_dst).
constexpr int32_t kHpCluster = -1;
struct HpJob {
  int32_t family;
  uint32_t dim;
  uint32_t hpf;              // floats per point (msc_hp_floats)
  uint32_t npoints;
  uint32_t nu32, nf32;       // raw table rows of the family (raw_u32_rows / raw_f32_rows)
  const float *grid;         // [npoints][hpf] (device)
  const double *logprior;    // [npoints] (device) or null
  const uint32_t *raw_u32;   // the feature's raw tables, rows of kpad
  const float *raw_f32;
  size_t part_off;           // doubles: [nblk][npoints] partial sums
  size_t out_off;            // doubles: [npoints] log marginal likelihood
  double *scores_out;        // draw: prior + likelihood, or null
  float *hp_dst;             // draw: the feature's device hp block (null: the CRP grid, index only)
  double *aux_dst;           // draw, dd / dm: FeatDesc::aux of the state's descriptor (null otherwise)
  uint64_t stream;           // draw: Philox counter (msc_hp_grid_gibbs)
};

// msc_hp_slice as k_hp_slice reads it (kernels_slice.hip): one target a workgroup -- a feature's chain of coordinates,
// entries [first, first + n) of the call's SliceCoord array in the caller's order, or the CRP concentration (family
// kHpCluster, one entry).  Per entry the kernel writes the installed value, the evaluations it took and a status
// (kSliceOk / kSliceNonFinite / kSliceStalled) at the entry's index; a feature's final block goes into hp.
constexpr uint32_t kSliceOk = 0, kSliceNonFinite = 1, kSliceStalled = 2;
struct SliceTarget {
  int32_t family;            // or kHpCluster
  uint32_t hpf;              // floats of the hp block (<= 4 for the families sliced)
  uint32_t nu32, nf32;       // raw table rows of the family
  const uint32_t *raw_u32;   // the feature's raw tables, rows of kpad
  const float *raw_f32;
  float *hp;                 // the feature's device hp block (null: alpha)
  float alpha;               // kHpCluster: alpha at the call
  uint32_t target;           // Philox counter word 0: the feature, or nfeatures for alpha
  uint32_t first, n;
};
struct SliceCoord {
  uint32_t coord, prior, partner;   // msc_slice_coord, as validated by msc_hp_slice
  float width, prior_a, prior_b;
};
// msc_chains_hp_slice: what is per chain of the ensemble's slice step (k_hp_slice_chains) and of the rebuild of the score
// and CRP tables that follows it (k_chains_prepare, kernels_score.hip)
struct HpChain {
  const FeatDesc *feats;     // the chain's state: descriptors, group counts, CRP terms
  const uint32_t *cnt;
  const uint8_t *slots;      // the chain's mask of counted slots or null (the non-empty ones)
  float *crp;
  uint64_t key;              // the chain's Philox key of the slice step (seed ^ kSliceKey)
  float alpha;               // alpha at the call; k_hp_slice_chains leaves the installed one here for the rebuild
  uint32_t pad;
};
// msc_score_joint / msc_chains_score_joint (kernels_joint.hip): the hyper-prior entries of a call travel as a kernel
// argument, kJointCoords of them a launch -- no table of them to upload, so the single-state call copies nothing at all.
// Entries past the first launch's are added, in entry order still, by follow-up launches of k_joint_priors.
constexpr uint32_t kJointCoords = 64;
struct JointCoord {
  uint32_t feature;          // the state feature, or MSC_HP_CLUSTER
  uint32_t coord, prior, partner;
  float prior_a, prior_b;
};
struct JointCoords {
  JointCoord e[kJointCoords];
};
// what is per chain of the ensemble's call: the chain's state, its mask and its row of the output
struct JointChain {
  const FeatDesc *feats;
  const uint32_t *cnt;
  const uint8_t *slots;      // the chain's mask of counted slots or null (the non-empty ones)
  double *out;               // the chain's row, nfeatures + 3 doubles
  float alpha;
  uint32_t pad;
};
// msc_theta_slice: one bbnc feature of the call (a row of workgroups, one lane a slot)
struct ThetaJob {
  const uint32_t *raw_u32;   // heads, tails
  float *raw_f32;            // p
  const float *hp;           // the feature's device hp {alpha, beta}
  float width;
  uint32_t feature;
};

// One drawn feature of msc_sample_predictive as the kernels of kernels_pred.hip read it: where its hp and raw tables are,
// the predictive parameters k_pred_prepare writes (par: [K][stride] doubles, pred_par_stride), and the columns a draw
// reads (the bound view's column in the model's value type, its mask) and writes (out: nrows x count values).
struct PredFeat {
  int32_t family;
  uint32_t dim;
  uint32_t feature;          // the state's feature index (the draw's Philox counter)
  uint32_t stride;           // doubles of par per group
  double *par;
  const float *hp;
  const uint32_t *raw_u32;
  const float *raw_f32;
  const double *niw_w64;     // niw: k_niw_prepare's whitening matrices
  const void *col;
  const uint8_t *mask;
  void *out;
};
// bb / bbnc {P(v = 0)}, gp {shape, scale}, bnb {alpha', beta', r}, dd {cumulative weights[dim]}, nich {mu', scale, nu'},
// niw {mu'[d], L[d (d + 1) / 2], dof}
inline uint32_t pred_par_stride(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB:
    case MSC_BBNC: return 1;
    case MSC_GP: return 2;
    case MSC_BNB:
    case MSC_NICH: return 3;
    case MSC_DD: return dim;
    case MSC_NIW: return dim + dim * (dim + 1) / 2 + 1;
    default: return 0;
  }
}

// One feature of the blocked Gibbs sampler as the kernels of kernels_blocked.hip read it (msc_blocked_*): where the draw
// finds hp and the slot's suff-stats, where its slices sit in the state's parameter table (row 0 of the table holds the
// log weights; blocked_post.hpp lists the slices), and the bound column the assign kernels score.
enum BlkKind : uint32_t { MSC_BLK_NOOP = 0, MSC_BLK_SELECT = 1, MSC_BLK_LINEAR = 2, MSC_BLK_GATHER = 3, MSC_BLK_NICH = 4 };
struct BlkFeat {
  uint32_t kind;             // BlkKind: how a value meets the slices
  uint32_t slice0;           // first table row of the feature's slices
  uint32_t nslices;
  int32_t family;
  uint32_t dim;
  uint32_t tag;              // the feature's index: the Philox stream of its draws
  const void *col;           // bound column in the model's value type (null until a view is bound)
  const uint8_t *mask;
  const float *hp;
  const uint32_t *raw_u32;
  const float *raw_f32;
};
inline uint32_t blocked_slices(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB:
    case MSC_GP:
    case MSC_BNB: return 2;
    case MSC_NICH: return 3;
    case MSC_DD: return dim;
    case MSC_NIW: return 1;     // (c; the matrices are BlockedWork's doubles, blocked_niw.hpp)
    default: return 0;
  }
}

// One start of msc_zmatrix_partition_refine (kernels_refine.hip): its running totals over the sweeps
struct RefineStart {
  int64_t dec;        // binder_num of the start less binder_num now
  uint64_t moves;
  uint32_t sweeps;
  uint32_t active;    // the last sweep moved a row (or none has run): the next one has work
};

// One split-merge proposal as the kernels of kernels_splitmerge.hip hand it on (msc_split_merge): written by
// k_sm_anchors, `accepted` by k_sm_decide.  A void proposal (an unassigned anchor, no empty slot for a split, fewer than
// two rows) makes every later kernel of the proposal a no-op.
struct SmProp {
  int32_t gi, gj;            // the anchors' groups
  uint32_t kind;             // sm::kSplit / kMerge / kVoid (splitmerge_math.hpp)
  int32_t target;            // where the label-1 rows go when accepted: a split's lowest empty slot, a merge's gi
  uint64_t i, j;             // the anchors, as offsets from the call's first row
  uint32_t accepted;
  uint32_t pad;
};

inline uint32_t tab_rows(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB: return 2;
    case MSC_BBNC: return 2;
    case MSC_GP: return 2 + kGpMaxTable;   // GP_T0 + table rows (family_math.hpp)
    case MSC_BNB: return 2 + kGpMaxTable;
    case MSC_DM: return 0;                  // sized when a column is bound (sum of the stages' tables)
    case MSC_DD: return dim;
    case MSC_NICH: return 6; // NICH_ROWS
    case MSC_NIW: return 8;  // NIW_ROWS + 1 (kernels_niw.hip)
    default: return 0;
  }
}
inline uint32_t loo_rows(int family) { return family == MSC_NICH ? kNlooStride : 0u; }
// (+ 1: the zero row a masked value selects, FeatDesc::col_sentinel)
inline uint32_t loo_tab_rows(int family, uint32_t dim) {
  return family == MSC_BB ? 3u : (family == MSC_GP || family == MSC_BNB) ? kGpMaxTable + 1u : family == MSC_DD ? dim + 1u : 0u;
}
inline uint32_t raw_u32_rows(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB: return 2;
    case MSC_BBNC: return 2;
    case MSC_GP: return 2;
    case MSC_BNB: return 2;
    case MSC_DM: return dim;
    case MSC_DD: return 1 + dim;
    case MSC_NICH: return 1;
    case MSC_NIW: return 1;
    default: return 0;
  }
}
// float raw rows with stride kpad (niw's vector fields are handled separately)
inline uint32_t raw_f32_rows(int family) {
  switch (family) {
    case MSC_GP: return 1;
    case MSC_BBNC: return 1;   // p
    case MSC_DM: return 1;     // ratio
    case MSC_NICH: return 2;
    default: return 0;
  }
}
inline uint32_t acc_i64_rows(int family, uint32_t dim) {
  switch (family) {
    case MSC_BB: return 2;
    case MSC_BBNC: return 2;
    case MSC_GP: return 2;
    case MSC_BNB: return 2;
    case MSC_DM: return dim;
    case MSC_DD: return dim;
    case MSC_NICH: return 1;
    case MSC_NIW: return 1;
    default: return 0;
  }
}
inline uint32_t acc_f64_rows(int family) {
  switch (family) {
    case MSC_GP: return 1;
    case MSC_DM: return 1;
    case MSC_NICH: return 2;
    default: return 0;
  }
}
inline int value_type_of(int family) {
  switch (family) {
    case MSC_BB: return MSC_TYPE_B;
    case MSC_BBNC: return MSC_TYPE_B;
    case MSC_GP: return MSC_TYPE_U32;
    case MSC_BNB: return MSC_TYPE_U32;
    case MSC_DM: return MSC_TYPE_I32;
    case MSC_DD: return MSC_TYPE_I32;
    case MSC_NICH: return MSC_TYPE_F32;
    case MSC_NIW: return MSC_TYPE_F32;
    default: return MSC_TYPE_B;
  }
}
size_t primitive_size(int t);

// rows of a niw feature's float table (k_niw_prepare fills them) and the padded width of its W matrices
enum { NIW_C0 = 0, NIW_C1 = 1, NIW_A_LOO = 2, NIW_B_LOO = 3, NIW_C_LOO = 4, NIW_LOGDET_HI = 5, NIW_LOGDET_LO = 6,
       NIW_ROWS = 7 };   // row NIW_ROWS holds the prior's ln det Psi (hi, lo) in its first two slots
constexpr int kNiwPad = 32;                 // the f32 kernel's padded matrix width (dim <= 32)
constexpr unsigned kMaxNiwDim = 128;        // what the prepare kernel's packed LDS triangles hold (2 x 66 KB)

// The f64 contraction works on 16-blocks: component block b (rows 16b .. 16b+15 of the lower-triangular W) meets
// feature blocks s4 = 0 .. b only.  A chunk = one (b, s4) pair = four MFMA steps; step e of the chunk contracts
// features 16 s4 + 4 e + kk (kk = lane / 16).  Per group the chunks are stored in the order the kernel walks them,
// 64 lanes x 4 doubles each, so a chunk is one coalesced 2 KiB read per wave.
__host__ __device__ inline uint32_t niw_blocks(uint32_t d) { return (d + 15u) / 16u; }
__host__ __device__ inline uint32_t niw_chunks(uint32_t d) { return niw_blocks(d) * (niw_blocks(d) + 1u) / 2u; }
__host__ __device__ inline size_t niw_w_stream(uint32_t d) { return (size_t)niw_chunks(d) * 256u; }   // doubles per group
__host__ __device__ inline size_t niw_b_stream(uint32_t d) { return (size_t)niw_blocks(d) * 256u; }
// where W[i][j] (j <= i) sits in a group's stream: lane (c = i % 16, kk = j % 4), slot e = (j % 16) / 4 of chunk (i / 16, j / 16)
__host__ __device__ inline size_t niw_w_index(uint32_t i, uint32_t j) {
  const uint32_t b = i >> 4, s4 = j >> 4;
  return (size_t)(b * (b + 1u) / 2u + s4) * 256u + (size_t)((i & 15u) + 16u * (j & 3u)) * 4u + ((j & 15u) >> 2);
}
// where (W mu)[i] sits: accumulator register r = (i % 16) / 4 of the lanes with kk = i % 4 (every c holds the same value;
// this is the c = 0 copy)
__host__ __device__ inline size_t niw_b_index(uint32_t i) {
  return (size_t)(i >> 4) * 256u + (size_t)(16u * (i & 3u)) * 4u + ((i & 15u) >> 2);
}

}  // namespace msc

// ---- workspaces of the opaque objects that one unit owns: the context's ----------------------------------------------
namespace msc {
// The workspaces a context keeps between calls for the posterior summaries of summary.cpp, each used by one entry point.
// msc_linkage_single: the chain's edges, 3 (n - 1) doubles
struct LinkageWork {
  DevBuf<double> edges;
};
// msc_partition_distances: the ids and cluster counts of a chunk of a and a chunk of b, log2 n for n <= log2_n, and the
// contingency tables of the pairs that do not fit LDS (zeroed once; the kernel leaves them zero)
struct PdWork {
  DevBuf<uint16_t> ids;
  DevBuf<uint32_t> k;
  DevBuf<double> log2;
  uint32_t log2_n = 0;
  DevBuf<uint32_t> table;
};
// msc_partition_refine_vi (kernels_refine_vi.hip), allocated at first use: the samples' ids [S][ldi], their cluster
// counts and running sums, the stretch indices [m][S], G of msc_vi_table for m = G_m rows (0: none; the host copy is
// what the upload reads), the visiting order, and a chunk of starts' ids, totals and contingency cells
struct ViWork {
  DevBuf<uint16_t> sample_ids;
  DevBuf<uint32_t> L, off, row;
  DevBuf<int64_t> G;
  std::vector<int64_t> G_host;
  uint32_t G_m = 0;
  DevBuf<uint32_t> order;
  DevBuf<uint16_t> ids;
  DevBuf<RefineStart> st;
  DevBuf<uint16_t> cells;
};
}  // namespace msc

// ---- opaque objects ---------------------------------------------------------
struct msc_context {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 256;
  // k_score_nich1 launch shape (index into kNich1Shapes) per output buffer: which shape suits the write stream
  // depends on where the buffer lies (abi.cpp run_score); most recent first, at most 16 buffers remembered
  struct ShapeEntry { const void *out; uint64_t nrows; uint32_t K; int shape; int plain_stores; };   // plain_stores: -1 = not timed
  std::vector<ShapeEntry> nich1_shapes;
  // buffers this context placed (msc_device_alloc >= 64 MiB, msc_device_alloc_probed) and how their probe went: a buffer
  // that took the probe's NON-TEMPORAL fill at kNtFastGbps or better takes the single-nich pass's non-temporal stores at
  // 0.85-0.88 of the HBM roof; every other buffer (the probe's lower bands, a caller's own) is written with plain stores --
  // 0.78-0.83 whatever the placement, where non-temporal ones run 0.69-0.76 (profiles/r04_store_policy.txt)
  struct Placed { const void *base; size_t size; bool nt_fast; };
  std::vector<Placed> placed;
  // a stream of the library's own on which sweep steps are recorded (the caller's may be the null stream, which
  // cannot capture); nothing ever executes on it
  hipStream_t record_stream = nullptr;
  // buffers msc_device_alloc_probed mapped from separately created physical chunks (hipMemCreate + hipMemMap); freed
  // through msc_device_free
  struct VmmAlloc { void *va; size_t size; std::vector<hipMemGenericAllocationHandle_t> handles; };
  std::vector<VmmAlloc> vmm;
  // the candidates of the most recent placed allocation (msc_device_alloc >= 64 MiB, msc_device_alloc_probed): fill
  // rates in GB/s and the index kept (msc_device_alloc_stats)
  std::vector<float> last_alloc_rates;
  uint32_t last_alloc_chosen = 0;
  // pinned, device-mapped mailbox for msc_value_op_single
  msc::MappedBuf<unsigned char> mailbox_host;
  void *mailbox_dev = nullptr;
  // msc_context_synchronize: a word of pinned memory the stream writes a sequence number into (hipStreamWriteValue32)
  // and the host watches, instead of sleeping in hipStreamSynchronize
  msc::MappedBuf<uint32_t> sync_word_host;
  void *sync_word_dev = nullptr;
  uint32_t sync_seq = 0;
  bool sync_word_ok = true;                // cleared when the stream operation is refused: plain stream waits from then on
  // the device's error word {code, detail} (device_error.hpp), pinned and shared by every context on the device
  volatile uint32_t *err_host = nullptr;
  msc::LinkageWork linkage;               // msc_linkage_single (summary.cpp)
  msc::PdWork pd;                         // msc_partition_distances (summary.cpp)
  msc::ViWork vi;                         // msc_partition_refine_vi (summary.cpp)
};

struct msc_dataview {
  msc_context *ctx = nullptr;
  uint64_t serial = 0;                   // unique per view: a state's binding is keyed on it, not on the address
  uint64_t nrows = 0;
  std::vector<msc_runtime_type> types;   // per feature, after conversion
  std::vector<void *> cols;              // device columns
  std::vector<void *> masks;             // device mask columns or null
  std::vector<msc::DevBuf<uint8_t>> owned;   // the columns and masks msc_dataview_from_records made
  mutable std::vector<long long> col_max;  // lazily computed maximum of uint32 columns (-1 = unknown)
  mutable std::vector<std::vector<uint32_t>> dm_max;  // dm columns: maxima of each category and of the row totals (lazy)
  // what the library derives from the columns and keeps with the view until it is destroyed or invalidated (abi.cpp
  // view_copy): one entry per (kind, key)
  enum CopyKind : uint32_t {
    kConverted,    // a column converted to another primitive type with runtime_cast semantics, made the first time a
                   // state binds it to a model whose value type differs (column_as); key {column, type}
    kSentinel,     // a masked lookup column with the mask folded in as a sentinel value (sentinel_column); key {column,
                   // element bytes, sentinel}
    kPackedBits,   // a byte column holding the bits of two to four bool columns, made when a state's plan fuses them
                   // (plan_groups, k_pack_bits); key: the member columns' device pointers, then the radix
    kNichX,        // float [nrows][n2p] of the columns in the key, position-major (msc::NichPos; nich_x_matrix)
    kLookIdx,      // uint32 [nrows][l4] lookup index matrix (msc::FeatDesc::lk_idx; look_idx_matrix); key: per feature
                   // {column, kind | clamp | slot offset, byte}
    kDmTot,        // a dm column's row totals (uint32 [nrows]; bind_dm_column); key {column}
    kDmMax,        // ... and the device scratch its maxima were found in; key {column}
  };
  struct Copy {
    CopyKind kind;
    std::vector<uint64_t> key;
    msc::DevBuf<uint8_t> buf;
  };
  mutable std::vector<Copy> copies;
};

struct msc_feature_host {
  int family = 0;
  uint32_t dim = 0;
  std::vector<float> hp;
  msc::DevBuf<float> hp_dev;
  msc::DevBuf<float> tab;             // dm: (re)sized when a column is bound (bind_dm_column)
  msc::DevBuf<uint32_t> raw_u32;
  msc::DevBuf<float> raw_f32;
  msc::DevBuf<double> loo64;          // nich: leave-one-out constants
  msc::DevBuf<float> loo_tab;         // bb, gp, bnb, dd: leave-one-out tables
  msc::DevBuf<float> niw_w, niw_b;
  msc::DevBuf<double> niw_w64, niw_mu64, niw_c64;
  size_t i64_off = 0, i64_len = 0;   // slices of the state's reduce buffers (elements)
  size_t f64_off = 0, f64_len = 0;
  msc::DevBuf<uint32_t> dm_meta_dev;  // dm: [dim+1][2] stage tables (FeatDesc::dm_meta)
  std::vector<uint32_t> dm_meta;     // host copy
};

struct msc_state;
// a grid of hyper-parameter points of one feature (or of alpha: feature == MSC_HP_CLUSTER), uploaded once
struct msc_hp_grid {
  msc_state *st = nullptr;
  uint32_t feature = 0;
  std::vector<float> blocks;          // [npoints][hpf], the host copy
  msc::DevBuf<float> grid_dev;
  msc::DevBuf<double> logprior_dev;   // null: no prior
  msc::HpJob job;                     // the grid alone (part_off = out_off = 0)
  msc::DevBuf<msc::HpJob> job_dev;
};

// ---- ... and the state's --------------------------------------------------------------------------------------------
namespace msc {
// grid hyper-parameter inference (hyper.cpp msc_hp_grid_*): the live grids (destroyed with the state at the latest) and
// the workspaces of the calls, grown on demand
struct HyperWork {
  std::vector<std::unique_ptr<msc_hp_grid>> grids;
  DevBuf<double> part;           // per (group block, point) partial sums
  DevBuf<double> out;            // msc_hp_grid_gibbs: every grid's likelihoods
  DevBuf<HpJob> jobs_dev;        // msc_hp_grid_gibbs: the grids of the call, then the indices drawn
  DevBuf<uint32_t> chosen_dev;
  std::vector<HpJob> jobs_host;
  // slice sampling (hyper.cpp msc_hp_slice / msc_theta_slice): the call's targets and entries, then its outputs; grown on
  // demand
  DevBuf<unsigned char> slice_buf;
};
// posterior predictive sampling (predict.cpp msc_sample_predictive): the drawn features' descriptors and parameters, and
// the scratch assignment of a group draw, grown on demand
struct PredWork {
  DevBuf<PredFeat> feats_dev;
  DevBuf<double> par;
  DevBuf<int32_t> z;
  std::vector<PredFeat> feats_host;   // what feats_dev holds
  StagedUpload upload;                // how feats_dev is written
};
// the blocked Gibbs sampler (blocked.cpp msc_blocked_*): the parameter table -- (1 + sum of the features' slices) rows of
// kpad floats, row 0 the log stick weights -- the features as the kernels read them, the stick kernel's scratch
// (log V, log(1 - V): 2 K doubles); whether the table was drawn from the tables as they stand: valid.draw_current().
// A state of one niw feature (BlockedKernel::niw1) also owns, from its first draw on, the drawn matrices in double:
// mean[K][dim], whiten[K][dim (dim + 1) / 2] (msc_blocked_niw_params) and the same V, V mu as the assign kernel's operand
// streams, [K][niw_w_stream(dim)] and [K][niw_b_stream(dim)]
struct BlockedWork {
  DevBuf<float> tab;
  DevBuf<BlkFeat> feats_dev;
  std::vector<BlkFeat> feats_host;
  DevBuf<double> work;
  uint32_t rows = 0;
  DevBuf<double> niw_mean, niw_whiten, niw_w64, niw_mu64;
};
// the split-merge move (blocked.cpp msc_split_merge): an internal three-slot state of the same features -- pair slots 0
// and 1, slot 2 their union -- created at the first call and destroyed with its state; the pair labels of the call's
// rows, the assign kernel's per-workgroup partials, the proposal descriptor and the pair state's score_data
struct SplitMergeWork {
  msc_state *pair = nullptr;
  DevBuf<int32_t> ell;
  DevBuf<double> part;
  DevBuf<SmProp> prop;
  DevBuf<float> sd;
};
}  // namespace msc

struct msc_state {
  msc_context *ctx = nullptr;
  uint32_t nfeat = 0, K = 0, kpad = 0;
  float alpha = 1.f;
  std::vector<msc_feature_host> feats;
  bool nich1 = false, has_dm = false;   // msc_state_create (no call changes the families): a single nich feature, any dm
  uint32_t n_niw = 0;                   // feature, how many niw features
  msc::DevBuf<long long> red_i64;   // [cnt[kpad] | feature slices]
  msc::DevBuf<double> red_f64;
  size_t n_i64 = 0, n_f64 = 0;
  msc::DevBuf<double> red_pack;   // both tables as one float64 buffer (msc_state_reduce_pack), made at the first call
  uint64_t sweep_rows_hint = 0;   // msc_state_set_sweep_rows: the rows of the WHOLE a sharded sweep's kernel choice goes by
  // msc_state_set_col_bounds: the WHOLE dataset's column maxima per feature (gp / bnb: one value; dm: each category's,
  // then the row total's; other families none) -- the plan goes by max(bound view's, these).  Empty: the view's alone.
  std::vector<std::vector<uint32_t>> col_bounds;
  bool rebind = false;            // the bounds changed: the next call binds its view afresh (and so re-plans)
  msc::DevBuf<uint32_t> cnt_u32;    // group sizes (group_manager counts), [kpad]
  msc::DevBuf<float> logpc;         // log pseudocount per group, [kpad] (+ loo variants, see prepare)
  msc::TableValidity valid;         // which of the tables above and below are current (table_validity.hpp)
  msc::DevBuf<msc::FeatDesc> desc_dev;
  std::vector<msc::FeatDesc> desc_host;
  // the same descriptors in the order the tile kernels walk them (tile_plan.hpp plan_phases): every feature but the
  // unmasked nich ones, in the caller's order, then the unmasked nich features (from index plan.tile_split on)
  msc::DevBuf<msc::FeatDesc> desc_tile_dev;
  std::vector<msc::FeatDesc> desc_tile_host;
  // the same plan with runs of unmasked bb / bbnc columns fused (FeatDesc::fuse_*): what the score / sweep kernels walk;
  // the leave-one-out pass keeps the plan above (its double sum over features stays term by term)
  msc::DevBuf<msc::FeatDesc> desc_fuse_dev;
  std::vector<msc::FeatDesc> desc_fuse_host;
  msc::DevBuf<float> fuse_tab;        // the fused tables, 32 rows of kpad floats a fused feature (16 or 27 used)
  // what msc_accumulate walks: the fused bb features first (each feeds its members' tables from one byte column), then
  // every feature no fused one covers, as the caller gave it (masks and all)
  msc::DevBuf<msc::FeatDesc> desc_acc_dev;
  std::vector<msc::FeatDesc> desc_acc_host;
  msc::DevBuf<msc::NichPlanInfo> nich_info;   // [nfeat]: per feature of the plans' second phase (FeatDesc::nich_info)
  msc::DevBuf<float> rn_pack;                 // the role-split kernels' second phase (msc::NichPos): (1 + 5 nfeat) x kpad floats
  msc::DevBuf<msc::NichPos> rn_pos;           // [nfeat rounded up to four]
  // what the planner found for the descriptors above (tile_plan.hpp writes it whole), and what the routes go by
  // (route.hpp): the plan and the per-feature facts as of the last bind or plan (abi.cpp upload_desc), view_rows as of
  // the call that routes
  msc::TilePlan plan;
  msc::RouteFacts route;
  const msc_dataview *bound_view = nullptr;
  uint64_t bound_serial = 0;
  std::vector<uint32_t> bound_cols;
  msc::Retired retired;           // buffers grow_retained replaced: a captured step graph may still read them
  msc::DevBuf<float> scratch;     // score chunk for the generic sweep path
  msc::DevBuf<float> tail_scores;   // 64 floats per row: the groups beyond the first tile (k_score_tail_rows -> k_sweep_tile_roles<true>)
  msc::DevBuf<float> own;         // per-row leave-one-out values (k_loo_own)
  msc::DevBuf<float> tail_pack;       // k_tail_pack's output: tail_pack_rows x 64 floats (grown on demand)
  msc::DevBuf<double> marg_norm;  // msc_score_marginal: {log(n + alpha), log(n - 1 + alpha)}, rewritten by every call
  msc::DevBuf<float> rows_table;  // k_sweep_nich1_rows: per-group constants as scalar operands (single nich, K > 1024)
  msc::DevBuf<uint32_t> colmax_dev;
  // (seed, sweep index) of the sampling kernels, device-resident (kernels_sweep.hip), and what the host believes it holds
  // (step_rules.hpp: the calls report events to the mirror; rng.mid_step() is also how a call learns that the state is
  // between msc_sweep_step_begin and msc_state_commit_reduce)
  msc::DevBuf<uint64_t> rng_dev;
  msc::RngMirror rng;
  // a whole sweep step (assign + accumulate + commit) captured as a graph for its steady state (abi.cpp msc_sweep_step;
  // step_rules.hpp step_action decides from key, seen and disabled; abi.cpp drop_step_graph is the one place that
  // destroys the executable)
  struct StepGraph {
    hipGraphExec_t exec = nullptr;
    msc::StepKey key;                       // what the executable was captured, or the eager steps are counted, under
    msc::TableValidity::Snapshot flags;     // validity flags of the state at the captured step's entry
    int seen = 0;                           // eager steps with this key so far
    bool disabled = false;                  // a capture failed: every later step runs eagerly
    uint64_t n_eager = 0, n_replayed = 0;   // steps run either way (msc_sweep_step_stats)
  } step_graph;
  msc::DevBuf<double> niw_qown;      // q of every row's own group (niw leave-one-out), one a row
  msc::DevBuf<int32_t> one_z;        // a one-entry assignment vector (msc_entity_op's general path)
  msc::DevBuf<uint32_t> niw_scratch;   // row bucketing for niw accumulate: 2 K + 1 + rows uint32
  msc::HyperWork hp;                  // msc_hp_grid_*, msc_hp_slice, msc_theta_slice (hyper.cpp)
  msc::PredWork pred;                 // msc_sample_predictive (predict.cpp)
  msc::BlockedWork blk;               // msc_blocked_*, msc_sweep_blocked (blocked.cpp)
  msc::SplitMergeWork sm;             // msc_split_merge (blocked.cpp)
  uint32_t chain_members = 0;                   // live msc_chains handles that hold this state: it cannot be destroyed meanwhile
};

// a z-matrix accumulator (summary.cpp msc_zmatrix_*, kernels_query.hip): m selected rows, counts as upper-triangle tiles
struct msc_zmatrix {
  msc_context *ctx = nullptr;
  uint64_t n = 0;
  uint32_t m = 0, nlabels = 0, nt = 0;     // nt: 64-row bands (m rounded up)
  bool wide = false;                       // 16-bit labels (nlabels > 256)
  msc::DevBuf<uint32_t> rows_dev;          // [m]
  msc::DevBuf<uint32_t> order_dev;         // [m], the order of the most recent counts / result call
  msc::DevBuf<uint32_t> batch;             // [64 nt][kZmBatchWords], zero where no sample is staged
  msc::DevBuf<uint32_t> bad;               // [kZmBatchMax + 1]: bad-sample flags of the batch's slots, then their number
  msc::DevBuf<uint32_t> counts;            // [nt (nt + 1) / 2][64][64]
  uint32_t staged = 0;                     // samples in the batch
  uint64_t nsamples = 0;
  // msc_zmatrix_partition_* (kernels_partition.hip), allocated at the first call: a chunk of gathered candidate labels
  // [chunk][64 nt], the chunk's sums for the loss ([chunk][m] w, then [chunk][m] size), and T
  msc::DevBuf<int32_t> part_lab;
  msc::DevBuf<uint64_t> part_w;
  msc::DevBuf<uint32_t> part_size;
  msc::DevBuf<uint64_t> part_T;
  // msc_zmatrix_partition_refine (kernels_refine.hip), allocated at the first call: the dense [m][m rounded up to 4] copy
  // of the counts, and of one chunk of starts the 16-bit ids [chunk][m rounded up to 4], the running totals and the
  // starts' own binder_num
  msc::DevBuf<uint32_t> ref_dense;
  msc::DevBuf<uint16_t> ref_ids;
  msc::DevBuf<msc::RefineStart> ref_st;
  msc::DevBuf<int64_t> ref_binder;
};
