/*
 * microscopes_hip.h -- C ABI of the MI355X (gfx950) implementation of the
 * component-model scoring hot path of datamicroscopes/common.
 *
 * The reference has no FFI for this path: downstream C++ drives the virtual
 * microscopes::models::group API one value at a time
 * (include/microscopes/models/base.hpp:21-37) and Cython only wraps object
 * lifetimes (microscopes/_models.pyx:16-52).  This header is the boundary a
 * maintainer binds instead (cgo-free: plain C, pointers and sizes only, no torch
 * or C++ types); include/microscopes/ holds the C++ plugin surface that sits on
 * top of it and INTEGRATION.md shows the binding stubs.  Each entry point names
 * the reference interface it replaces.
 *
 * Conventions
 *   - every function returns MSC_OK (0) or a negative msc_status; the message of
 *     the last failure on the calling thread is msc_last_error().  Nothing throws
 *     across this boundary (reference convention: C++ exceptions,
 *     distributions.hpp:140,152,178,198 -- the C++ layer above re-throws).
 *   - "dev" pointers are device (HBM) addresses valid on the context's device;
 *     "host" pointers are ordinary host memory.  Work is enqueued on the
 *     context's HIP stream and is asynchronous unless stated otherwise.
 *   - there is no CPU fallback: without a usable gfx950 device context creation
 *     fails and nothing else can be called.
 */
#ifndef MICROSCOPES_HIP_H
#define MICROSCOPES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSC_ABI_VERSION 1

typedef enum msc_status {
  MSC_OK = 0,
  MSC_EINVAL = -1,       /* bad argument (shape, family, null pointer, ...) */
  MSC_EHIP = -2,         /* HIP runtime error (message carries hipGetErrorString) */
  MSC_ENODEVICE = -3,    /* no gfx950 device / extension not usable */
  MSC_EUNSUPPORTED = -4, /* valid request outside what is built (e.g. dd dim > 128) */
  MSC_ENOMEM = -5,
  MSC_EDEVICE = -6       /* a kernel of an EARLIER call on this device reported that something it relies on did not hold
                            (an entity leaving a group it is not in, a relation offset past the score row, a wave barrier
                            that timed out); noticed at the synchronising and launching calls, reported once; the tables of
                            the state that call touched are to be rebuilt (msc_accumulate with MSC_ACC_RESET) */
} msc_status;

/* likelihood families; one kernel family each (distributions.hpp:58-64) */
typedef enum msc_family {
  MSC_BB = 0,   /* BetaBernoulli            value bool   (uint8)          */
  MSC_GP = 1,   /* GammaPoisson             value uint32                  */
  MSC_DD = 2,   /* DirichletDiscrete<128>   value int32 in [0, dim)       */
  MSC_NICH = 3, /* NormalInverseChiSq       value float                   */
  MSC_NIW = 4,  /* NormalInverseWishart<-1> value float[dim]              */
  MSC_NOOP = 5, /* noop model, models/noop.hpp:13-53 (API-overhead control) */
  MSC_BBNC = 6, /* non-conjugate Beta-Bernoulli with explicit p (src/models/bbnc.cpp:22-73), value bool */
  MSC_BNB = 7,  /* BetaNegativeBinomial (distributions.hpp:29-36,59-64), hp {alpha, beta, r}, value uint32 */
  MSC_DM = 8    /* Dirichlet-Multinomial (src/models/dm.cpp:10-97), hp alphas[dim], value int32[dim] */
} msc_family;

/* primitive types, include/microscopes/common/type_info.h:10-44 (same order) */
typedef enum msc_primitive_type {
  MSC_TYPE_B = 0, MSC_TYPE_I8, MSC_TYPE_U8, MSC_TYPE_I16, MSC_TYPE_U16, MSC_TYPE_I32,
  MSC_TYPE_U32, MSC_TYPE_I64, MSC_TYPE_U64, MSC_TYPE_F32, MSC_TYPE_F64, MSC_TYPE_NELEMS
} msc_primitive_type;

/* runtime_type{t, n, vec} (runtime_type.hpp:65-141); count == n() */
typedef struct msc_runtime_type {
  int32_t type;   /* msc_primitive_type */
  uint32_t count; /* elements per value: 1 for scalars, n for vector fields */
} msc_runtime_type;

typedef struct msc_feature_spec {
  int32_t family; /* msc_family */
  uint32_t dim;   /* dd: number of categories (<=128); niw: dimension (<=128); dm: categories (<=128); else 0 */
} msc_feature_spec;

typedef struct msc_context msc_context;
typedef struct msc_dataview msc_dataview;
typedef struct msc_state msc_state;

/* ---- library / context ------------------------------------------------- */
int msc_abi_version(void);
const char *msc_last_error(void);
const char *msc_build_info(void); /* "gfx950 hipcc <ver> ..." */
/*
 * Which kernel INSTANTIATION the library chose for this process's most recent scoring pass (which = 0: msc_score_value)
 * or fused assignment pass (which = 1: msc_sweep_assign / msc_sweep_step), or the most recent kernel of the z-matrix
 * accumulator, of its linkage or of the partition distances (which = 2: msc_zmatrix_*, msc_linkage_single,
 * msc_partition_distances' pair kernel), or the kernel that reduced the rows of the most recent row predictive pass
 * (which = 3: msc_score_marginal), spelled as rocprofv3 spells it, e.g.
 * "k_score_tile_roles<false, false, false>" ("" before the first such call).  Measurement tooling only: bench.py keys the
 * committed counter summaries (profiles/ *_pmc.json) by it, so that a roofline figure is always the figure of the kernel
 * that ran.  Nothing comparable upstream (the reference has no kernels).
 */
const char *msc_last_kernel(int which);

/* stream: a hipStream_t (may be NULL = the device's null stream). */
int msc_context_create(int device, void *stream, msc_context **out);
int msc_context_destroy(msc_context *ctx);
int msc_context_set_stream(msc_context *ctx, void *stream);
int msc_context_synchronize(msc_context *ctx);

/*
 * Device buffers (zero-filled), for hosts that keep no HIP headers of their own: the assignment vector z, a row of
 * scores, the [N, K] score matrix.  upload / download are ordered on the context's stream and complete before they
 * return.
 *
 * From 64 MiB on a buffer is PLACED for the write stream of a score matrix: the same 1 GB stream takes 5.5 TB/s into
 * most allocations and 7.0 TB/s into some, decided by where the driver put the pages (profiles/r02_placement_study.txt),
 * and no allocator argument selects that.  A candidate is mapped from 32 MiB physical chunks through the virtual-memory
 * API (such buffers land in the upper band more often than hipMalloc'ed ones), stream-filled a few times on the
 * context's stream, and kept when it takes the stream at 6.65 TB/s or better; otherwise the next candidate is tried, up
 * to 12, and the fastest is kept.  The search also ends when the candidates held side by side would exceed half of what
 * the device had free at the call, and after six candidates whose rates lie within 6 % of each other (a box without a
 * fast stretch: nothing to find).  SYNCHRONOUS, about 1 ms per candidate and GB; MSC_ALLOC_CANDIDATES /
 * MSC_ALLOC_ACCEPT_GBPS in the environment change the bounds, MSC_ALLOC_CANDIDATES=0 is plain hipMalloc.
 * What the probe finds also decides how the single-nich scoring pass WRITES such a buffer: non-temporal stores into a
 * buffer that took the probe at 6.65 TB/s or better (the pass then runs at 0.85-0.88 of the HBM roof), plain stores into
 * every other buffer -- a placed one from the probe's lower bands, or one the caller brought -- where they run 0.78-0.83
 * whatever the placement and non-temporal ones 0.69-0.76 (profiles/r04_store_policy.txt; msc_score_tune times both for
 * a given buffer).
 * msc_device_alloc_probed is the same with the bounds given by the caller: all `candidates` are probed and the fastest
 * is returned; rates_gbps (nullable, `candidates` floats) receives every candidate's fill rate, *chosen (nullable) the
 * index kept.  msc_device_alloc_stats reports the same for the context's most recent placed allocation.
 * Free with msc_device_free.
 */
int msc_device_alloc(msc_context *ctx, size_t nbytes, void **out_dev);
int msc_device_alloc_probed(msc_context *ctx, size_t nbytes, uint32_t candidates, void **out_dev,
                            float *rates_gbps, uint32_t *chosen);
int msc_device_alloc_stats(msc_context *ctx, float *rates_gbps, uint32_t capacity, uint32_t *ntried, uint32_t *chosen);
int msc_device_free(msc_context *ctx, void *dev);
/*
 * Pinned host memory the device writes straight into (zero-copy): a row of scores the host reads after
 * msc_context_synchronize, with no copy in between -- what a per-entity caller wants for its one row of K floats.
 * *host is the CPU address, *dev the address to hand to the kernels (msc_score_value's out_dev).
 */
int msc_pinned_alloc(msc_context *ctx, size_t nbytes, void **host, void **dev);
int msc_pinned_free(msc_context *ctx, void *host);
int msc_device_upload(msc_context *ctx, void *dst_dev, const void *src_host, size_t nbytes);
int msc_device_download(msc_context *ctx, void *dst_host, const void *src_dev, size_t nbytes);

/* ---- columnar dataview (replaces recarray/dataview.hpp:194-217) -------- */
/*
 * Packed row-major records exactly as numpy_dataview hands them over
 * (microscopes/common/recarray/_dataview.pyx:61-92): n records of
 * sum(size(types[i])) bytes, no padding, optional mask with one bool per
 * element (runtime_type.hpp:123-134).  The records are copied to the device
 * once and transposed there into one contiguous column per feature, converted
 * with runtime_cast::cast semantics (runtime_type.hpp:145-166) to col_types[i]
 * (NULL: keep each feature's own primitive type).  Synchronous w.r.t. the host
 * buffers: they may be freed on return.
 */
int msc_dataview_from_records(msc_context *ctx, const void *host_records, const uint8_t *host_mask,
                              uint64_t nrows, const msc_runtime_type *types, uint32_t ntypes,
                              const int32_t *col_types, msc_dataview **out);
/*
 * Adopt columns that already live in HBM (generated on the device, or a torch
 * tensor): dev_columns[i] has nrows * types[i].count elements of types[i].type,
 * row-major for vector features, aligned to the element size (MSC_EINVAL otherwise).  dev_masks may be NULL or hold NULL entries;
 * a non-NULL entry has nrows * count bytes (nonzero = masked).  Borrowed, not
 * owned: the caller keeps them alive for the life of the view.
 */
int msc_dataview_from_device_columns(msc_context *ctx, uint64_t nrows,
                                     const msc_runtime_type *types, uint32_t ntypes,
                                     void *const *dev_columns, void *const *dev_masks,
                                     msc_dataview **out);
int msc_dataview_destroy(msc_dataview *view);
/*
 * What the library derives from a view's columns and keeps with the view (a column converted to a model's value type,
 * a masked column with the mask folded in, bool columns packed four to a byte, the maxima that size the exact count
 * tables) is a snapshot of the columns' CONTENTS.  After rewriting columns adopted by msc_dataview_from_device_columns
 * in place (minibatches through fixed buffers), call this: every derived copy is dropped and every state binds and
 * derives afresh at its next call.  Synchronises the context's stream.  (A view made from records owns its columns:
 * nothing can rewrite them.)
 */
int msc_dataview_invalidate(msc_dataview *view);
int msc_dataview_size(const msc_dataview *view, uint64_t *nrows, uint32_t *nfeatures);
int msc_dataview_column(const msc_dataview *view, uint32_t feature, void **dev_ptr,
                        msc_runtime_type *type);

/* ---- group tables: hypers + K groups of suff-stats per feature --------- */
/*
 * One state = the (hypers[f], groups[f][gid]) tables a mixture state object
 * keeps (entity_state.hpp:25-90): nfeatures component models, ngroups group
 * slots each, plus the CRP bookkeeping of group_manager (group_manager.hpp:
 * 218-283: per-group entity counts and alpha).  Group ids are the dense slot
 * numbers 0..ngroups-1.
 */
int msc_state_create(msc_context *ctx, const msc_feature_spec *features, uint32_t nfeatures,
                     uint32_t ngroups, msc_state **out);
/* MSC_EINVAL, and the state lives on, while it is a member of an msc_chains handle (destroy the handle first) */
int msc_state_destroy(msc_state *st);
int msc_state_shape(const msc_state *st, uint32_t *nfeatures, uint32_t *ngroups);

/*
 * hypers::set_hp / get_hp / get_hp_mutator (base.hpp:44-47) as flat float
 * blocks, field order as the reference names them (distributions.hpp:21-56):
 *   bb {alpha, beta}  bbnc {alpha, beta}  gp {alpha, inv_beta}  dd {alphas[dim]}
 *   nich {mu, kappa, sigmasq, nu}  niw {kappa, nu, mu[dim], psi[dim*dim]}
 *   bnb {alpha, beta, r (integral, carried as a float)}  dm {alphas[dim]} (dm.hpp:168)
 */
size_t msc_hp_floats(int family, uint32_t dim);
int msc_state_set_hp(msc_state *st, uint32_t feature, const float *host_hp, size_t nfloats);
int msc_state_get_hp(const msc_state *st, uint32_t feature, float *host_hp, size_t nfloats);

/*
 * group::set_ss / get_ss / get_ss_mutator (base.hpp:31-34) as packed host
 * records, one per group, float fields in float exactly as the reference keeps
 * them (distributions.hpp:21-56,79-91):
 *   bb   {u32 heads, u32 tails}
 *   bbnc {u32 heads, u32 tails, f32 p}       (p is state, not a count: accumulate leaves it alone)
 *   gp   {u32 count, u32 sum, f32 log_prod}
 *   dd   {u32 count_sum, u32 counts[dim]}
 *   nich {u32 count, f32 mean, f32 count_times_variance}
 *   niw  {u32 count, f32 sum_x[dim], f32 sum_xxT[dim*dim]}
 *   bnb  {u32 count, u32 sum}                (distributions.hpp:34-36)
 *   dm   {u32 counts[dim], f32 ratio}        (include/microscopes/models/dm.hpp:86-88)
 * Synchronous.
 */
size_t msc_ss_bytes(int family, uint32_t dim);
int msc_state_set_ss(msc_state *st, uint32_t feature, uint32_t first_group, uint32_t ngroups,
                     const void *host_records, size_t nbytes);
int msc_state_get_ss(msc_state *st, uint32_t feature, uint32_t first_group, uint32_t ngroups,
                     void *host_records, size_t nbytes);

/* group_manager: alpha (get_hp_mutator("alpha"), group_manager.hpp:124-130) and counts */
int msc_state_set_alpha(msc_state *st, float alpha);
/* the CRP concentration the state holds (msc_state_set_alpha, or what a hyper-parameter move installed) */
int msc_state_get_alpha(const msc_state *st, float *alpha);
int msc_state_set_group_counts(msc_state *st, const uint32_t *host_counts, uint32_t ngroups);
int msc_state_get_group_counts(msc_state *st, uint32_t *host_counts, uint32_t ngroups);

/* ---- the hot path ------------------------------------------------------ */
#define MSC_SCORE_CRP_PRIOR 0x1u /* add log(pseudocount(gid)), group_manager.hpp:274-283 */
#define MSC_SCORE_NIW_F32 0x2u   /* niw (dim <= 32) Mahalanobis on the f32 matrix pipe: 2x the rate, ~1e-5 instead of 1e-6;
                                    ignored for wider features */

/*
 * score_value for nrows rows x all groups x all features of the state:
 *   out[(r) * ld_out + k] = sum_f groups[f][k].score_value(hypers[f], row(row0+r)[cols[f]])
 * i.e. the K x D inner loop of entity_based_state_object::inplace_score_value
 * (entity_state.hpp:69-72) for a block of rows at once.
 * cols[f] = dataview column feeding state feature f (NULL: identity).
 * z_dev (nullable, int32[nrows] indexed from row0): leave-one-out -- row r is
 * scored against group z[r] with itself removed (remove_value before
 * score_value); z < 0 means unassigned, and so does an id >= ngroups
 * (no entry point indexes a table with an id it has not range-checked).
 * out_dev: float[nrows * ld_out], ld_out >= ngroups.  Any ld_out and alignment work; the kernels store 16 bytes a lane
 * when out_dev is 16-byte aligned and ld_out a multiple of 4 (8 bytes a lane when both are even), and a row that is whole
 * 64-byte lines -- ld_out a multiple of 16 -- is written at up to 1.7x the rate of one that is not (8 bb columns, 1M rows:
 * ld_out = 348: 0.46 ms, 352: 0.28; neighbouring rows share a line then, written by different waves at different times).
 */
int msc_score_value(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                    uint64_t nrows, const int32_t *z_dev, uint32_t flags, float *out_dev,
                    uint64_t ld_out);

/*
 * Optional and SYNCHRONOUS (about 10 ms): settle the launch shape of the single-NICH scoring pass (the HBM-write-bound
 * kernel of config C2 / C5) for passes of nrows rows into out_dev -- eight shapes, seven launches each into the
 * caller's own buffer (every run writes the same scores).  The winner is remembered in the context for (out_dev,
 * nrows, ngroups) and, as the fallback, for (nrows, ngroups); msc_score_value itself never times anything and never
 * waits.  *shape_out (nullable) = index of the chosen shape or -1 when the state does not take that kernel,
 * *ms_out (nullable) = its time per pass.  Not on a capturing stream.
 */
int msc_score_tune(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                   uint64_t nrows, float *out_dev, uint64_t ld_out, int *shape_out, float *ms_out);

#define MSC_ACC_RESET 0x1u    /* zero the tables first (then: suff-stats := f(z)) */
#define MSC_ACC_SUBTRACT 0x2u /* remove_value instead of add_value */
#define MSC_ACC_NO_COMMIT 0x4u /* leave the sums in the reduce buffer (all-reduce follows) */

/*
 * Bulk add_value / remove_value (base.hpp:25-26 + group_manager.hpp:218-248):
 * every row r in [row0, row0+nrows) with z[r] >= 0 is added to (removed from)
 * group z[r] of every feature, and the group counts follow.  Integer fields are
 * exact; float fields are accumulated in double in additive form and converted
 * to the reference's fields on commit.
 */
int msc_accumulate(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                   uint64_t nrows, const int32_t *z_dev, uint32_t flags);

/*
 * ONE entity joins (sign > 0) or leaves (sign < 0) ONE group, the group passed by value: group_manager::add_value /
 * remove_value together with every component model's add_value / remove_value for that row (the per-entity calls of
 * entity_based_state_object, entity_state.hpp:57-68).  For states of scalar families this is a single launch that
 * leaves every table current (sums, the reference's fields, score constants and CRP terms of the one group that
 * changed), so a Gibbs move -- leave, msc_score_value of the row, join -- is three launches and one copy back;
 * niw / dm features take the general accumulate path.  z_dev (nullable): the caller's device assignment vector, of
 * which entry `row` is set to the group (join) or -1 (leave).  Asynchronous.
 * Preconditions the device checks (the reference asserts them, group_manager.hpp:218-248): a leave needs a non-empty
 * group -- and, with z_dev, z_dev[row] == group --, a join with z_dev needs z_dev[row] unassigned.  A violation skips the
 * update it concerns and surfaces as MSC_EDEVICE at the next synchronising or launching call.  MSC_EINVAL between
 * msc_sweep_step_begin and msc_state_commit_reduce (the additive tables hold one rank's uncommitted sums then).
 */
int msc_entity_op(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row, uint32_t group,
                  int sign, int32_t *z_dev);

/* score_data (base.hpp:28) for every (feature, group): out_dev[f * ngroups + k] */
int msc_score_data(msc_state *st, float *out_dev);

/*
 * One synchronous Gibbs assignment sweep over rows [row0, row0+nrows)
 * (SURVEY 3.2 as a data-parallel schedule): every row is scored leave-one-out
 * against the tables as they stand, plus the CRP term, and re-drawn with
 * util::sample_discrete_log (util.hpp:125-156) using the counter-based uniform
 * Philox4x32-10(key = seed, counter = (global row id, sweep)).  row_id0 is the
 * global id of row0 (rank offset when rows are sharded).  z_dev is updated in
 * place; tables are NOT updated (call msc_accumulate with MSC_ACC_RESET next,
 * then all-reduce).
 */
int msc_sweep_assign(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                     uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed,
                     uint64_t sweep);

/*
 * One whole single-process sweep step: msc_sweep_assign, then
 * msc_accumulate(MSC_ACC_RESET) of the same rows with the new assignment
 * (commit included) -- the loop body of SURVEY 3.2 when nothing is sharded.
 * Same results as the two calls, in fewer launches: the fused sweep kernels
 * empty the additive tables on their way, and commit + prepare + the CRP terms
 * of the next sweep are one kernel (3 launches per step for a single nich
 * feature instead of 7), which is what bounds small problems.
 * MSC_SWEEP_GRAPH=1 in the environment additionally captures the step as a HIP
 * graph once consecutive calls repeat (same view, rows, z_dev, seed; sweep =
 * previous + 1) and replays it; off by default because it measured slower
 * than the launches it replaces on ROCm 7.2.
 */
int msc_sweep_step(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                   uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep);
/*
 * The row-sharded form of the step, up to the exchange: msc_sweep_assign +
 * msc_accumulate(MSC_ACC_RESET | MSC_ACC_NO_COMMIT) with the step's fusions.
 * Then all-reduce msc_state_reduce_buffers and call msc_state_commit_reduce.
 */
int msc_sweep_step_begin(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                         uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep);
/* how many msc_sweep_step calls on this state ran launch by launch / as a graph launch */
int msc_sweep_step_stats(const msc_state *st, uint64_t *eager_steps, uint64_t *graph_steps);

/*
 * nsweeps SEQUENTIAL collapsed Gibbs sweeps over rows [row0, row0+nrows): the reference's sampler (the
 * per-entity moves of entity_state.hpp:57-89), in which row i+1 is scored against the tables row i has just changed.
 * Each sweep visits the rows in the order order_dev (nullable: uint32[nrows] offsets from row0, the same for every
 * sweep of the call; NULL = ascending).  For each visited row:
 *   leave  if z_dev[offset] is in [0, ngroups) the row leaves that group (every feature's remove_value, the group
 *          count); an id outside that range is unassigned and the row only joins -- a sweep from an all-unassigned z
 *          is sequential CRP seating;
 *   score  every slot: log pseudocount + sum over features of score_value, against the tables as they now stand (what
 *          msc_score_value(..., MSC_SCORE_CRP_PRIOR) gives for the row; empty slots share alpha);
 *   draw   util::sample_discrete_log semantics with philox_uniform01(seed, sweep + s, row_id0 + offset) in sweep s of
 *          the call: the counter msc_sweep_step uses for that row, so a one-row call draws what msc_sweep_step draws;
 *   join   the drawn group; z_dev[offset] is written.
 * z_dev: int32[nrows] for the row range.  trace_dev (nullable): int32[nsweeps * nrows], receives z of the row range
 * after every sweep.  Every table is current on return (additive sums, fields, score constants, CRP terms, as after
 * msc_entity_op): msc_score_value, msc_score_data, msc_state_get_ss, msc_sweep_step and msc_sample_predictive may
 * follow with nothing rebuilt.  Asynchronous; does not touch msc_sweep_step's device (seed, sweep) pair or its graph.
 * Exactness: the chain is the collapsed CRP Gibbs sampler whenever an empty slot exists at every visit, which always
 * holds when ngroups >= the rows in play; with every slot full it is the chain truncated to ngroups groups.
 * Families: bb, gp, bnb, dd, nich and noop (masked entries honoured); at most 256 features and 8192 groups.  States
 * that hold niw or dm features (prepare kernels of their own), or bbnc (a slot that empties mid-sweep would be offered
 * with a stale p; free slots' p is drawn between sweeps) return MSC_EUNSUPPORTED.  MSC_EINVAL between
 * msc_sweep_step_begin and msc_state_commit_reduce.  An order entry >= nrows skips that visit, and a leave from an
 * empty group only joins; both surface as MSC_EDEVICE at the next call.
 */
int msc_sweep_sequential(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                         uint64_t row_id0, int32_t *z_dev, const uint32_t *order_dev, uint32_t nsweeps, uint64_t seed,
                         uint64_t sweep, int32_t *trace_dev);

/*
 * MANY sequential chains in one launch.  An msc_chains handle groups nchains states of one context; msc_chains_sweep
 * runs msc_sweep_sequential's sweeps on all of them at once, a workgroup (one compute unit) per chain, where a single
 * call occupies one compute unit of the card.  The chains need nothing from each other.
 * msc_chains_create: at least one state; all on one context; pairwise distinct (two workgroups on one state's tables
 * would race); equal ngroups and equal feature lists (family and dim) -- hyper-parameters, suff-stats and alpha may
 * differ per chain.  A violation is MSC_EINVAL and names the offending index.  The families and limits are
 * msc_sweep_sequential's (niw, dm, bbnc: MSC_EUNSUPPORTED; at most 256 features and 8192 groups), checked here once
 * since no call changes them.  While the handle lives its member states cannot be destroyed: msc_state_destroy
 * returns MSC_EINVAL (destroy the handle first); every other call on a member state keeps working between sweeps.
 * msc_chains_destroy waits for the context's stream.  msc_chains_size: the number of chains.
 *
 * msc_chains_sweep: chain c performs exactly what
 *   msc_sweep_sequential(states[c], view, cols, row0, nrows, row_id0, z_dev + c * ld_z, order of c, nsweeps,
 *                        host_seeds[c], sweep, ...)
 * performs -- the same arithmetic in the same order, so the same bits in z, the tables and the trace.  That is the
 * contract.  Layout:
 *   z_dev         int32, chain c's row range at z_dev + c * ld_z, ld_z >= nrows;
 *   order_dev     nullable; uint32 offsets from row0; ld_order == 0: one order of nrows entries shared by all chains,
 *                 else chain c's at order_dev + c * ld_order, ld_order >= nrows;
 *   host_seeds    uint64[nchains] on the host: the Philox key of each chain.  The counter of the draw at a row in sweep
 *                 s of the call stays (row_id0 + offset, sweep + s), whatever the chain;
 *   trace_dev     nullable; int32 [nchains][ntrace][nrows], contiguous, ntrace = nsweeps / trace_every: after sweep s of
 *                 the call, when (s + 1) % trace_every == 0, chain c's z of the row range goes to sample
 *                 (s + 1) / trace_every - 1.  As [nchains * ntrace][nrows] it is what msc_zmatrix_add takes;
 *   occupied_dev  nullable; uint32 [nchains][ntrace]: the chain's occupied slots (ngroups - its empty slots) at the same
 *                 moments;
 *   trace_every   ignored when both are null, otherwise >= 1 (a trace_every > nsweeps writes no sample).
 * On return (asynchronously) every table of every member state is current, as after msc_sweep_sequential.  nrows == 0
 * or nsweeps == 0 changes nothing and returns MSC_OK.  The per-chain table (pointers, keys, alpha: read afresh from the
 * states at every call) reaches the device through a buffer the handle owns; the host fills one of TWO pinned staging
 * areas, taken in turn, each with an event recorded after the copy out of it, and waits for that event before it fills
 * the area again, so a call never writes under a pending copy; the device buffer is ordered by the stream (calls on one
 * handle go to one stream, or the caller orders them).  A launch takes max(1, V / R) visits of every chain, V the
 * visits msc_sweep_sequential would give the costliest member and R = ceil(nchains / compute units) the rounds a grid
 * beyond the compute units runs in (one workgroup is resident per compute unit), so a launch stays inside its time
 * budget on a shared card.
 * Errors: MSC_EINVAL for a null argument, nrows >= 2^32, ld_z < nrows, ld_order neither 0 nor >= nrows, trace_every
 * == 0 with a trace or an occupied array, rows outside the view, a column that does not fit a feature, or a member
 * between msc_sweep_step_begin and msc_state_commit_reduce (the index is named); MSC_EDEVICE when an earlier kernel
 * reported an error.  An order entry >= nrows skips that visit and a leave from an empty group only joins, in any
 * chain; both surface as MSC_EDEVICE at the next call (one error word serves all chains).
 */
typedef struct msc_chains msc_chains;
int msc_chains_create(msc_state *const *states, uint32_t nchains, msc_chains **out);
int msc_chains_destroy(msc_chains *ch);
int msc_chains_size(const msc_chains *ch, uint32_t *nchains);
int msc_chains_sweep(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                     uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order,
                     uint32_t nsweeps, const uint64_t *host_seeds, uint64_t sweep,
                     uint32_t trace_every, int32_t *trace_dev, uint32_t *occupied_dev);

/*
 * PART of one sweep of every chain, with the log predictive of every visit: what a particle filter over the rows needs
 * (common_amd.ChainEnsemble.smc).  msc_chains_visit performs positions [pos0, pos0 + npos) of the order of ONE sweep for
 * every chain: exactly the visits at those positions of
 *   msc_chains_sweep(ch, view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, 1, host_seeds, sweep, ...)
 * -- the same counters (row_id0 + offset, sweep), the same arithmetic in the same order, so the same bits in z and in
 * every table.  Calls over [0, a), [a, b), ..., [y, nrows) together are that sweep.  z_dev, ld_z, order_dev, ld_order,
 * host_seeds: as msc_chains_sweep.  On top of the sweep's work a visit has two outputs, which move no draw:
 *   visit_logp_dev  nullable; float, chain c's row at visit_logp_dev + c * ld_logp, ld_logp >= nrows, indexed by order
 *                   POSITION: the visit at position p writes entry p with
 *                     inc = m + log(total) - log(n + alpha)   (in double, rounded to float)
 *                   where m and total = sum_k exp(t_k - m) are the block max and sum the draw itself makes of the row's
 *                   scores t_k (log pseudocount + the features' score_value, as the tables stand at that visit, after
 *                   the row has left its own group) and n is the number of rows seated at that moment, the row itself
 *                   not among them.  It is the row's log predictive density given the rows seated before it: the
 *                   quantity msc_score_marginal defines, taken against the tables of that visit.  -inf when total == 0
 *                   or m == -inf.  Entries of positions outside [pos0, pos0 + npos), and of a skipped visit, are left
 *                   as they are;
 *   logw_dev        nullable; double[nchains] on the device: chain c's entry is ADDED to (the caller zeroes it) -- inc in
 *                   double, visit by visit in visit order, by one thread: no atomics, no partial sums, so its bits do
 *                   not depend on how the positions are cut into calls, or a call into launches.
 * On return (asynchronously, on the context's stream) every table of every member state is current, as after
 * msc_chains_sweep.  npos == 0 returns MSC_OK and touches nothing.  The launch slicing by time budget, the two pinned
 * staging areas, the families and limits are msc_chains_sweep's.
 * Errors: MSC_EINVAL for pos0 + npos > nrows, visit_logp_dev with ld_logp < nrows, and whatever msc_chains_sweep
 * refuses (null argument, nrows >= 2^32, ld_z < nrows, ld_order neither 0 nor >= nrows, rows outside the view, a column
 * that does not fit a feature, a member between msc_sweep_step_begin and msc_state_commit_reduce); MSC_EDEVICE when an
 * earlier kernel reported an error.  Nothing is written when a call is refused.
 *
 * msc_chains_clone: for every chain c with a = host_ancestors[c] != c, chain c BECOMES chain a: one launch copies, for all
 * such pairs, state a's additive tables (the two buffers of msc_state_reduce_buffers: the int64 sums, the group counts
 * leading, and the float64 sums) onto state c's and the z row z_dev + a * ld_z onto z_dev + c * ld_z (nrows entries,
 * ld_z >= nrows).  The sums are copied, not accumulated again from z -- msc_accumulate adds its double sums with atomics
 * in an order that varies from run to run -- so a clone holds its ancestor's bits.  host_ancestors: uint32[nchains] on the
 * host, read before the call returns.  State c's reference fields, score constants and CRP terms are marked stale and
 * rebuilt from the copied sums by the next call that needs them (the next msc_chains_visit / msc_chains_sweep, or a
 * getter on the state); they come out as the ancestor's, which the same kernels' code built from the same sums.  Hyper-
 * parameters and alpha are NOT copied: a chain keeps its own.  Reads: the sources' additive tables and z rows.  Writes:
 * the destinations' only.  Sources, chains with host_ancestors[c] == c, and every state's hyper-parameters stay valid
 * and untouched.  No random numbers are drawn.  Asynchronous on the context's stream.  An all-identity array returns
 * MSC_OK and launches nothing.
 * Errors, with nothing changed: MSC_EINVAL for a null argument, ld_z < nrows, an entry >= nchains (named), a source that
 * is itself overwritten (host_ancestors[a] != a: ancestors must survive in place, so no pair reads what another writes),
 * or a member between msc_sweep_step_begin and msc_state_commit_reduce; MSC_EDEVICE when an earlier kernel reported an
 * error.
 */
int msc_chains_visit(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                     uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order,
                     uint64_t pos0, uint64_t npos, const uint64_t *host_seeds, uint64_t sweep,
                     double *logw_dev, float *visit_logp_dev, uint64_t ld_logp);
int msc_chains_clone(msc_chains *ch, const uint32_t *host_ancestors, int32_t *z_dev, uint64_t ld_z, uint64_t nrows);

/*
 * The POSTERIOR-AVERAGED row predictive density over the chains of an ensemble, in one pass over (rows x chains):
 *   mix[r] = logsumexp_c (lw_c + L[c][r])   ~   log p(x_r | data) = log sum_c w_c p(x_r | state_c)
 * for rows [row0, row0 + nrows) of the view -- the held-out log-likelihood or anomaly score of the fitted model rather
 * than of one sample; the difference of two calls over nested feature sets is a model-averaged conditional density.
 *   L[c][r]   what msc_score_marginal(states[c], view, cols, row0, nrows, NULL, 0, ...) defines for logp_dev[r] (no
 *             leave-one-out): logsumexp_k t[r][k] - log(n_c + alpha_c), taken over the SELECTED features only -- an
 *             unselected feature contributes nothing to any t[r][k], exactly as a masked entry does.  The scores are the
 *             score kernels' accurate form (table lookups, the compensated nich evaluation, the CRP term added as its
 *             (hi, lo) pair, lo first; gp and bnb values beyond the exact table in the large-count forms of
 *             msc_sweep_sequential); the sum over the groups is kept in double and L is formed in double.
 *   features  host array of nfeatures strictly ascending feature indices < the states' feature count, read before the
 *             call returns; NULL or nfeatures == 0: every feature.
 *   logw_dev  nullable; double[nchains] on the device, only read: the chains' log weights, which need not be normalised:
 *             lw_c = logw_dev[c] - logsumexp(logw_dev), in double on the device.  NULL: lw_c = -log(nchains).  A weight
 *             of -inf excludes its chain.  If NO weight is finite -- all -inf -- or one is NaN or +inf, every entry of
 *             mix is NaN (chain_logp is unaffected).
 *   flags     reserved: 0.
 *   mix_dev   nullable; float[nrows]: (float)logsumexp_c(lw_c + L[c][r]).  The sum over the chains is taken in double
 *             in a FIXED order -- ascending chains within a slice of the chains, then ascending slices; no float
 *             atomics -- so the same call gives the same bits on every run.  -inf when no chain of finite weight can
 *             hold the row.
 *   chain_logp_dev, ld_logp   nullable; float, chain c's row at chain_logp_dev + c * ld_logp (ld_logp >= nrows):
 *             (float)L[c][r].  At least one of the two outputs is non-NULL.
 * A one-hot weight vector (one finite entry, the others -inf) gives mix bit-equal to that chain's row of chain_logp.
 * A row's results depend on nothing but the row: the size of the group tiles and the cut of the chains into slices follow
 * from the ensemble, the device and the rows of the VIEW, never from row0 / nrows, so a call over a sub-range gives the
 * whole call's bits.
 * Families: those an ensemble holds (bb, gp, bnb, dd, nich, noop).  Every member is read-only apart from the view it is
 * left bound to (a later msc_chains_sweep on the training view gives the bits it would have given without this call); its
 * score tables and CRP terms are brought current first, as msc_score_marginal does.  The per-chain table reaches the
 * device through the two pinned staging areas of msc_chains_sweep.  Asynchronous on the context's stream; the call itself
 * does not synchronise with the device (it may wait for the upload of the call before last to leave its staging area,
 * and binding a view whose count columns' maxima are not known yet finds them once, as every call that binds a view).
 * nrows == 0 binds the view, writes nothing and returns MSC_OK.
 * Errors, with nothing written: MSC_EINVAL for a null ch or view, both outputs NULL, chain_logp_dev with ld_logp < nrows,
 * a feature list that is not strictly ascending or names a feature outside the state, non-zero flags, nrows >= 2^32,
 * rows outside the view, a column that does not fit its feature, a member between msc_sweep_step_begin and
 * msc_state_commit_reduce (the index is named), or a member whose exact gp / bnb table has other rows than member 0's
 * (its own msc_state_set_col_bounds differ: one tile plan serves every chain); MSC_EDEVICE when an earlier kernel
 * reported an error.
 */
int msc_chains_score_marginal(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                              const uint32_t *features, uint32_t nfeatures, const double *logw_dev, uint32_t flags,
                              float *mix_dev, float *chain_logp_dev, uint64_t ld_logp);

/*
 * POSTERIOR PREDICTIVE DRAWS from the model average of an ensemble -- multiple imputation, posterior predictive checks,
 * synthetic rows -- for rows [row0, row0 + nrows) of the view, in one pass: row r draws a chain with probability
 * ~ w_c p(x_r,observed | state_c), a group of that chain ~ CRP term x likelihood of the observed entries, and its entries
 * from that group's predictive.  R = row_id0 + r is the row's global id.  flags: 0 or MSC_PRED_MASKED_ONLY.
 *   chain_out_dev, z_out_dev   nullable; int32[nrows]: the chain and the group row r used, or -1 / -1 for a skipped row.
 *   out_dev   one entry per state feature, as for msc_sample_predictive: NULL = not drawn, else nrows values of the
 *             family's type (bb uint8, gp / bnb uint32, dd int32, nich float).
 * 1. Chain weights.  Lf[c][r] is the float msc_chains_score_marginal(ch, view, cols, row0, nrows, NULL, 0, ...) writes to
 *    chain_logp_dev for chain c and row r (every feature counts, masked entries contribute nothing, no leave-one-out);
 *    lw_c is that call's normalised log weight of logw_dev (NULL: equal weights; -inf leaves a chain out).  The draw reads
 *    those very bits: the two launches of that call run first, into a scratch of the handle.
 * 2. Chain draw.  One Philox4x32-10 block, key = seed ^ 0xC2B2AE3D27D4EB4F, counter = (R & 0xffffffff, R >> 32,
 *    sweep & 0xffffffff, 0x80000000); u1 from its words (w0, w1), u2 from (w2, w3), each msc_sample_predictive's two-word
 *    uniform ((a >> 5) * 2^26 + (b >> 6) + 0.5) * 2^-53.  In double, chains ascending: a_c = lw_c + (double)Lf[c][r],
 *    M = max a_c, e_c = exp(a_c - M) (0 for -inf), S = sum e_c; the row's chain is the smallest c whose running sum
 *    e_0 + .. + e_c exceeds u1 * S, or, if rounding lets none exceed it, the last c with e_c > 0.  If no a_c is finite, or a
 *    weight is NaN or +inf, the row is SKIPPED as msc_sample_predictive skips a row: chain_out[r] = z_out[r] = -1 and none
 *    of its value outputs is written.
 * 3. Group draw in the chosen chain c.  t[k], k ascending, is the float total msc_chains_score_marginal forms for (chain
 *    c, row, group k): the features' scores added in ascending feature order (table lookups, the compensated nich
 *    evaluation, gp / bnb counts beyond the exact table in the large-count forms), then the CRP term lo first and hi last,
 *    empty slots sharing alpha.  In double, m = max t, e_k = exp(t[k] - m); a first pass over the groups forms m and
 *    s = sum e_k together (s is rescaled when the maximum rises), a second the running sum: the group is the smallest k
 *    whose running sum exceeds u2 * s, with the chain draw's fallback.
 * 4. Values.  Every drawn entry of a row with chain c and group k equals, bit for bit, what
 *    msc_sample_predictive(states[c], ..., z = k for that row, same flags, seed, sweep, row_id0) writes: the same counters
 *    (key = seed, the 0x80000000 | f << 16 | b streams), the same parameter formulas in double read from chain c's raw
 *    sufficient statistics and hp.  With MSC_PRED_MASKED_ONLY observed entries are copied.
 * 5. A row's results depend on the row alone: a call over a sub-range with a matching row_id0 gives the whole call's bits,
 *    and a repeated call the same bits.  The rows go through the handle's scratch (at most 256 MiB of Lf) a chunk at a
 *    time, which moves no bit.  No atomics.  m imputations are m calls with sweep = 0 .. m - 1.
 * 6. Every member is read-only apart from the view it is left bound to: tables, counts, hp, alpha and the sweeps' device
 *    (seed, sweep) pair stay as they were (a later msc_chains_sweep on the training view gives the bits it would have
 *    given without this call).  Asynchronous on the context's stream; the call synchronises with the device no more than
 *    msc_chains_score_marginal does.
 * Families: bb, gp, bnb, dd, nich; MSC_EUNSUPPORTED for a noop feature with a non-NULL output.
 * nrows == 0 binds the view, writes nothing and returns MSC_OK.
 * Errors, with nothing written: those of msc_chains_score_marginal -- MSC_EINVAL for a null ch or view, nrows >= 2^32, rows
 * outside the view, a column that does not fit its feature, a member between msc_sweep_step_begin and
 * msc_state_commit_reduce (the index is named), members whose exact gp / bnb tables differ in their rows -- and
 * MSC_EINVAL for unknown flags, a null out_dev and a drawn feature index >= 32768; MSC_EDEVICE when an earlier kernel
 * reported an error.
 */
int msc_chains_sample_predictive(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                                 uint64_t nrows, uint64_t row_id0, const double *logw_dev, uint32_t flags, uint64_t seed,
                                 uint64_t sweep, int32_t *chain_out_dev, int32_t *z_out_dev, void *const *out_dev);

/*
 * The BLOCKED (uncollapsed) Gibbs sampler for the truncated stick-breaking Dirichlet process mixture (Ishwaran & James,
 * JASA 2001): an exact sampler that is parallel over rows.  With ngroups = K slots a sweep draws, given the tables,
 * every slot's component parameters from their conjugate posteriors and the mixture weights from the stick-breaking
 * posterior, and then every row's slot INDEPENDENTLY from pi_k f(x | theta_k): rows do not depend on each other, so
 * nothing is stale.  Against the CRP posterior the only error is the truncation: the L1 distance of the marginal
 * density is at most 4 N exp(-(K - 1) / alpha) (N rows) -- 1e-12 at K = 32, alpha = 1, N = 6.
 *
 * msc_blocked_draw: makes the reference's fields and the group counts current, then draws, for every slot k < K (an
 * empty slot draws from the prior)
 *   V_k ~ Beta(1 + n_k, alpha + sum_{l > k} n_l) for k < K - 1, V_{K-1} = 1;
 *   log pi_k = log V_k + sum_{l < k} log(1 - V_l), summed in slot order in double;
 * and the parameters of every feature into a state-owned float32 table of slices, [slice][ld] with the slot minor:
 *
 *   family  posterior draw (hp + the slot's suff-stats)                      slices                   log-lik. of value v
 *   bb      p ~ Beta(alpha + heads, beta + tails)                            log(1 - p), log p        slice v
 *   gp      lambda ~ Gamma(alpha + sum, rate inv_beta + count)               -lambda, log lambda      s0 + v s1
 *   bnb     p ~ Beta(alpha + r count, beta + sum)                            r log p, log(1 - p)      s0 + v s1
 *   dd      theta ~ Dirichlet(alpha_i + c_i): dim gammas from one stream     log theta_i, i < dim     slice v
 *           in value order, normalised in double
 *   nich    sigma^2 = nu' sigma'^2 / chi2(nu'), mu ~ N(mu', sigma^2/kappa')  -log(2 pi sigma^2) / 2,  s0 + s2 (v - s1)^2
 *           (kappa' = kappa + n, nu' = nu + n, mu' = (kappa mu + n mean) /   mu, -1 / (2 sigma^2)
 *           kappa', nu' sigma'^2 = nu sigma^2 + ctv + n kappa (mu-mean)^2 / kappa')
 *   noop    --                                                               none                     0
 *
 * (terms that do not depend on the slot -- lgamma(v + 1) and the like -- are dropped: they cancel in the draw).  Draws
 * are made in double and stored as floats; every stored value is finite (the log of 0 is stored as -1e28).  The Philox
 * key is seed ^ 0x9FB21C651E98DF25; the stream of (slot, feature) is that of msc_sample_predictive's entries with the
 * slot as the row (counter words: slot, slot >> 32, sweep, 0x80000000 | feature << 16 | block), the stick weights take
 * feature 0x7fff.  Nothing else enters a counter: two states with equal tables -- the ranks of a row-sharded run after the
 * all-reduce -- draw bit-identical tables.
 *
 * msc_blocked_tables: the table of one feature (*dev = float[*nslices][*ld], the slot minor) or, feature == UINT32_MAX,
 * the log weights (one slice).  The pointers stay valid for the state's life.
 *
 * msc_blocked_assign: for every row of [row0, row0 + nrows): s_k = log pi_k + sum over features of the log-likelihood
 * of the row's value under slot k (masked entries skipped; dd values clamped into [0, dim)), over all K slots, then
 * z_dev[r] by util::sample_discrete_log semantics with the dart philox_uniform01(seed, sweep, row_id0 + r) -- the
 * counter msc_sweep_step uses.  Reads the drawn table only; no table of the state is touched.  MSC_EINVAL when no draw
 * was made, when anything that changes tables, hyper-parameters, alpha or group counts ran since the draw (the draw is
 * stale), and between msc_sweep_step_begin and msc_state_commit_reduce.
 *
 * msc_sweep_blocked: sweep s of nsweeps does msc_blocked_draw(seed, sweep + s), msc_blocked_assign(seed, sweep + s),
 * msc_accumulate(MSC_ACC_RESET) of the same rows (commit included).  The first draw conditions on the state's tables as
 * they stand at the call (z_dev's content is not read).  trace_dev (nullable): int32[nsweeps * nrows], z after every
 * sweep; top_slot_dev (nullable): uint32[nsweeps], the highest occupied slot after every sweep -- K - 1 means the
 * truncation binds and K should be raised.  Asynchronous; the reference's fields, the additive sums and the group
 * counts are current on return, and msc_sweep_step's device (seed, sweep) pair and graph are untouched.
 *
 * Families: bb, gp, bnb, dd, nich and noop.  States with niw, dm or bbnc features: MSC_EUNSUPPORTED from all four --
 * but for one shape, the Dirichlet-process Gaussian mixture:
 *
 * A state whose ONLY feature is one niw column of dim <= 32 is taken by all four calls (dim 33 .. 128: MSC_EUNSUPPORTED,
 * "the blocked sweep takes a niw feature of dimension at most 32"; split-merge and the sequential sweep refuse it as
 * before).  With kappa' = kappa + n, nu' = nu + n, mu' = (kappa mu + sum_x) / kappa', Psi' = psi + sum_xxT + kappa mu mu^T
 * - kappa' mu' mu'^T = L L^T, a slot draws a lower-triangular whitening matrix V = T L^-1, T lower triangular with
 * T_ii^2 ~ chi2(nu' - dim + 1 + i) (0-based: the degrees of freedom increase down the diagonal) and T_ij ~ N(0, 1), j < i,
 * so that Sigma = (V^T V)^-1 ~ IW(Psi', nu'); and mu = mu' + V^-1 z / sqrt(kappa'), z ~ N(0, I).
 *
 *   family  posterior draw                                                   slices                   log-lik. of value x
 *   niw     V, mu as above                                                   -(dim / 2) log 2 pi      s0 - |V x - V mu|^2 / 2
 *                                                                            + sum_i log V_ii         (V, mu: in double, below)
 *
 * Row i of a slot's matrix draws from the stream of (slot | (i + 1) << 32, feature) -- counter words slot, i + 1, sweep,
 * 0x80000000 | feature << 16 | block; every other stream above has a second word of 0 --: z_i first, then T_i0 ..
 * T_i,i-1, then the chi-square of T_ii.  The assign pass evaluates |V x - V mu|^2 in double (a row with any masked
 * element scores log pi_k alone).
 *
 * msc_blocked_niw_params: the matrices of the latest draw, in double, as the assign pass reads them: *mean =
 * double[K][*dim], *whiten = double[K][*dim (*dim + 1) / 2], V's lower triangle packed by rows (entry (i, j), j <= i, at
 * i (i + 1) / 2 + j).  Every value is finite; zeros before the first draw.  The pointers stay valid for the state's
 * life.  A state of any other shape: the refusal msc_blocked_draw gives it, or MSC_EINVAL where it holds no niw feature.
 */
int msc_blocked_draw(msc_state *st, uint64_t seed, uint64_t sweep);
int msc_blocked_tables(msc_state *st, uint32_t feature, const float **dev, uint32_t *nslices, uint32_t *ld);
int msc_blocked_niw_params(msc_state *st, uint32_t feature, const double **mean, const double **whiten, uint32_t *dim);
int msc_blocked_assign(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                       uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep);
int msc_sweep_blocked(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                      uint64_t row_id0, int32_t *z_dev, uint32_t nsweeps, uint64_t seed, uint64_t sweep,
                      int32_t *trace_dev, uint32_t *top_slot_dev);

/*
 * SPLIT-MERGE Metropolis-Hastings proposals (Jain & Neal 2004 / 2007, with an uncollapsed launch): moves that split one
 * group in two or merge two groups in one step, which no chain of single-row moves makes.  One call runs nproposals
 * proposals back to back without a host synchronisation; proposal p uses the sweep counter sweep + p.
 *
 *   1. anchors: an ordered pair of distinct rows (i, j), uniform over the call's nrows rows.  An unassigned anchor (z
 *      outside [0, K)) makes the proposal VOID; so does nrows < 2.
 *   2. S = the rows of the call with z in {z_i, z_j}; z_i = z_j: a SPLIT (void when no slot is empty), else a MERGE.  A
 *      void proposal changes nothing and is counted.
 *   3. launch -- a function of (S, i, j, data, hyper-parameters, alpha, streams) only, never of how S is divided now:
 *      pair labels l_i = 0, l_j = 1, a coin for every other row of S; then launch_iters times: the two pair slots'
 *      suff-stats from l, their parameters from the conjugate posteriors (msc_blocked_draw's draws) and the weights as
 *      the K = 2 stick V_0 ~ Beta(1 + n_0, alpha + n_1), and every free row (not an anchor) redraws l_r with
 *      P(l_r = s) ~ pi_s prod_f lik_f(x_rf | theta_s), masked entries adding nothing.  One more accumulate and draw give
 *      theta*.
 *   4. final labels l': a split draws them under theta* for the free rows, a merge takes l'_r = [z_r = z_j]; either way
 *      log q = sum over free rows of log P(l'_r | theta*), added in double in a fixed order (lanes, waves, workgroups).
 *   5. with n_0, n_1 the sizes under l' and sd(.) the sum over features of score_data of a block:
 *        log A_split = log alpha + lgamma(n_0) + lgamma(n_1) - lgamma(n_0 + n_1) + sd(0) + sd(1) - sd(S) - log q
 *        log A_merge = -(the same without log q) + log q
 *      accepted when log u < log A; the decision is made on the device in double.
 *   6. apply: a split moves the rows with l' = 1 to the lowest-numbered empty slot, a merge the rows of z_j's group to
 *      z_i's.  Rows outside S are never written.
 *
 * Random numbers: Philox4x32-10 under keys made from seed ^ 0xA0761D6478BD642F (a key no sweep, grid draw, slice step,
 * predictive or blocked draw uses): stream s has key (seed ^ that) + s 0x9E3779B97F4A7C15; s = 0 the proposal's darts
 * (counters 0 .. 4: anchor i from two darts, anchor j from two, the acceptance), s = 1 the coins (counter: the row's
 * global id row_id0 + offset), s = 2 + t pass t of the launch (parameters: msc_blocked_draw's streams under this key;
 * labels: the row's global id).  common_amd/csrc/splitmerge_math.hpp states every stream and the arithmetic.
 *
 * Outputs, all nullable, all device memory:
 *   log_dev       double[nproposals][8] = {i, j, kind (0 split, 1 merge, 2 void), n_0, n_1, log q, log A, accepted};
 *                 i and j are offsets from the call's first row
 *   trace_dev     int32[nproposals][nrows], z after each proposal
 *   proposed_dev  int32[nproposals][nrows], l' of each proposal, -1 outside S
 *   counters_dev  uint64[5] = {splits proposed, splits accepted, merges proposed, merges accepted, void}, added to
 *
 * The group sizes must be current at the call (they say which slots are empty) and follow the proposals on the device.
 * On return the reference's fields, the additive sums and the group counts are those of msc_accumulate(MSC_ACC_RESET) of
 * the call's rows under the final z (one accumulate at the end of the call); a blocked draw made before is stale.
 * Asynchronous.  MSC_EINVAL between msc_sweep_step_begin and msc_state_commit_reduce; MSC_EUNSUPPORTED for states with
 * niw, dm or bbnc features.
 *
 * msc_split_merge_tables: theta* of the last proposal made, as msc_blocked_tables gives the blocked sweep's table: one
 * feature's slices (*dev = float[*nslices][*ld], pair slots 0 and 1 the first two of a row) or, feature == UINT32_MAX,
 * the two log weights.
 */
int msc_split_merge(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                    uint64_t row_id0, int32_t *z_dev, uint32_t nproposals, uint32_t launch_iters, uint64_t seed,
                    uint64_t sweep, double *log_dev, int32_t *trace_dev, int32_t *proposed_dev, uint64_t *counters_dev);
int msc_split_merge_tables(msc_state *st, uint32_t feature, const float **dev, uint32_t *nslices, uint32_t *ld);

/*
 * SPLIT-MERGE PROPOSALS FOR EVERY CHAIN OF AN ENSEMBLE in one launch (kernels_chains_sm.hip k_sm_chains): workgroup c
 * makes nproposals proposals on member c, proposal p with the sweep counter sweep + p under the key host_seeds[c].  A
 * proposal is msc_split_merge's move above, step for step -- the same streams, anchors, coins, passes, draws, label darts,
 * acceptance ratio and dart -- so chain c proposes, decides and moves as msc_split_merge(states[c], ..., host_seeds[c],
 * ...) does.  Only the ORDER in which the double sums are formed differs (nich sum x and sum x^2, gp sum ln Gamma(v + 1),
 * log q): a thread adds its rows r = t, t + 256, ... in that order, a wave's lanes combine by shuffles, the waves are added
 * in wave order.  The order depends on nrows alone, so a call repeats its bits, and a call of P proposals gives the bits of
 * calls of P1 + P2 = P proposals with sweep advanced by P1.  States whose suff-stats are integers (bb, bnb, dd) match
 * msc_split_merge in every output bit but log q and log A.
 *
 * The call covers rows [0, nrows) of the view; nrows must be the view's row count.  z_dev: int32, chain c's row at
 * z_dev + c * ld_z.  EVERY TABLE OF EVERY MEMBER MUST BE THAT OF ITS z ROW at the call -- as after msc_accumulate of the
 * row, msc_chains_sweep or this call -- because an accepted proposal rewrites the two groups involved and leaves the rest
 * as it was.  On return every table of every member is current for the new z (additive sums, fields, score constants,
 * counts, CRP terms), as msc_chains_sweep leaves them: a sweep that follows launches nothing before its kernel.  A blocked
 * draw made before is stale.  A void or rejected proposal changes nothing but its outputs.
 *
 * Outputs: msc_split_merge's with a leading chain dimension, all nullable, all device memory: log_dev
 * double[nchains][nproposals][8], trace_dev and proposed_dev int32[nchains][nproposals][nrows], counters_dev
 * uint64[nchains][5], added to.  msc_split_merge_tables(states[c], ...) afterwards gives theta* of chain c's last proposal.
 *
 * A launch takes the whole proposals that fit a launch's time budget by an estimate from (nrows, features, launch_iters);
 * a chain has one workgroup, so the call suits an ensemble's shapes (thousands of rows a chain).  Asynchronous: no host
 * synchronisation.  nproposals == 0 checks its arguments, writes nothing and returns MSC_OK.
 * Errors, all before the first launch: MSC_EINVAL for a null argument, launch_iters > 1024, nrows != the view's rows,
 * ld_z < nrows, a member between msc_sweep_step_begin and msc_state_commit_reduce (the index is named); MSC_EUNSUPPORTED
 * when one proposal alone is estimated beyond the budget (use msc_split_merge on each member: its kernels are parallel
 * over rows).  Families: bb, gp, bnb, dd, nich, noop (what an ensemble holds).
 */
int msc_chains_split_merge(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t nrows,
                           uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, uint32_t nproposals, uint32_t launch_iters,
                           const uint64_t *host_seeds, uint64_t sweep, double *log_dev, int32_t *trace_dev,
                           int32_t *proposed_dev, uint64_t *counters_dev);

/* ---- multi-GPU hook ---------------------------------------------------- */
/*
 * The additive form of every table, ready for a sum all-reduce across row
 * shards: *dev_i64 = int64[n_i64] (counts), *dev_f64 = double[n_f64] (float
 * sums).  After reducing both in place call msc_state_commit_reduce.
 */
int msc_state_reduce_buffers(msc_state *st, void **dev_i64, size_t *n_i64, void **dev_f64,
                             size_t *n_f64);
/*
 * The same two tables as ONE float64 buffer, for a collective that takes one dtype (the payload is a few KB, so an
 * exchange costs the collective's latency: one all-reduce, not two): msc_state_reduce_pack copies counts (as doubles --
 * integers below 2^53 add exactly and in any order, so they come back bit-exact) and float sums into a buffer the state
 * owns and returns it; sum-all-reduce *pack_dev in place; msc_state_reduce_unpack copies both back; then
 * msc_state_commit_reduce.  One small launch each (common_amd/dist.py drives torch.distributed this way).
 */
int msc_state_reduce_pack(msc_state *st, void **pack_dev, size_t *n_f64);
int msc_state_reduce_unpack(msc_state *st);
/*
 * The rows of the WHOLE dataset, for a state whose sweeps run on a SHARD of it through a view of its own: a sweep picks
 * between two kernels by row count, and they associate a row's float sum differently, so a shard must pick what the
 * unsharded sweep would (it then draws identical assignments).  Row ranges of ONE view need nothing (the default is the
 * bound view's row count); 0 restores that default.
 */
int msc_state_set_sweep_rows(msc_state *st, uint64_t global_rows);
/*
 * The column bounds of the WHOLE dataset, for the same states.  A count feature's exact tables cover 0 .. its column's
 * maximum, and the maxima decide the plan: table sizes, how features pack into groups, masked columns' sentinels, which
 * tile / narrow / lane <-> row kernel runs, and (a count >= 1024) the generic sweep.  A shard's maxima are not the
 * whole's, so it must plan with the whole's or it may add a row's scores in another order and draw other bits.
 *   msc_state_col_bounds      this view's bounds for the state's features, in feature order: gp / bnb one value (the
 *                             column's maximum), dm dim + 1 (each category's maximum, then the largest row total), other
 *                             families none.  n must be that count (MSC_EINVAL naming it).  Binds the view if needed.
 *   msc_state_set_col_bounds  the whole dataset's bounds (the elementwise MAX of every rank's msc_state_col_bounds), in the
 *                             same layout; from then on the state plans with max(view's own, given) (capped at the table
 *                             limit as before).  NULL / 0 restores the view's alone.  A change re-plans at the next call
 *                             and drops a captured step graph.
 * Row ranges of ONE view need neither; msc_accumulate_sharded installs both these and the rows when nranks > 1.
 */
int msc_state_col_bounds(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint32_t *out, size_t n);
int msc_state_set_col_bounds(msc_state *st, const uint32_t *bounds, size_t n);
int msc_state_commit_reduce(msc_state *st);

/*
 * The same exchange for hosts that are not Python: a communicator over RCCL (xGMI inside a node), one rank per
 * process and GPU.  The 128-byte id is created on one rank (msc_comm_unique_id) and carried to the others by the
 * caller's own means (MPI, a file, a socket), exactly as ncclGetUniqueId / ncclCommInitRank want it;
 * msc_comm_adopt wraps an ncclComm_t the caller already has.  librccl is resolved at the first of these calls.
 *   msc_state_allreduce      sums both additive tables in place across the ranks (one RCCL group, context's stream)
 *   msc_sweep_step_sharded   msc_sweep_step_begin + that + msc_state_commit_reduce: a whole sharded sweep step
 *   msc_accumulate_sharded   suff-stats of the GLOBAL assignment: local accumulate, exchange, commit.  What starts a
 *                            sharded run: with nranks > 1 it also exchanges the views' column bounds (RCCL MAX) and row
 *                            counts (RCCL SUM) and installs them (msc_state_set_col_bounds, msc_state_set_sweep_rows), so
 *                            that every rank's sweeps take the kernels of the unsharded sweep.  Synchronous.
 * With one rank these are msc_sweep_step / msc_accumulate.  Asynchronous (msc_comm_create / destroy are not).
 */
typedef struct msc_comm msc_comm;
size_t msc_comm_unique_id_bytes(void);
int msc_comm_unique_id(void *id_out, size_t nbytes);
int msc_comm_create(msc_context *ctx, const void *unique_id, size_t nbytes, int nranks, int rank, msc_comm **out);
int msc_comm_adopt(msc_context *ctx, void *nccl_comm, int nranks, int rank, msc_comm **out);
int msc_comm_destroy(msc_comm *comm);
int msc_comm_size(const msc_comm *comm, int *nranks, int *rank);
int msc_state_allreduce(msc_state *st, msc_comm *comm);
int msc_sweep_step_sharded(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                           uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep,
                           msc_comm *comm);
int msc_accumulate_sharded(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0,
                           uint64_t nrows, const int32_t *z_dev, msc_comm *comm);

/* ---- grid hyper-parameter inference (grid_feature_hp / grid_cluster_hp downstream) ---- */
/*
 * A grid of hyper-parameter points of one feature, or of the CRP concentration (feature MSC_HP_CLUSTER: blocks of one
 * float, alpha, every one > 0), owned by the state: npoints full hp blocks of block_floats = msc_hp_floats(family, dim)
 * floats each (the msc_state_set_hp layout) and, nullable, npoints log-prior values, copied to the device once and kept
 * on the host.  Freed by msc_hp_grid_destroy or with the state.  Synchronous.  MSC_EINVAL for a block size that is not
 * msc_hp_floats, npoints == 0 or a non-positive alpha; MSC_EUNSUPPORTED for niw (upstream defines no niw grid, and every
 * point would need its own factorisation of Psi).
 */
typedef struct msc_hp_grid msc_hp_grid;
#define MSC_HP_CLUSTER 0xFFFFFFFFu
int msc_hp_grid_create(msc_state *st, uint32_t feature, const float *host_blocks, size_t block_floats, uint32_t npoints,
                       const double *host_logprior, msc_hp_grid **out);
int msc_hp_grid_destroy(msc_hp_grid *grid);
/*
 * out_dev[g] (double[npoints]) = log marginal likelihood of the feature's groups under grid point g, no prior:
 * sum over the counted slots k of score_data(hp = point g, group k) (entity_state.hpp score_likelihood), in double, in a
 * fixed order (two calls on the same tables give the same bits).  The counted slots are those with a non-zero group count,
 * or, with slots_dev (device uint8[ngroups]), those with a non-zero byte -- e.g. every group a group_manager holds, empty
 * ones included; no other slot is read.  The CRP grid: out_dev[g] = score_assignment(alpha_g) of the group counts
 * (group_manager.hpp:207-218; slots_dev does not apply).  Asynchronous.  MSC_EINVAL between msc_sweep_step_begin and
 * msc_state_commit_reduce.
 */
int msc_hp_grid_score(msc_hp_grid *grid, const uint8_t *slots_dev, double *out_dev);
/*
 * One grid Gibbs step for n grids of the state (at most one per feature; MSC_HP_CLUSTER allowed): score every grid as
 * above, add its prior, draw a point from the softmax (the CDF in double in index order, dart = Philox(seed, sweep,
 * stream) with stream = 2^64 - 1 - feature, and 2^64 - 1 - nfeatures for alpha: counters no sweep gives a row), and
 * install it exactly as msc_state_set_hp / msc_state_set_alpha would.  chosen_host[i] = index drawn from grids[i];
 * scores_dev (nullable; per grid a device double[npoints] or NULL) receives prior + likelihood.  Every rank of a sharded
 * sweep holding the same tables and passing the same seed draws the same points.  Synchronous: ONE host synchronisation
 * whatever n is.  MSC_EINVAL when a grid has no point of finite positive weight (its feature keeps its hp) and between
 * msc_sweep_step_begin and msc_state_commit_reduce.
 */
int msc_hp_grid_gibbs(msc_state *st, msc_hp_grid *const *grids, uint32_t n, const uint8_t *slots_dev, uint64_t seed,
                      uint64_t sweep, uint32_t *chosen_host, double *const *scores_dev);

/* ---- slice sampling of hyper-parameters and bbnc group parameters (downstream's hp / theta kernels) ---- */
/*
 * Two kinds of target, each updated by one slice step:
 *   hyper-parameter coordinate: one float of a feature's hp block (msc_state_set_hp layout), or the CRP alpha
 *     (feature MSC_HP_CLUSTER, coord 0).  Target of a feature coordinate:
 *       g(x) = sum over the counted slots k of score_data(hp with coordinate := x, group k) + prior(x)
 *     the sum msc_hp_grid_score computes (in double, in a fixed order; counted: a non-zero group count, or with slots_dev
 *     a non-zero byte; no other slot is read).  Target of alpha: score_assignment(alpha) of the device counts + prior.
 *   group parameter: the p of a counted bbnc slot, target bbnc_score_data(hp, heads, tails, p) -- the Beta(alpha, beta)
 *     prior plus the likelihood, so the stationary law of p is Beta(alpha + heads, beta + tails).
 * Supports (a target is -inf outside and never evaluated there): bb / bbnc / bnb alpha, beta > 0; gp alpha, inv_beta > 0;
 * nich mu any finite value, kappa, sigmasq, nu > 0; alpha > 0; bbnc p in (0, 1).  MSC_EUNSUPPORTED: bnb r (an integer),
 * dd / dm alphas, niw (and noop).
 * Priors, in double on the device: FLAT 0; EXPONENTIAL(lambda = prior_a) log lambda - lambda x (-inf for x < 0);
 * NORMAL(mu = prior_a, sigma2 = prior_b) -0.5 log(2 pi sigma2) - 0.5 (x - mu)^2 / sigma2; NONINF_BETA -2.5 log(x + y)
 * with y the feature's coordinate `partner` at its current value -- downstream's tuple key ('alpha', 'beta') is two
 * entries, each against the joint prior with the other as partner.
 * The step (Neal 2003, "Slice sampling", Fig. 3 stepping out with m = 64, Fig. 5 shrinkage), x0 the current value, w the
 * width, u_b the uniforms below; the interval is kept in double and every point the target is evaluated at is first
 * rounded to float32:
 *   y = g(x0) + log u_0;  L = x0 - w u_1, R = L + w;  J = floor(m u_2), Kr = m - 1 - J
 *   while J > 0 and y < g(L): L -= w, J--;   while Kr > 0 and y < g(R): R += w, Kr--
 *   proposal j = 0, 1, ...: x1 = float(L + u_{3+j} (R - L)); accept if y < g(x1), else L = x1 if x1 < x0, R = x1 if not
 *   after 256 rejected proposals x0 is kept (the update "stalls": floating point has collapsed the interval)
 * The accepted float is installed.  The entries of one feature are updated one after another in the caller's order,
 * each against the values installed before it; different features, alpha and different bbnc slots are independent.
 * When g(x0) is not finite (e.g. the current value lies outside the prior's support) that entry (bbnc: that slot) keeps
 * its value, every other target is still installed, and the call returns MSC_EINVAL naming it.
 * Random numbers: Philox4x32-10, key = seed ^ 0x2545F4914F6CDD1D (a key no sweep, grid draw or predictive uses);
 *   hyper-parameter entry: counter (target, entry, sweep & 0xffffffff, b), target = the feature or nfeatures for alpha,
 *     entry = the entry's position among that target's entries in the call;
 *   bbnc slot: counter (slot, 0x80000000 | feature, sweep & 0xffffffff, b);
 *   u_b from block b, words a = w0, b = w1: ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53, in (0, 1).
 * Every sum runs in a fixed order with no atomics on values: the same tables and seed give the same bits, so every rank of
 * a sharded sweep installs the same values after msc_state_commit_reduce without exchanging anything.  Both calls are
 * synchronous with ONE host synchronisation, and return MSC_EINVAL between msc_sweep_step_begin and
 * msc_state_commit_reduce.
 */
#define MSC_PRIOR_FLAT 0u
#define MSC_PRIOR_EXPONENTIAL 1u
#define MSC_PRIOR_NORMAL 2u
#define MSC_PRIOR_NONINF_BETA 3u
typedef struct {
  uint32_t feature;  /* state feature, or MSC_HP_CLUSTER */
  uint32_t coord;    /* float index in the feature's hp block; 0 for alpha */
  float width;       /* w > 0 */
  uint32_t prior;    /* MSC_PRIOR_* */
  float prior_a;     /* EXPONENTIAL: lambda > 0; NORMAL: mu */
  float prior_b;     /* NORMAL: sigma2 > 0 */
  uint32_t partner;  /* NONINF_BETA: the other coordinate of the feature */
} msc_slice_coord;
/*
 * One slice step of each of the n entries.  values_host[i] (nullable) = the value installed by entry i, evals_host[i]
 * (nullable) = the evaluations of the target its update took (the one at x0 included; none outside the support).  The
 * device hp, the host copy msc_state_get_hp reads, the score tables' staleness and alpha are left exactly as
 * msc_state_set_hp / msc_state_set_alpha would leave them.  MSC_EINVAL (nothing installed) for a width that is not a
 * positive finite float, a coordinate or partner outside the block, an unknown prior or a non-positive lambda / sigma2.
 */
int msc_hp_slice(msc_state *st, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev, uint64_t seed,
                 uint64_t sweep, float *values_host, uint32_t *evals_host);
/*
 * One slice step of the p of every counted slot of each of the n bbnc features (features[i], widths[i] > 0): p is written
 * into the slot's table and the feature's score tables go stale as after msc_state_set_ss (the next scoring call
 * rebuilds them); slots that are not counted are not touched.  evals_host[i] (nullable) = the evaluations over all of
 * feature i's slots.  MSC_EINVAL (nothing installed) for a feature that is not bbnc, twice in the call, or a bad width.
 */
int msc_theta_slice(msc_state *st, const uint32_t *features, const float *widths, uint32_t n, const uint8_t *slots_dev,
                    uint64_t seed, uint64_t sweep, uint64_t *evals_host);
/*
 * The slice step of EVERY chain of an ensemble (msc_chains_create, above; declared here because it takes
 * msc_slice_coord) in one launch: the other half of an iteration of the reference's runner (an assignment sweep, then
 * the hp kernel, on every chain).  msc_chains_hp_slice leaves chain c exactly where
 *   msc_hp_slice(state c, coords, n, the chain's mask, host_seeds[c], sweep, ...)
 * would: the same counters (target, entry, sweep, b) under the chain's key host_seeds[c] ^ the slice key, the same
 * arithmetic in the same order (one kernel body serves both calls), so the same bits in the installed values, in every
 * hp block and in alpha.  A grid of (targets x chains) workgroups takes the step; a second launch then rebuilds, for
 * every chain, what the step made stale -- the score tables of every feature from the new hp blocks and the CRP table
 * from the new alpha -- with the bits the per-state rebuild (the next call that scores that state) would have written,
 * so the next msc_chains_sweep / msc_chains_visit launches nothing before its kernel.
 *   coords, n     ONE list for all chains (their feature lists are equal by msc_chains_create); msc_hp_slice's entries
 *                 and msc_hp_slice's checks, made once, before anything is launched;
 *   slots_dev     nullable; uint8 masks of the counted slots on the device.  ld_slots == 0: one mask of ngroups bytes
 *                 for all chains; ld_slots >= ngroups: chain c's at slots_dev + c * ld_slots.  Null: every chain counts
 *                 its non-empty slots;
 *   host_seeds    uint64[nchains] on the host, read before the call returns;
 *   values_host, evals_host   nullable; [nchains][n] on the host, each chain's row in the caller's entry order: the
 *                 installed value and the evaluations of the target, as msc_hp_slice returns them.
 * ONE host synchronisation for the whole call, whatever the number of chains.  The tables of the call (per-chain
 * pointers and keys, per-chain targets, the entries) go through a device buffer the handle owns; it only grows, after a
 * wait for the stream, and the host image it is copied from is rewritten only by the next call, every return past the
 * copy having waited for the stream.  Every member's reference fields are made current before the launch.
 * A target that is not finite at its current value (msc_hp_slice's case): that entry of that chain keeps its value,
 * every other update of every chain is installed and book-kept, the rebuild runs, and the call returns MSC_EINVAL with
 * a message that names the chain, the feature and the coordinate (the lowest such chain's last such entry).
 * Errors, with nothing launched and nothing changed: MSC_EINVAL for a null argument, n == 0, ld_slots neither 0 nor >=
 * ngroups, whatever msc_hp_slice refuses of an entry, or a member between msc_sweep_step_begin and
 * msc_state_commit_reduce (the index is named); MSC_EUNSUPPORTED for a coordinate msc_hp_slice does not slice (dd
 * alphas, bnb r); MSC_EDEVICE when an earlier kernel reported an error.
 */
int msc_chains_hp_slice(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                        uint64_t ld_slots, const uint64_t *host_seeds, uint64_t sweep, float *values_host,
                        uint32_t *evals_host);

/* ---- the log joint log p(X, z | hp, alpha) of a state and of every chain; the best sample kept on the device ---- */
/*
 * What the reference's users plot to judge burn-in and rank samples by (score_assignment + the sum of score_likelihood,
 * entity_state.hpp:76-83), in double on the device.  A state's score is a row of nfeatures + 3 doubles, F = nfeatures:
 *   [0]      the total (((a + d_0) + d_1) + ... + d_{F-1}) + p, added in double in that written order
 *   [1]      a = score_assignment(alpha) = occ ln alpha + sum lgamma(n_k) + lgamma(alpha) - lgamma(N + alpha) of the device
 *            group counts, as msc_hp_grid_score's CRP grid and the slice step's alpha target write it
 *   [2 + f]  d_f = the sum over the counted slots k of score_data(hp_f, group k), the sum a slice target of feature f
 *            evaluates (counted: a non-zero group count, or with slots_dev a non-zero byte; no other slot is read)
 *   [2 + F]  p = the sum over the n entries of coords, in entry order from 0, of the entry's prior (MSC_PRIOR_*, as
 *            msc_hp_slice defines them) at the coordinate's CURRENT value (alpha, or a float of the device hp block;
 *            NONINF_BETA with its partner's current value); width is checked and not used; 0 when n == 0
 * The parts are kept apart so that a caller can plot the assignment term and the features' terms separately; adding
 * them up in the written order in double gives the bits of [0].
 * The order of the sums (one workgroup of 256 threads a state): a -- thread t adds lgamma(n_k), n_k and the occupied
 * slots over k = t, t + 256, ... ascending, the 256 partials fold in a tree (t += t + w, w = 128, ..., 1); d_f -- thread t
 * adds its counted slots k = t, t + 256, ... ascending, a wave of 64 folds by xor butterflies (32, ..., 1), the four waves
 * are added (w0 + w1) + (w2 + w3); p -- one thread.  No atomics: the order depends on ngroups and nothing else, a call
 * repeats its bits, and row c of msc_chains_score_joint equals msc_score_joint on member c bit for bit, whatever the
 * number of chains in the launch (one kernel body serves both calls).
 * noop contributes 0; bb, bbnc, bnb, gp, dd, dm and nich are supported (an ensemble holds neither bbnc nor dm).  bnb's
 * score_data is the marginal up to the data-only term sum_i log C(r + v_i - 1, v_i), as everywhere in this library (its
 * statistics cannot carry it): the same for every assignment, so traces, differences and ranks are unaffected.
 * MSC_EUNSUPPORTED for a state with a niw feature: the double evaluator these sums run through (the slice targets' and
 * the hp grids') has no niw.
 * Both calls are asynchronous on the context's stream and change nothing in any state: a sweep after a call gives the
 * bits it gives without it (the reference fields are made current first, as every call that reads them does).
 * msc_score_joint copies nothing: the entries travel as kernel arguments, 64 a launch.  msc_chains_score_joint uploads
 * one table (per-chain pointers and alpha) through a device buffer the handle owns, which only grows, after a wait for
 * the stream (once), out of the pinned areas msc_chains_sweep stages its table through; no other wait.
 *   coords, n     nullable with n == 0; else msc_hp_slice's entries and checks, made once before anything is launched;
 *   slots_dev     nullable; as msc_hp_slice / msc_chains_hp_slice (ld_slots == 0: one mask for all chains);
 *   out_dev       double[nfeatures + 3]; the chains' call: chain c's row at out_dev + c * ld_out, ld_out >= nfeatures + 3.
 * Errors, with nothing launched and nothing written: MSC_EINVAL for a null output, a null coords with n > 0, ld_out <
 * nfeatures + 3, ld_slots neither 0 nor >= ngroups, whatever msc_hp_slice refuses of an entry, or a state (a member:
 * the index is named) between msc_sweep_step_begin and msc_state_commit_reduce; MSC_EUNSUPPORTED for niw, and for an
 * entry msc_hp_slice does not slice; MSC_EDEVICE when an earlier kernel reported an error.
 */
int msc_score_joint(msc_state *st, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev, double *out_dev);
int msc_chains_score_joint(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, const uint8_t *slots_dev,
                           uint64_t ld_slots, double *out_dev, uint64_t ld_out);       /* ld_out >= nfeatures + 3 */
/*
 * The best sample of every chain so far, kept on the device: for every chain c with joint_dev[c * ld_joint] >
 * best_dev[c] -- strictly: a tie keeps the earlier sample, and a NaN never wins -- the chain's row z_dev + c * ld_z
 * (nrows int32) is copied over best_z_dev + c * ld_best, best_dev[c] takes the total and best_iter_dev[c] takes iter.
 * Start best_dev at -inf and best_iter_dev at -1.  A chain has one workgroup, which compares before it writes.
 * Asynchronous, no wait; no state is read or changed.  MSC_EINVAL (nothing launched) for a null argument, ld_joint < 1,
 * ld_z or ld_best < nrows, or an iter beyond int64; MSC_EDEVICE when an earlier kernel reported an error.
 */
int msc_chains_keep_best(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, const int32_t *z_dev, uint64_t ld_z,
                         uint64_t nrows, uint64_t iter, double *best_dev, int32_t *best_z_dev, uint64_t ld_best,
                         int64_t *best_iter_dev);

/* ---- tempered chains: the sweep at a temperature, replica exchange, and the weights of an annealing step ---- */
/*
 * msc_chains_sweep_tempered: msc_chains_sweep with chain c at its own temperature beta_dev[c], targeting
 *   pi_beta(z) ~ p(z | alpha) p(X | z, hp)^beta       (beta = 1: the posterior; 0: the CRP prior; > 1 sharpens).
 * Every argument but beta_dev is msc_chains_sweep's, with its layout, launch slicing, limits and errors.
 *   beta_dev      float[nchains] ON THE DEVICE, read by the kernel once per launch.  The call neither uploads nor reads
 *                 it and waits for nothing, so the temperatures msc_chains_exchange swapped on the stream are what the
 *                 next sweep reads.
 * A visit scores slot k as log pseudocount_k + beta * (the features' score_value sum): each of the sweep's partial sums
 * goes on by one fused multiply-add in the place and order of msc_chains_sweep's add, beta is not factored out, and so at
 * beta = 1 every bit -- z, tables, trace, occupied -- is msc_chains_sweep's.  At beta == 0 (-0.0f too) the score reads no
 * feature table and adds no partial (no 0 * -inf): the slot's score is the CRP term alone, while the row still leaves
 * and joins its groups' suff-stats; a sweep at beta = 0 from all-unassigned is a draw from the CRP prior.
 * A beta that is NaN, negative or infinite stops ITS chain for the launch: no visit, no sample written, z and tables as
 * they were; the other chains run, and the next call returns MSC_EDEVICE naming this one (detail: the chain).
 * Errors: MSC_EINVAL, with nothing launched, for a null beta_dev when nsweeps * nrows > 0, and whatever msc_chains_sweep
 * refuses.  There is no tempered msc_chains_visit: a visit's log predictive keeps its untempered meaning.
 */
int msc_chains_sweep_tempered(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                              uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order,
                              uint32_t nsweeps, const uint64_t *host_seeds, uint64_t sweep, const float *beta_dev,
                              uint32_t trace_every, int32_t *trace_dev, uint32_t *occupied_dev);

/*
 * The two steps a tempered ensemble makes BETWEEN its sweeps, chain c targeting pi_beta(z) at its own temperature beta_c.
 * Both calls read the chains' joint rows exactly as msc_chains_score_joint wrote them (chain c's at joint_dev + c *
 * ld_joint, ld_joint >= nfeatures + 3) and take from them the data log-likelihood
 *   L_c = ((d_0 + d_1) + ...) + d_{F-1},   the entries [2, 2 + F), added in double in that written order.
 * Both are asynchronous on the context's stream, wait for nothing, upload nothing and read or change no state.
 *
 * msc_chains_exchange: one step of replica exchange.  nchains must be a multiple of nrungs = R; ladder l owns chains [l R,
 * (l + 1) R).  rung_dev: int32[nchains], the rung each chain holds -- within a ladder a permutation of 0 .. R - 1;
 * beta_dev: float[nchains], the temperature each chain holds.  For every ladder and
 * every j < R - 1 with j % 2 == parity % 2, in ascending j, with a and b the chains that hold rungs j and j + 1:
 *   r = ((double)beta_a - (double)beta_b) * (L_b - L_a);   the swap is accepted when log(u) < r,
 *   u = the Philox uniform of (key seed, counter (l R + j, sweep)), msc_sweep_assign's generator.
 * A non-finite r (a NaN likelihood, inf - inf) rejects.  An accepted swap exchanges the two chains' entries of beta_dev
 * and of rung_dev: the TEMPERATURES move, the states stay where they are, so no table is touched and the sweep that
 * follows launches nothing before its kernel.  proposed_dev, accepted_dev: uint32[(nchains / R) (R - 1)], entry l (R - 1)
 * + j counts the pair (j, j + 1) of ladder l; both are ADDED to (the caller zeroes them).  One thread walks a ladder, so
 * the pairs of a ladder are decided one after another and a call repeats its bits.
 * Errors: MSC_EINVAL, with nothing launched, for a null argument, nrungs == 0, nchains % nrungs != 0 or ld_joint <
 * nfeatures + 3; MSC_EDEVICE when an earlier kernel reported an error.  A rung_dev that is no permutation within some
 * ladder leaves THAT ladder as it was (entries and counters) and surfaces as MSC_EDEVICE at the next call.
 *
 * msc_chains_anneal_weights: logw_dev[c] += ((double)beta_to_dev[c] - (double)beta_from_dev[c]) * L_c in double, one
 * thread per chain -- the weight of a step of annealed importance sampling.  Where beta_to == beta_from the entry is left
 * untouched (an infinite L_c does not turn it into NaN).  MSC_EINVAL for a null argument or ld_joint < nfeatures + 3.
 */
int msc_chains_exchange(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, uint32_t nrungs, float *beta_dev,
                        int32_t *rung_dev, uint64_t parity, uint64_t seed, uint64_t sweep, uint32_t *proposed_dev,
                        uint32_t *accepted_dev);
int msc_chains_anneal_weights(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, const float *beta_from_dev,
                              const float *beta_to_dev, double *logw_dev);

/* ---- posterior predictive sampling (group::sample_value, base.hpp:29) ---- */
#define MSC_PRED_MASKED_ONLY 0x1u /* draw masked entries only; observed ones are copied */
/*
 * Posterior predictive draws for rows [row0, row0+nrows) of the view (cols as in msc_score_value).
 * Groups:
 *   z_dev non-NULL (int32[nrows], indexed from row0): row r uses group z_dev[r] (in-sample imputation).  A row whose id
 *     is < 0 or >= ngroups is skipped: none of its outputs is written.
 *   z_dev NULL: every row's group is drawn as msc_sweep_assign draws an UNASSIGNED row -- its observed entries scored
 *     against the tables as they stand (no leave-one-out), plus log pseudocount, util::sample_discrete_log -- with the
 *     uniform Philox4x32-10(key = seed ^ 0xD1B54A32D192ED03, counter = (global row id, sweep)): a key no sweep with the
 *     same (seed, sweep) uses.
 *   z_out_dev (nullable, int32[nrows]) receives the group each row used.
 * Values: out_dev has one entry per state feature; out_dev[f] == NULL: feature f is not drawn, else it receives nrows x
 * count values of the type the kernels read for the family:
 *   bb / bbnc uint8 0|1, gp / bnb uint32, dd int32, nich float, niw float[dim] row-major.
 * Without MSC_PRED_MASKED_ONLY every entry is drawn from the posterior predictive of its row's group; with it only the
 * masked ones are, and observed entries are copied as the model's value type (the output is the completed column).  A niw
 * value with any masked element counts as missing and is drawn whole.
 * Draws (the predictives of the host sampler, include/microscopes_amd/hip_models.hpp detail::sampler): bb / bbnc / dd by inverse CDF of ONE
 * uniform, gp Gamma then Poisson, bnb Beta then Gamma then Poisson, nich Student-t, niw mu' + L z sqrt(dof / chi2).
 * Counters: the entry (global row id R = row_id0 + r, state feature f) reads the Philox4x32-10 blocks b = 0, 1, ... of
 *   key = seed, counter = (R & 0xffffffff, R >> 32, sweep & 0xffffffff, 0x80000000 | (f & 0x7fff) << 16 | b)
 * word by word (w0..w3 of block 0, then block 1, ...).  A one-uniform draw takes u = (w0 >> 8) * 2^-24 of block 0 and
 * picks the smallest value v whose predictive CDF exceeds u (bb: v = 1 iff u >= P(v = 0); dd: u * sum of weights
 * against the cumulative weights alpha_i + counts_i).  Every other uniform takes two consecutive words a, b:
 * u = ((a >> 5) * 2^26 + (b >> 6) + 0.5) * 2^-53; normals are Box-Muller pairs (r cos, r sin) of two such uniforms.
 * Sweeps' counters have a last word below 2^31, so no draw here shares one with a sweep; the sweep index enters mod 2^32.
 * The same arguments give the same bits, and the draws of a row do not depend on the rows around it (calls over row
 * ranges with matching row_id0 give the bits of one call over all of them).
 * The state is read-only: tables, counts, score tables, alpha and hp are left as they were.
 * MSC_EUNSUPPORTED for a dm (or noop) feature with a non-NULL output (upstream dm.cpp:100-111 throws), the state
 * untouched; MSC_EINVAL for bad arguments, a feature index >= 32768 drawn, and between msc_sweep_step_begin and
 * msc_state_commit_reduce.  Asynchronous on the context's stream.
 */
int msc_sample_predictive(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                          uint64_t row_id0, const int32_t *z_dev, int32_t *z_out_dev, uint32_t flags, uint64_t seed,
                          uint64_t sweep, void *const *out_dev);

/*
 * The log posterior predictive density of rows [row0, row0+nrows) under the state, reduced over the groups on chip:
 *   log p(x_r | state) = log sum_k pseudocount(k) / (n_r + alpha) * prod_f p_f(x_rf | group k).
 * For row r and slot k let t[r][k] be exactly what msc_score_value(st, view, cols, row0, nrows, z_dev,
 * MSC_SCORE_CRP_PRIOR, ...) defines: log pseudocount (empty slots share alpha) + the sum over features of score_value,
 * masked entries contributing nothing, leave-one-out when z_dev is given (int32[nrows], indexed from row0; an id < 0 or
 * >= ngroups is unassigned).  Then, indexed from row0,
 *   logp_dev[r]        = logsumexp_k t[r][k] - log(n_r + alpha), n_r = the sum of the group counts, minus one when the
 *                        row is assigned under leave-one-out.  With at least one empty slot this is the exact CRP
 *                        predictive; with every slot full it is the chain truncated to ngroups groups
 *                        (msc_sweep_sequential);
 *   map_dev[r]         (nullable) = the lowest k at which t[r][k] is the row's maximum: the hard (MAP) assignment;
 *   map_logresp_dev[r] (nullable) = t[r][map] - logsumexp_k t[r][k] (<= 0): the log responsibility of that group.
 * The [nrows, ngroups] matrix is never written where a fused kernel takes the state (a single nich feature up to 1024
 * groups; scalar features up to 256 groups on plans the plain tile kernel scores); every other state is scored chunk by
 * chunk into the state's scratch and reduced from there -- min(nrows, 4 GiB / row) x ngroups floats that stay allocated
 * with the state (the buffer msc_sweep_assign's materialised route uses).  All eight families and noop are taken.  flags is reserved: 0.
 * A row's results do not depend on the rows around it: a call over a sub-range gives the bits the whole call gives
 * for those rows (the kernels are chosen from the state and the view's rows, never the call's).
 * The state is read-only: tables, counts, alpha, hp, the sweeps' device (seed, sweep) pair and a captured step graph
 * are left as they were.  MSC_EINVAL for bad arguments and between msc_sweep_step_begin and msc_state_commit_reduce.
 * Asynchronous on the context's stream.  msc_last_kernel(3) names the kernel that reduced the rows.
 */
int msc_score_marginal(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                       const int32_t *z_dev, uint32_t flags, float *logp_dev, int32_t *map_dev, float *map_logresp_dev);

/* ---- per-value entry (the virtual group API, base.hpp:25-28) ----------- */
typedef enum msc_value_op {
  MSC_OP_ADD = 0, MSC_OP_REMOVE = 1, MSC_OP_SCORE_VALUE = 2, MSC_OP_SCORE_DATA = 3
} msc_value_op;
/*
 * One group, one value, evaluated on the device (a batch of one): host_hp and
 * host_ss as in msc_state_set_hp / set_ss, host_value one value of the family's
 * type.  ADD/REMOVE rewrite host_ss in place; SCORE_* write *score.  Synchronous;
 * latency-bound (one launch per call) -- the batched calls above are the fast path.
 */
int msc_value_op_single(msc_context *ctx, int family, uint32_t dim, int op, const float *host_hp,
                        void *host_ss, const void *host_value, float *score);

/* ---- relations (irm's per-cell data; relation/dataview.hpp:25-578) ------ */
/*
 * A relation reaches the kernels as a one-feature dataview whose rows are its
 * cells (dense: row-major order; compressed: the stored entries).  This turns the
 * per-dimension cluster assignments into the cell's block (= group) index:
 *   z_cell[c] = sum_d z_dev[d][index_d(c)] * prod_{e > d} ngroups[e]
 * (-1 when one of the cell's entities is unassigned).  positions_dev: null for a
 * dense relation, else uint32 [ncells][ndim] index tuples.  z_dev[d]: device int32
 * [shape[d]].  Asynchronous on the context's stream.
 */
int msc_relation_blocks(msc_context *ctx, uint32_t ndim, const uint64_t *shape,
                        const int32_t *const *z_dev, const uint32_t *ngroups,
                        const uint32_t *positions_dev, uint64_t ncells, int32_t *z_cell_dev);

/*
 * irm's slice reduction (what its assignment kernel does with relation::dataview::slice, dataview.hpp:265-578): entity e
 * of the domain on dimension `dim` is scored against every candidate cluster g of that domain by summing, over the
 * cells c of slice (dim, e), the cell's score against the block it would then lie in:
 *   out[e * ld_out + g] = sum_c scores[c * ld + g * cand_stride + off[c]]
 * scores_dev: the per-cell matrix msc_score_value wrote for the relation's cells ([ncells][ld], one column per block);
 * off_dev[c]: the block index of cell c with the candidate dimension's cluster set to 0 (msc_relation_blocks with an
 * all-zero assignment vector for `dim`; -1 = an entity of the cell is unassigned: the cell is skipped);
 * cand_stride: what one step of the candidate cluster adds to the block index (product of the cluster counts of the
 * later dimensions).  Dense relation: seg_dev = ids_dev = NULL and the slices are enumerated from shape; sparse: the
 * cells of entity e are ids_dev[seg_dev[e] .. seg_dev[e + 1]).  nent = entities scored (= shape[dim] for a dense one).
 * Sums are taken in double in a fixed order.  Asynchronous on the context's stream.
 */
int msc_relation_slice_scores(msc_context *ctx, const float *scores_dev, uint64_t ld, uint32_t ndim,
                              const uint64_t *shape, uint32_t dim, const uint32_t *seg_dev, const uint32_t *ids_dev,
                              const int32_t *off_dev, uint32_t ncand, uint32_t cand_stride, uint64_t nent,
                              float *out_dev, uint64_t ld_out);

/* ---- posterior co-clustering (z-)matrix (replaces microscopes.common.query.zmatrix) ---- */
/*
 * An accumulator of the co-clustering counts of m chosen rows over S assignment samples: C[a][b] = the number of
 * samples in which rows rows[a] and rows[b] share a label, and Z = C / S, the reference's zmatrix (query.py) restricted
 * to those rows.  The handle belongs to its context, as a view or a state does.
 * host_rows: m row indices into assignment vectors of n labels, in output order (repeats allowed, any order); NULL =
 * every row (m must equal n).  An entry >= n is MSC_EINVAL.  1 <= m <= 262144.  nlabels (the state's K): every label
 * must lie in [0, nlabels), 1 <= nlabels <= 65536.  Labels are packed 8 bits wide when nlabels <= 256, 16 bits otherwise.
 * Device footprint: the counts as upper-triangle tiles of 64 x 64 u32, 8 T (T + 1) KiB with T = ceil(m / 64) (m =
 * 16384: 514 MiB; m = 65536: 8 GiB), plus a batch of 64 T x 1 KiB (m = 16384: 16 MiB) and m u32 for the rows and as
 * many for an order: MSC_ENOMEM when that cannot be allocated.  Synchronous.
 */
typedef struct msc_zmatrix msc_zmatrix;
int msc_zmatrix_create(msc_context *ctx, uint64_t n, const uint32_t *host_rows, uint32_t m, uint32_t nlabels,
                       msc_zmatrix **out);
/*
 * Stage nsamples assignment vectors: sample s is z_dev[s * ld .. s * ld + n) (ld >= n), int32 labels.  Asynchronous on
 * the context's stream; the labels the matrix needs are packed before the call returns in stream order, so the caller
 * may overwrite z_dev with the next work it enqueues (the next msc_sweep_step, a replayed step graph included).  Samples
 * are gathered into a batch (1024 samples at 8 bits, 512 at 16) and the counts are updated when the batch fills; a call
 * larger than the space left spreads over several updates.  A label outside [0, nlabels) is never used as an address:
 * its sample adds nothing (it is still counted by msc_zmatrix_nsamples) and the failure surfaces as MSC_EDEVICE at the
 * next synchronising or launching call (reset the accumulator then).
 */
int msc_zmatrix_add(msc_zmatrix *zm, const int32_t *z_dev, uint32_t nsamples, uint64_t ld);
/* samples handed to msc_zmatrix_add since creation or the last reset (host bookkeeping, no synchronisation) */
int msc_zmatrix_nsamples(const msc_zmatrix *zm, uint64_t *out);
/*
 * Update the counts with the staged samples, then write the full symmetric m x m matrix into out_dev (row a at
 * out_dev + a * ld_out, ld_out >= m): msc_zmatrix_counts the exact u32 counts C, msc_zmatrix_result float(C) / float(S)
 * with IEEE division (for S < 2^24 bit for bit the reference's float32 sum of ones divided by float(S)).  host_order
 * (nullable): a permutation of [0, m); the matrix is written reordered, out[a][b] = Z[order[a]][order[b]] (MSC_EINVAL
 * when it is not a permutation).  msc_zmatrix_result with no sample is MSC_EINVAL (the reference raises on an empty
 * list).  Asynchronous on the context's stream; host_order is read before the call returns.
 */
int msc_zmatrix_counts(msc_zmatrix *zm, const uint32_t *host_order, uint32_t *out_dev, uint64_t ld_out);
int msc_zmatrix_result(msc_zmatrix *zm, const uint32_t *host_order, float *out_dev, uint64_t ld_out);
/*
 * Candidate partitions scored against the counts: the sums behind a decision-theoretic point estimate (Binder's loss,
 * i.e. Dahl's least squares, and Wade & Ghahramani's lower bound on the variation of information).  With C what
 * msc_zmatrix_counts writes (no order) and V = C[0][0], the valid samples, a candidate c is an assignment vector of n
 * int32 labels laid out as for msc_zmatrix_add (candidate c at cand_dev + c * ld, ld >= n); position a carries
 * l_c(a) = cand[c][rows[a]].  Only equality of labels is used: any int32 value is a label and there is no range check.
 *   size_c[a] = #{ b < m : l_c(b) == l_c(a) }   (b = a included)
 *   w_c[a]    = the sum of C[a][b] over those b  (>= V)
 *   binder_num[c] = T + V P_c - 2 Q_c,  P_c = sum_a (size_c[a] - 1) / 2,  Q_c = sum_a (w_c[a] - V) / 2,
 *                   T = sum_{a<b} C[a][b]:  V * sum_{a<b} |[l_c(a) == l_c(b)] - C[a][b] / V|, an exact int64 >= 0;
 *                   binder_num / V is the posterior expected number of mis-paired pairs, and Dahl's
 *                   sum_{a<b} ([..] - Z)^2 differs from it by a term that does not depend on c (same argmin)
 *   vi_lb[c]      = (1 / m) sum_a (log2 size_c[a] - 2 log2 w_c[a]) + 2 log2 V  in float64: the lower bound on the
 *                   expected VI less its candidate-independent term (1 / m) sum_a E[log2 size_sample(a)], which the
 *                   counts do not determine; 0 for all singletons.  The sum runs in a fixed order: the same arguments
 *                   give the same bits.
 * Both calls first update the counts with the staged samples (as msc_zmatrix_counts does) and otherwise leave the
 * accumulator as it was; both are asynchronous on the context's stream.  Outputs are device pointers, each nullable:
 * w_dev [ncand][m] uint64 and size_dev [ncand][m] uint32; binder_num_dev [ncand], vi_lb_dev [ncand], valid_dev [1] (V).
 * Every sum is an exact integer for every m and number of samples the accumulator takes.  Candidates are processed a
 * chunk at a time over buffers the accumulator owns, allocated at the first call: a chunk of 64 .. 512 candidates (8 Mi
 * labels over 64 ceil(m / 64), rounded down to 64) holds chunk x 64 ceil(m / 64) int32 labels and, for
 * msc_zmatrix_partition_loss, chunk x m x 12 bytes of sums (m = 16384: 32 MiB + 96 MiB).  MSC_EINVAL: no sample yet,
 * ncand == 0, ld < n, a null handle or a null cand_dev.  msc_zmatrix_partition_loss returns MSC_EUNSUPPORTED, before
 * anything is launched, when m (m - 1) / 2 x nsamples does not fit 63 bits.  msc_last_kernel(2) names the
 * instantiation of the sums kernel (packed 24 + 8 bit partial sums while nsamples < 2^20, 64-bit sums after).
 */
int msc_zmatrix_partition_sums(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t ncand, uint64_t ld,
                               uint64_t *w_dev, uint32_t *size_dev);
int msc_zmatrix_partition_loss(msc_zmatrix *zm, const int32_t *cand_dev, uint32_t ncand, uint64_t ld,
                               int64_t *binder_num_dev, double *vi_lb_dev, uint64_t *valid_dev);
/*
 * Greedy refinement of partitions under Binder's loss: from each start, rows move one at a time to the cluster (or to a
 * new one) that lowers binder_num most, sweep after sweep, until a sweep moves nothing.  With C, V and the layout of a
 * candidate as above, a start is start_dev + s * ld (ld >= n), position a carrying start[s][rows[a]]; only equality of
 * labels is used.  The rule (the device and common_amd.query's host path implement exactly this; all integer):
 *   ids      a start's labels over the positions are renumbered from 0 in the order of each label's first position;
 *            1 <= max_clusters <= m is the id capacity and n_k the number of positions with id k.
 *   a sweep  visits the positions in ascending order, or in host_order (nullable: a permutation of [0, m), read before
 *            the call returns).  For position a with id c:  n'_k = n_k - [k == c],  s_k = the sum of C[a][b] over the
 *            b != a with id k (uint64),  g_k = 2 s_k - V n'_k (int64) for every k with n'_k > 0,  g_cur = g_c if
 *            n'_c > 0 and 0 otherwise (a is alone already).
 *   target   (1) the existing cluster k (n'_k > 0) of the largest g_k, the lowest id among equals, if g_k > g_cur
 *            strictly: gain g_k;  (2) else, if n'_c > 0, 0 > g_cur and some id f < max_clusters has n_f == 0, a moves
 *            alone into the lowest such f: gain 0;  (3) else a stays.  Ties keep a row where it is, and an existing
 *            cluster is preferred to a new one at equal gain.
 *   a move   lowers binder_num by exactly gain - g_cur > 0, so the process ends.  Sweeps repeat until one makes no move
 *            or max_sweeps have run (0 is allowed: the outputs describe the start).
 * Outputs, device pointers, each nullable: labels_dev [nstarts][m] int32 over the positions, numbered from 0 in the order
 * of first position; binder_num_dev [nstarts], the start's value less the decreases (what msc_zmatrix_partition_loss
 * gives for the output labels); sweeps_dev [nstarts], the sweeps run, the last one that moved nothing included;
 * moves_dev [nstarts], all moves.  Starts are independent: any split of them over calls gives the same outputs.
 * Like msc_zmatrix_partition_loss the call first updates the counts with the staged samples, otherwise leaves the
 * accumulator as it was, and is asynchronous on the context's stream: one launch per sweep (one workgroup per start; a
 * start that has converged returns at once) with no wait in between up to 64 sweeps; beyond 64 the host waits once per
 * 64 further sweeps to see whether any start still moves.  Caps: m <= 32768 and max_clusters <= 1024 (16-bit ids, sizes
 * and bins of s_k in LDS); beyond them MSC_EUNSUPPORTED before anything is launched, as when m (m - 1) / 2 x
 * nsamples does not fit 63 bits.  MSC_EINVAL: no sample yet, nstarts == 0, ld < n, a null handle or start_dev,
 * host_order not a permutation, max_clusters 0 or above m.  A start with more than max_clusters clusters is found on
 * the device after the gather: it is not refined, its outputs mean nothing, and the failure surfaces as MSC_EDEVICE at
 * the next synchronising or launching call (the accumulator itself stays good).  Workspaces the accumulator owns,
 * allocated at the first call, beside those of msc_zmatrix_partition_loss: a dense copy of the counts, m x 4 ceil(m / 4)
 * u32 (m = 16384: 1 GiB; m = 32768: 4 GiB), written once per call, and chunk x 4 ceil(m / 4) 16-bit ids: MSC_ENOMEM
 * when they cannot be allocated.  msc_last_kernel(2) names the instantiation of the sweep kernel (its LDS id capacity, the 16-byte loads a thread has in
 * flight, and whether nsamples x m < 2^32 let it keep s_k in 32-bit bins instead of 64-bit ones).
 * The variation-of-information bound is not refined: its gains are floats, and a tie decided in the last ulp would
 * change the trajectory.
 */
int msc_zmatrix_partition_refine(msc_zmatrix *zm, const int32_t *start_dev, uint32_t nstarts, uint64_t ld,
                                 uint32_t max_sweeps, uint32_t max_clusters, const uint32_t *host_order,
                                 int32_t *labels_dev, int64_t *binder_num_dev, uint32_t *sweeps_dev, uint64_t *moves_dev);
/* zero the counts and drop the staged samples (asynchronous); destroy frees everything the accumulator allocated */
int msc_zmatrix_reset(msc_zmatrix *zm);
int msc_zmatrix_destroy(msc_zmatrix *zm);

/* ---- single linkage of a z-matrix (replaces scipy's linkage in microscopes.common.query.zmatrix_heuristic_block_ordering) ---- */
/*
 * scipy.cluster.hierarchy.linkage(y, 'single') and leaves_list of it, for y the condensed distances 1 - Z of a dense
 * float32 matrix on the device: z_dev[i * ld + j], 0 <= i, j < n, ld >= n (read only; a row of a strided view may start
 * at any multiple of 4 bytes).  When z_dev and ld * 4 are multiples of 16 (of 8 for 1024 < n <= 2048) a row of n > 1024
 * is read 16 (8) bytes a lane: up to 3 floats past column n - 1, inside the row's ld floats, which must then be readable
 * in the last row too; their values are never used.  Otherwise one float at a time and nothing outside columns [0, n).
 * The distance of i and j is 1.0f - Z[i][j] in float, as the reference forms it, widened to double in the output.
 * Tie rule (it decides the tree: a z-matrix holds multiples of 1 / S): Prim's chain from point 0; every step moves to the
 * unmerged point of the lowest (distance so far, index) in lexicographic order, i.e. the lowest index among equal
 * distances; the n - 1 edges are then sorted by distance with a stable sort and relabelled by union-find, row i joining
 * (min(root, root), max(root, root)) into node n + i.  Bit for bit scipy's matrix and scipy's leaf order (pre-order from
 * node 2 n - 2, column 0 first) whenever every distance is finite.
 * Precondition: Z is symmetric.  Step x reads row x alone, never column x, and the diagonal's value is never used (it may
 * hold anything, NaN included).  A caller whose matrix is not symmetric passes a symmetrised copy (common_amd.query does).
 * host_linkage (nullable): [n - 1][4] doubles (node, node, distance, size).  host_order (nullable): the n leaves.
 * The chain runs in ONE workgroup whose threads hold its n distances in registers (msc_last_kernel(2) names the
 * instantiation: columns a thread, wide loads or not): n <= 65536, MSC_EUNSUPPORTED above, before anything is launched.
 * MSC_EINVAL for n < 2, ld < n, a null z_dev, or flags != 0 (none is defined).  Synchronous: the kernel, a copy of the
 * 3 (n - 1) edge values, then the sort and the relabelling on the host.
 */
int msc_linkage_single(msc_context *ctx, const float *z_dev, uint64_t ld, uint32_t n, uint32_t flags,
                       double *host_linkage, uint32_t *host_order);

/* ---- distances between partitions: what the exact expected VI, credible balls and the adjusted Rand index are made of ---- */
/*
 * Every partition of one set against every partition of another.  Partition i of a is a_dev + i * lda, partition j of b is
 * b_dev + j * ldb (lda, ldb >= m): int32 labels of the same m rows; only equality of labels is used, any int32 value is a
 * label.  b_dev == NULL: a against itself (ldb and nb are ignored, nb = na, and the b outputs repeat the a outputs).
 * For partitions a and b write n_ij for the contingency counts (rows with label i in a and label j in b), a_i and b_j for
 * the cluster sizes, C(n, 2) = n (n - 1) / 2.  The call writes
 *   pairs_ab = sum_ij C(n_ij, 2),  pairs_a = sum_i C(a_i, 2),  pairs_b likewise            exact int64
 *   nlogn_ab = sum_ij n_ij log2 n_ij,  nlogn_a = sum_i a_i log2 a_i,  nlogn_b likewise     float64
 *   nclusters_a, nclusters_b                                                               the numbers of clusters
 * from which (common_amd.query does this arithmetic)
 *   binder(a, b) = pairs_a + pairs_b - 2 pairs_ab: the row pairs that one partition joins and the other separates, an
 *                  exact integer;
 *   vi(a, b)     = (nlogn_a + nlogn_b - 2 nlogn_ab) / m: the variation of information in bits, a metric, 0 iff a = b;
 *   ari(a, b)    = (pairs_ab - E) / ((pairs_a + pairs_b) / 2 - E),  E = pairs_a pairs_b / C(m, 2), in float64 from the
 *                  integers, defined as 1.0 where the denominator is 0.
 * With n(r) the count of row r's own cell, sum_r (n(r) - 1) = 2 pairs_ab and sum_r log2 n(r) = nlogn_ab: the kernel counts
 * the rows into a table, lets every row read its own cell back and never walks the cells.  nlogn_ab is that sum of m terms
 * log2 n(r) (each within an ulp), in an order and a reduction tree that m alone fixes: the same arguments give the same
 * bits; any split of a or of b over calls gives the same bits; (a, b) and (b, a) give the same bits; and so do the two
 * places the table may live in (LDS while K_a K_b <= 15360 cells, else a global workspace; msc_last_kernel(2) names the
 * pair kernel that ran last: threads, steps of four rows a thread, LDS or not).  nlogn_a is summed over the clusters in
 * the order of their first rows.
 * Outputs are device pointers: pairs_ab_dev, nlogn_ab_dev [na][nb] (either may be NULL; both NULL: no pair is computed);
 * pairs_a_dev, nlogn_a_dev, nclusters_a_dev [na] and the same three for b [nb], each nullable.
 * Caps: m <= 32768, MSC_EUNSUPPORTED above, before anything is launched; at most 1024 clusters a partition.  A partition
 * with more is found on the device: every output it takes part in is written as -1 (uint32: all ones) or NaN and the
 * failure surfaces as MSC_EDEVICE at the next synchronising or launching call.  MSC_EINVAL: a null ctx or a_dev, na, nb or
 * m equal to 0, lda or ldb below m, flags != 0 (none is defined).
 * The outputs are written asynchronously on the context's stream.  Partitions are taken 256 of a against 256 of b at a
 * time; the host waits once for the cluster counts of each chunk (4 bytes a partition), which say which of the two
 * kernels a block needs.  Workspaces the context owns, allocated at first use and kept: 2 x 256 x 4 ceil(m / 4) 16-bit
 * ids, m + 1 doubles of log2 n, and -- from the first pair that does not fit LDS -- 128 tables of 4 MiB, zeroed once
 * (the kernel leaves them zero).  MSC_ENOMEM when they cannot be allocated.
 */
int msc_partition_distances(msc_context *ctx, const int32_t *a_dev, uint64_t lda, uint32_t na,
                            const int32_t *b_dev, uint64_t ldb, uint32_t nb, uint32_t m, uint32_t flags,
                            int64_t *pairs_ab_dev, double *nlogn_ab_dev,
                            int64_t *pairs_a_dev, double *nlogn_a_dev, uint32_t *nclusters_a_dev,
                            int64_t *pairs_b_dev, double *nlogn_b_dev, uint32_t *nclusters_b_dev);

/* ---- greedy refinement of partitions under the exact posterior expected variation of information ---- */
/*
 * msc_vi_table: F[0..m] on the host, F(0) = 0 and F(n) = rint(n log2(n) 2^24) for 1 <= n <= m, computed in double.  It
 * needs no context and no device.  Everything that needs the table -- the kernels below, common_amd.query's host path --
 * takes it from this one function, so no libm difference can separate the two.  G(n) = F(n + 1) - F(n), 0 <= n < m.
 * MSC_EINVAL: host_F null.
 *
 * msc_partition_refine_vi: from each start, rows move one at a time to the cluster (or to a new one) that lowers the
 * posterior expected VI most, sweep after sweep, until a sweep moves nothing.  Sample s is samples_dev + s * lds, a start
 * is start_dev + i * ld (lds, ld >= m): int32 labels of the same m rows; any int32 value is a label and only equality is
 * used.  The rule (the device and common_amd.query's host path implement exactly this; all integer):
 *   objective  a partition c has sizes n_k; n^s_{k,l} counts the rows with id k in c and label l in sample s;
 *              J(c) = S sum_k F(n_k) - 2 sum_s sum_{k,l} F(n^s_{k,l}).  J / (S m 2^24) is the posterior expected VI in
 *              bits less its candidate-independent term, up to the table's rounding.  J is never formed, only differences.
 *   ids        a start's labels are renumbered from 0 in the order of each label's first row; 1 <= max_clusters <= m is
 *              the id capacity.
 *   a sweep    visits the rows in ascending order, or in host_order (nullable: a permutation of [0, m), read before the
 *              call returns).  For row a with id c and sample labels l_s:
 *              (1) take a out: n'_k = n_k - [k == c], and n'^s likewise;
 *              (2) for every k with n'_k > 0:  D_k = S G(n'_k) - 2 sum_s G(n'^s_{k, l_s}), an int64: J with a in k is J
 *                  without a, plus D_k;
 *              (3) D_cur = D_c if n'_c > 0, else 0 (a is alone already);
 *              (4) the target is the existing cluster (n'_k > 0) of the smallest D_k, the lowest id among equals;
 *              (5) a new cluster is taken instead in one case only, when all three hold: n'_c > 0; some id below
 *                  max_clusters is empty; and that smallest D_k is strictly above 0.  Then a goes alone into the lowest
 *                  empty id, with D = 0.  An existing cluster is preferred to a new one at equal D;
 *              (6) a moves only if the target's D is strictly below D_cur; otherwise a stays;
 *              (7) a move lowers J by exactly D_cur - D_target > 0, so the process ends, and the running int64
 *                  `decrease` needs no second pass.
 *   Sweeps repeat until one moves nothing or max_sweeps have run (0 is allowed: the outputs describe the start).
 *   widths     G < 17 2^24 for m <= 32768, |D| <= 3 S G_max and decrease <= 2 S F(m): under 2^62 within the caps.  The
 *              host checks these bounds before any launch: MSC_EUNSUPPORTED if they fail.
 * Outputs, device pointers, each nullable (all null: nothing is done): labels_dev [nstarts][m] int32, numbered from 0 in
 * the order of first row; decrease_dev [nstarts], J of the start less J of the output; sweeps_dev [nstarts], the sweeps
 * run, the last one that moved nothing included; moves_dev [nstarts], all moves.  Starts are independent: any split of
 * them over calls, and any workspace_bytes, gives the same outputs.
 * The call is asynchronous on the context's stream but for one wait: the samples are canonicalised first (16-bit ids by
 * first row, their cluster counts L_s) and the host waits for the sum of the L_s, which sizes the cells; max_sweeps == 0
 * does not need them and waits for nothing.  Then, a chunk of starts at a time: the starts' ids, their contingency cells
 * (u16, sum L_s x max_clusters rounded up to 32 a start, in blocks of 32 ids so that the ids in use lie together; counted
 * once), one launch per sweep (one workgroup per start; a
 * start that has converged returns at once) with no wait in between up to 64 sweeps; beyond 64 the host waits once per
 * 64 further sweeps to see whether any start still moves.  msc_last_kernel(2) names the sweep kernel's instantiation.
 * workspace_bytes (0: 2 GiB) bounds the cells of one chunk; a single start whose cells do not fit returns
 * MSC_EUNSUPPORTED, naming the bytes it needs, with no output written.
 * Caps: m <= 32768, nsamples <= 65536, max_clusters <= 1024: MSC_EUNSUPPORTED before anything is launched.  At most 1024
 * clusters a sample, max_clusters a start: one with more is found on the device after canonicalisation; such a start is
 * not refined, the outputs of a call with such a sample mean nothing, and the failure surfaces as MSC_EDEVICE at the next
 * synchronising or launching call (the context stays good).  MSC_EINVAL: a null ctx, samples_dev or start_dev; nsamples,
 * nstarts or m equal to 0; lds or ld below m; host_order not a permutation; max_clusters 0 or above m; flags != 0 (none is
 * defined).  Workspaces the context owns, allocated at first use and kept: the samples' ids (S x 4 ceil(m / 4) x 2 bytes),
 * the rows' stretch indices (m x S x 4 bytes), G (m x 8 bytes), and a chunk's ids, totals and cells: MSC_ENOMEM when they
 * cannot be allocated.
 */
int msc_vi_table(uint32_t m, int64_t *host_F);
int msc_partition_refine_vi(msc_context *ctx, const int32_t *samples_dev, uint64_t lds, uint32_t nsamples, uint32_t m,
                            const int32_t *start_dev, uint64_t ld, uint32_t nstarts,
                            uint32_t max_sweeps, uint32_t max_clusters, const uint32_t *host_order,
                            size_t workspace_bytes, uint32_t flags,
                            int32_t *labels_dev, int64_t *decrease_dev, uint32_t *sweeps_dev, uint64_t *moves_dev);

#ifdef __cplusplus
}
#endif
#endif /* MICROSCOPES_HIP_H */
