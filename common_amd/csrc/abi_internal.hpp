// abi_internal.hpp -- the seam between the core of the C ABI's host side (abi.cpp: context, dataviews, the state, its
// plan and tables, score and sweep) and the units that hold one subsystem each (blocked.cpp, chains.cpp, hyper.cpp,
// predict.cpp, summary.cpp): the environment switches, and the core's helpers that such a unit calls.  abi.cpp defines
// them; a helper that only abi.cpp uses is static there and is not listed.  Last, the slice step's host side, which
// hyper.cpp defines and chains.cpp shares.  No object with state lives here.
#pragma once

#include <cstdlib>
#include <vector>

#include "joint_math.hpp"
#include "msc_internal.hpp"

namespace msc {

// the environment's switches (route.hpp Switches), read afresh by every call that plans, routes or allocates
inline Switches read_switches() {
  Switches sw;
  if (const char *e = std::getenv("MSC_TAIL_MIN_ROWS")) sw.tail_forced = true, sw.tail_min_rows = (uint64_t)std::atoll(e);
  sw.no_narrow_tail = std::getenv("MSC_NO_NARROW_TAIL") != nullptr, sw.no_bb_fuse = std::getenv("MSC_NO_BB_FUSE") != nullptr;
  if (const char *e = std::getenv("MSC_LOO_LDS")) sw.loo_lds = std::atoi(e);
  if (const char *e = std::getenv("MSC_SWEEP_NICH1")) sw.sweep_nich1 = std::atoi(e);
  if (const char *e = std::getenv("MSC_MARGINAL_TILE")) sw.marginal_tile = std::atoi(e);
  if (const char *g = std::getenv("MSC_SWEEP_GRAPH")) sw.sweep_graph = g[0] != '0' && g[0] != 0;
  if (const char *e = std::getenv("MSC_ALLOC_CANDIDATES")) sw.alloc_candidates = std::atoi(e);
  if (const char *e = std::getenv("MSC_ALLOC_ACCEPT_GBPS")) sw.alloc_accept_gbps = (float)std::atof(e);
  return sw;
}

// count elements (at least one), zero-filled
template <typename T>
int alloc_zeroed(DevBuf<T> &buf, size_t count) {
  MSC_HIP(buf.alloc(count, 1));
  MSC_HIP(hipMemset(buf, 0, std::max<size_t>(count, 1) * sizeof(T)));
  return MSC_OK;
}

// ---- what abi.cpp defines (each is described where it is defined) ------------------------------------------------------
// Hidden: the library does not export them, and a unit's call is a direct one, as it was when all of this was one file
// (msc_chains_visit makes a dozen of them per member state and call).
#pragma GCC visibility push(hidden)
int device_error_check(msc_context *ctx);
int refuse_mid_step(const msc_state *st, const char *entry);
bool refresh_alpha_sum(msc_state *st, uint32_t feature);
int bind_view(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows);
const RouteFacts &route_facts_now(msc_state *st);   // what a unit hands the routes of route.hpp / route_calls.hpp

uint32_t prepare_value_slices(const msc_state *st);
int ensure_raw(msc_state *st);
int ensure_derived(msc_state *st);
int ensure_crp(msc_state *st);
int ensure_additive(msc_state *st);
int ensure_all_current(msc_state *st);

int refresh_fused_tables(msc_state *st);
int run_loo_own(msc_state *st, uint64_t row0, uint64_t nrows, const int32_t *z, bool crp);
int run_score(msc_state *st, uint64_t row0, uint64_t nrows, const int32_t *z_dev, bool crp, bool niw_f32, float *out_dev,
              uint64_t ld_out);

// internal flags of accumulate_impl, next to the public MSC_ACC_*: the additive tables are already zero (a fused
// sweep kernel did it); commit and prepare in one launch, which also moves the random stream on (msc_sweep_step)
enum : uint32_t { kAccZeroed = 0x100, kAccThenPrepare = 0x200 };
int commit(msc_state *st);
int accumulate_impl(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                    const int32_t *z_dev, uint32_t flags);

int sweep_assign_impl(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t row0, uint64_t nrows,
                      uint64_t row_id0, int32_t *z_dev, uint64_t seed, uint64_t sweep, bool *zeroed = nullptr);

// ---- what hyper.cpp defines: the slice step's host side, shared by msc_hp_slice and msc_chains_hp_slice (chains.cpp) ----
constexpr uint64_t kSliceKey = 0x2545F4914F6CDD1Dull;   // the slice steps' key is seed ^ this
void hp_installed(msc_state *st, uint32_t feature, const float *blk);
void alpha_installed(msc_state *st, float alpha);
// a checked call's targets (tslot: the feature, or nfeat for alpha) and their entries in device order
struct SlicePlan {
  std::vector<uint32_t> tslot, first, count;   // per target: entries [first, first + count) of dc
  std::vector<SliceCoord> dc;                  // per entry, targets one after the other
  std::vector<uint32_t> caller;                // device entry -> the caller's index
  uint32_t ntargets() const { return (uint32_t)tslot.size(); }
  uint32_t n() const { return (uint32_t)dc.size(); }
};
int slice_plan(const msc_state *st, const msc_slice_coord *coords, uint32_t n, SlicePlan &plan);
void slice_targets(const msc_state *st, const SlicePlan &plan, SliceTarget *targets);
int slice_installed(msc_state *st, const SlicePlan &plan, const msc_slice_coord *coords, const float *val, const uint32_t *ev,
                    const uint32_t *stat, float *values_host, uint32_t *evals_host, int64_t chain);
// the joint score's checks of a state's features and of the call's entries (msc_hp_slice's), and the entries as the
// kernels take them, in the caller's order; shared by msc_score_joint and msc_chains_score_joint (chains.cpp)
int joint_entries(const msc_state *st, const char *who, const msc_slice_coord *coords, uint32_t n,
                  std::vector<JointCoord> &entries);
// ---- what blocked.cpp defines for msc_chains_split_merge (chains.cpp): the move's route for a member, and the member's
// pair state as the pair half of its table entry (launchers.hpp SmChain) ----
struct SmChain;
int sm_chain_route(msc_state *st);
int sm_chain_pair(msc_state *st, const msc_dataview *view, const uint32_t *cols, uint64_t nrows, SmChain *entry);
#pragma GCC visibility pop

}  // namespace msc
