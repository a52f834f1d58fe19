// step_rules.hpp -- the host bookkeeping of the sweep step (abi.cpp msc_sweep_step and the calls beside it): what the host
// believes the device's (seed, sweep) pair holds, and when a step is run, counted, replayed or captured.  Host only:
// standard headers alone, builds with the plain host compiler (tests/cxx/test_step_rules.cpp).
#pragma once

#include <cstdint>
#include <vector>

namespace msc {

// The sampling kernels read (seed, sweep) from a pair on the device (msc_state::rng_dev) and a step ends by incrementing
// the sweep index there; RngMirror is the one owner of what the host believes that pair holds.  Callers report the
// EVENTS below, after the launch that makes them true was enqueued, and never write a field:
//
//   event                   valid   seed   sweep        owed   who reports it
//   set(seed, sweep)        1       seed   sweep        .      k_rng_set enqueued: sweep_assign_impl, msc_sample_predictive
//   advanced()              .       .      + 1          .      k_rng_bump enqueued: a plain sweep_assign_impl, a replayed graph
//   tail_owes()             0       .      .            .      msc_sweep_step's eager step, before its accumulate
//   tail_paid()             1       .      + 1          .      ... after it (the accumulate's tail moved the pair on)
//   deferred()              0       .      .            1      msc_sweep_step_begin (next = sweep + 1)
//   deferred_paid()         1       .      next         0      msc_state_commit_reduce, when owed
//   invalidate()            0       .      .            .      msc_sample_predictive, after its borrowed draw
//
//   ("." = left as it is.)  A step that fails between tail_owes and tail_paid, or between deferred and deferred_paid,
//   leaves the mirror invalid: the next sweep sets the pair afresh.
class RngMirror {
 public:
  // ---- queries ----
  bool holds(uint64_t seed, uint64_t sweep) const { return valid_ && seed_ == seed && sweep_ == sweep; }
  bool valid() const { return valid_; }
  uint64_t seed() const { return seed_; }     // (what the pair held when last valid: for putting a borrowed pair back)
  uint64_t sweep() const { return sweep_; }
  // between msc_sweep_step_begin and msc_state_commit_reduce: the additive tables hold one rank's uncommitted sums
  bool mid_step() const { return owed_; }

  // ---- events ----
  void set(uint64_t seed, uint64_t sweep) {
    valid_ = true;
    seed_ = seed;
    sweep_ = sweep;
  }
  void advanced() { sweep_++; }
  void tail_owes() { valid_ = false; }
  void tail_paid() {
    valid_ = true;
    sweep_++;
  }
  void deferred() {
    valid_ = false;
    owed_ = true;
    next_ = sweep_ + 1;
  }
  void deferred_paid() {
    owed_ = false;
    valid_ = true;
    sweep_ = next_;
  }
  void invalidate() { valid_ = false; }

  // the mirror as a value (a step recorded for a graph has not run; a borrowed pair is put back)
  RngMirror snapshot() const { return *this; }
  void restore(const RngMirror &s) { *this = s; }
  bool operator==(const RngMirror &o) const {
    return valid_ == o.valid_ && owed_ == o.owed_ && seed_ == o.seed_ && sweep_ == o.sweep_ && next_ == o.next_;
  }
  bool operator!=(const RngMirror &o) const { return !(*this == o); }

 private:
  uint64_t seed_ = 0, sweep_ = 0, next_ = 0;
  bool valid_ = false, owed_ = false;
};

// ---- the step graph ----
// The steady state of msc_sweep_step -- same view, rows and assignment vector, consecutive sweep indices -- is captured
// once as a HIP graph and replayed.  What "same" means:
struct StepKey {
  const void *view = nullptr, *z = nullptr;
  uint64_t view_serial = 0, row0 = 0, nrows = 0, row_id0 = 0;
  float alpha = 0.f;
  std::vector<uint32_t> cols;
  bool operator==(const StepKey &o) const {
    return view == o.view && view_serial == o.view_serial && row0 == o.row0 && nrows == o.nrows && row_id0 == o.row_id0 &&
           z == o.z && alpha == o.alpha && cols == o.cols;
  }
};

enum class StepAction {
  eager,     // run the step as it is; nothing of the graph's bookkeeping moves
  rekey,     // a new key: drop the executable, take the key, seen = 0 -- then as `count`
  count,     // seen++ and run eagerly
  replay,    // launch the executable (it ends with k_rng_bump: the mirror has advanced(); the flags end as they began)
  capture,   // record the eager step, instantiate and launch it; a failure sets `disabled`, puts flags and mirror back
             // and runs eagerly
};

struct StepInputs {
  bool graph_on = false;      // the MSC_SWEEP_GRAPH switch
  bool disabled = false;      // a capture failed on this state before
  bool has_exec = false;      // an executable exists
  bool same_key = false;      // ... and this step's key equals the one it was captured (or is being counted) under
  bool holds = false;         // RngMirror::holds(seed, sweep): the device's pair is already this step's
  bool flags_equal = false;   // the validity flags at entry equal those the executable was captured under
  int seen = 0;               // eager steps counted under the key so far
  bool fused = false;         // the route is the fused kind (nothing in it allocates, copies to the host or waits)
};

// (a step of no rows never gets here: it is the resetting accumulate.)  With the switch off or after a failed capture the
// rule reads nothing but those two.  The first two steps under a key run eagerly -- allocations, bindings and first-use
// setup happen there and the state reaches its steady flags -- and the third is captured.  An executable that cannot be
// replayed this time (another pair, other flags) is kept: the step after may be its steady state again.
inline StepAction step_action(const StepInputs &in) {
  if (!in.graph_on || in.disabled) return StepAction::eager;
  if (!in.same_key) return StepAction::rekey;
  if (in.has_exec) return in.holds && in.flags_equal ? StepAction::replay : StepAction::eager;
  if (in.seen < 2 || !in.holds || !in.fused) return StepAction::count;
  return StepAction::capture;
}

}  // namespace msc
