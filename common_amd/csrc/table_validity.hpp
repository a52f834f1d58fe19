// table_validity.hpp -- which of a state's device tables are current: the one owner of the host flags.  Host only: no
// HIP header, builds with the plain host compiler (tests/cxx/test_table_validity.cpp).
//
// A msc_state keeps the same truth in four device representations (msc_internal.hpp lists the tables): the RAW fields,
// the ADDITIVE int64 / float64 sums, the DERIVED score constants and the CRP table; the blocked sampler's parameter DRAW
// is made from the raw fields, the hyper-parameters, alpha and the counts.  Per feature the flags say whether raw holds
// the truth, whether additive and derived are in sync with it; per state, whether the additive copy of the counts and
// the CRP table are in sync with the counts, and whether a draw was made from everything as it stands.
//
// The interface is the EVENTS that happen to a state (abi.cpp and the units beside it say which, never what to do to a flag):
//
//   event                      raw     additive    derived    counts' additive   crp     draw     who reports it
//   created(n)                 all 1   all 1       all 0      1                  0       0        msc_state_create (all zero)
//   fields_written(f)          .       f: 0        f: 0       .                  .       0        msc_state_set_ss
//   hp_changed(f)              .       .           f: 0       .                  .       0        msc_state_set_hp, hp_installed,
//                                                                                                 msc_theta_slice (*)
//   derived_dropped(f)         .       .           f: 0       .                  .       .        bind_view, bind_dm_column re-plan
//   alpha_changed()            .       .           .          .                  0       0        msc_state_set_alpha, alpha_installed
//   counts_changed()           .       .           .          0                  0       0        msc_state_set_group_counts (host),
//                                                                                                 msc_split_merge (a kernel moved them)
//   additive_lifted()          .       all 1       .          1                  .       .        ensure_additive; a resetting
//                                                                                                 accumulate's zeroing in its place
//   accumulated()              all 0   all 1       .          1                  .       0        accumulate_impl; msc_chains_clone
//                                                                                                 (a destination's sums replaced)
//   additive_rewritten()       .       .           .          .                  .       0        msc_state_reduce_unpack
//   committed()                all 1   .           all 0      .                  0       0        commit, ensure_raw
//   committed_and_prepared()   all 1   .           all 1      .                  1       0        commit_and_prepare
//   prepared()                 .       .           all 1      .                  .       .        ensure_derived, msc_chains_hp_slice
//   crp_prepared()             .       .           .          .                  1       .        ensure_crp, msc_chains_hp_slice
//   kept_current()             all 1   all 1       all 1      1                  1       0        msc_entity_op's kernel,
//                                                                                                 msc_sweep_sequential, msc_chains_sweep,
//                                                                                                 msc_chains_sweep_tempered
//   step_began()               .       .           .          .                  .       0        msc_sweep_step (a replayed graph
//                                                                                                 passes none of the events above)
//   drawn()                    .       .           .          .                  .       1        blocked_draw_impl
//
//   ("." = left as it is.  (*) the p of a bbnc group: the states that hold bbnc never have a draw.)
//
// Every event that changes what a draw was made from drops the draw here; no caller does.
#pragma once

#include <cstddef>
#include <vector>

namespace msc {

class TableValidity {
 public:
  // the flags as a value: a captured sweep step must leave them as it found them (msc_sweep_step)
  class Snapshot {
   public:
    bool operator==(const Snapshot &o) const {
      return feat == o.feat && cnt_additive == o.cnt_additive && crp == o.crp && draw == o.draw;
    }
    bool operator!=(const Snapshot &o) const { return !(*this == o); }

   private:
    friend class TableValidity;
    struct Feat {
      bool raw, additive, derived;
      bool operator==(const Feat &o) const { return raw == o.raw && additive == o.additive && derived == o.derived; }
    };
    std::vector<Feat> feat;
    bool cnt_additive = false, crp = false, draw = false;
  };
  Snapshot snapshot() const { return v_; }
  void restore(const Snapshot &s) { v_ = s; }

  // ---- events ----
  void created(size_t nfeat) {
    v_.feat.assign(nfeat, {true, true, false});
    v_.cnt_additive = true;
    v_.crp = v_.draw = false;
  }
  void fields_written(size_t f) {
    v_.feat[f].additive = v_.feat[f].derived = false;
    v_.draw = false;
  }
  void hp_changed(size_t f) {
    v_.feat[f].derived = false;
    v_.draw = false;
  }
  void derived_dropped(size_t f) { v_.feat[f].derived = false; }
  void alpha_changed() { v_.crp = v_.draw = false; }
  void counts_changed() { v_.cnt_additive = v_.crp = v_.draw = false; }
  void additive_lifted() {
    for (auto &h : v_.feat) h.additive = true;
    v_.cnt_additive = true;
  }
  void accumulated() {
    for (auto &h : v_.feat) h.raw = false, h.additive = true;
    v_.cnt_additive = true;
    v_.draw = false;
  }
  void additive_rewritten() { v_.draw = false; }
  void committed() {
    for (auto &h : v_.feat) h.raw = true, h.derived = false;
    v_.crp = v_.draw = false;
  }
  void committed_and_prepared() {
    for (auto &h : v_.feat) h.raw = h.derived = true;
    v_.crp = true;
    v_.draw = false;
  }
  void prepared() {
    for (auto &h : v_.feat) h.derived = true;
  }
  void crp_prepared() { v_.crp = true; }
  void kept_current() {
    for (auto &h : v_.feat) h.raw = h.additive = h.derived = true;
    v_.cnt_additive = v_.crp = true;
    v_.draw = false;
  }
  void step_began() { v_.draw = false; }
  void drawn() { v_.draw = true; }

  // ---- queries ----
  bool any_raw_stale() const {
    for (auto &h : v_.feat)
      if (!h.raw) return true;
    return false;
  }
  bool raw_stale(size_t f) const { return !v_.feat[f].raw; }
  bool additive_stale(size_t f) const { return !v_.feat[f].additive; }
  bool counts_additive_stale() const { return !v_.cnt_additive; }
  bool derived_stale(size_t f) const { return !v_.feat[f].derived; }
  bool any_derived_stale() const {
    for (auto &h : v_.feat)
      if (!h.derived) return true;
    return false;
  }
  bool crp_stale() const { return !v_.crp; }
  bool draw_current() const { return v_.draw; }

 private:
  Snapshot v_;
};

}  // namespace msc
