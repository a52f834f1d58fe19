// mixture_state.hpp -- an entity_based_state_object (entity_state.hpp) whose component models live in
// the device tables of microscopes_hip.h: the state object a Dirichlet-process mixture model hands to the
// sampling kernels, with the same per-entity contract (add_value / remove_value / score_value /
// score_likelihood / create_group / delete_group, entity_state.hpp:57-89) plus the batched calls the
// device is built for (assign_all, gibbs_sweep).
//
// What is where:
//   host    the partition (group_manager: assignment vector, group sizes, the set of empty groups, alpha),
//           the hypers objects of the component models, the group id <-> device slot map
//   device  the data (columnar, uploaded once), the assignment vector as slots, every group's suff-stats
// A group id is what the caller sees (never reused, as group_manager hands them out); a slot is the group's
// column in the device tables (0 .. max_groups-1, reused after delete_group).
//
// Per-entity calls are the latency path -- each is a handful of launches plus, for scores, one copy back
// (~30-100 us) -- and exist so that kernels written against the reference's interface run unchanged.
// gibbs_sweep() is the throughput path: one synchronous sweep over all entities on the device
// (msc_sweep_step), after which the host partition is rebuilt from the new assignment vector.
#pragma once

#include <cmath>
#include <map>
#include <memory>
#include <set>
#include <cstring>
#include <string>
#include <stdexcept>
#include <vector>

#include "../microscopes_hip.h"
#include "entity_state.hpp"
#include "group_manager.hpp"
#include "hip_models.hpp"
#include "recarray.hpp"

namespace microscopes {
namespace hip {

class mixture_state : public common::entity_based_state_object {
public:
  typedef common::entity_based_state_object::scores_t scores_t;

  // models[f] scores column f of `data`; max_groups = slots reserved in the device tables (groups alive at once)
  mixture_state(const std::vector<models::model_shared_ptr> &models, const common::recarray::row_major_dataview &data,
                size_t max_groups, msc_context *ctx = default_context())
      : ctx_(ctx), n_(data.size()), kmax_(max_groups), gm_(data.size()) {
    if (models.empty()) throw std::runtime_error("no component models");
    if (models.size() != data.types().size()) throw std::runtime_error("one model per column expected");
    if (!max_groups) throw std::runtime_error("max_groups must be positive");
    std::vector<msc_feature_spec> specs(models.size());
    std::vector<int32_t> col_types;
    for (size_t f = 0; f < models.size(); f++) {
      hypers_.push_back(models[f]->create_hypers());
      std::vector<float> hp;
      if (!hypers_[f]->device_spec(specs[f], hp)) throw std::runtime_error("component model has no device family");
      col_types.push_back(int32_t(models[f]->get_runtime_type().t()));     // convert at upload (runtime_type.hpp:153-161)
      hp_pushed_.push_back(std::vector<float>());
      nonconj_.push_back(specs[f].family == MSC_BBNC);   // the group carries a parameter of its own (bbnc.cpp:22-73)
      any_nonconj_ = any_nonconj_ || nonconj_.back();
    }
    view_ = data.to_device(ctx_, &col_types);
    specs_ = specs;
    col_types_ = col_types;
    check(msc_state_create(ctx_, specs.data(), uint32_t(specs.size()), uint32_t(kmax_), &st_));
    check(msc_device_alloc(ctx_, 4 * (n_ ? n_ : 1), reinterpret_cast<void **>(&z_dev_)));
    check(msc_pinned_alloc(ctx_, 4 * kmax_, reinterpret_cast<void **>(&row_host_), reinterpret_cast<void **>(&row_dev_)));   // the score row lands in host memory
    check(msc_device_alloc(ctx_, 4 * kmax_ * hypers_.size(), reinterpret_cast<void **>(&sd_dev_)));
    z_host_.assign(n_, -1);
    check(msc_device_upload(ctx_, z_dev_, z_host_.data(), 4 * n_));
    for (size_t s = kmax_; s-- > 0;) free_slots_.push_back(s);
  }
  ~mixture_state() override {
    if (st_) msc_state_destroy(st_);
    if (view_) msc_dataview_destroy(view_);
    msc_device_free(ctx_, z_dev_);
    msc_pinned_free(ctx_, row_host_);
    msc_device_free(ctx_, sd_dev_);
  }
  mixture_state(const mixture_state &) = delete;
  mixture_state &operator=(const mixture_state &) = delete;

  // ---- sizes and the partition ----
  size_t nentities() const override { return n_; }
  size_t ngroups() const override { sync(); return gm_.ngroups(); }
  size_t ncomponents() const override { return hypers_.size(); }
  std::vector<ssize_t> assignments() const override { sync(); return gm_.assignments(); }
  std::vector<size_t> groups() const override { sync(); return gm_.groups(); }
  size_t groupsize(size_t gid) const override { sync(); return gm_.groupsize(gid); }
  std::vector<size_t> empty_groups() const override {
    sync();
    return std::vector<size_t>(gm_.empty_groups().begin(), gm_.empty_groups().end());
  }

  // ---- parameters ----
  common::hyperparam_bag_t get_cluster_hp() const override { return gm_.get_hp(); }
  void set_cluster_hp(const common::hyperparam_bag_t &hp) override { gm_.set_hp(hp); }
  common::value_mutator get_cluster_hp_mutator(const std::string &key) override { return gm_.get_hp_mutator(key); }
  common::hyperparam_bag_t get_component_hp(size_t c) const override { return hypers_.at(c)->get_hp(); }
  void set_component_hp(size_t c, const common::hyperparam_bag_t &hp) override { hypers_.at(c)->set_hp(hp); }
  void set_component_hp(size_t c, const models::hypers &proto) override { hypers_.at(c)->set_hp(proto); }
  common::value_mutator get_component_hp_mutator(size_t c, const std::string &key) override {
    return hypers_.at(c)->get_hp_mutator(key);       // (written through a raw pointer: pushed to the device before the next device call)
  }

  // ---- sufficient statistics (identifier = group id) ----
  std::vector<common::ident_t> suffstats_identifiers(size_t) const override { sync(); return gm_.groups(); }
  common::suffstats_bag_t get_suffstats(size_t c, common::ident_t gid) const override { return fetch_group(c, gid)->get_ss(); }
  void set_suffstats(size_t c, common::ident_t gid, const common::suffstats_bag_t &ss) override {
    common::rng_t rng;
    auto g = hypers_.at(c)->create_group(rng);
    g->set_ss(ss);
    store_group(c, gid, *g);
  }
  // the device owns the numbers: a mutator would be a pointer into a copy (the reference's own dm model has no
  // mutators either, dm.cpp:120-124); read with get_suffstats, write with set_suffstats
  common::value_mutator get_suffstats_mutator(size_t, common::ident_t, const std::string &) override {
    throw std::runtime_error("suff-stats live on the device: use get_suffstats / set_suffstats");
  }

  // ---- membership ----
  void add_value(size_t gid, size_t eid, common::rng_t &) override {
    sync();
    const size_t slot = gm_.add_value(gid, eid);
    push_params();
    z_host_[eid] = int32_t(slot);
    // the group goes by value: one launch updates the sums, the group's fields and score constants, the counts and
    // the device's copy of the assignment -- nothing to upload, nothing to wait for
    check(msc_entity_op(st_, view_, nullptr, eid, uint32_t(slot), +1, z_dev_));
  }
  size_t remove_value(size_t eid, common::rng_t &) override {
    sync();
    const auto r = gm_.remove_value(eid);                 // (throws if the entity is not assigned); r = (gid, its slot)
    check(msc_entity_op(st_, view_, nullptr, eid, uint32_t(r.second), -1, z_dev_));
    z_host_[eid] = -1;
    return r.first;
  }

  // score[i] = log pseudocount(group i) + sum over components of score_value(group i, entity's value): the
  // unnormalised log-probability of the entity joining each group, empty groups included (alpha / n_empty each).
  // The likelihood terms come from one device pass over all slots; the prior is added here from the host partition.
  void inplace_score_value(scores_t &scores, size_t eid, common::rng_t &) const override {
    sync();
    if (gm_.assignments().at(eid) != -1) throw std::runtime_error("entity must be removed before it is scored");
    mixture_state *self = const_cast<mixture_state *>(this);
    self->push_params(true);
    check(msc_score_value(st_, view_, nullptr, eid, 1, nullptr, 0, row_dev_, kmax_));
    check(msc_context_synchronize(ctx_));                 // the only wait of a move; the row was written into pinned host memory
    const float *row = row_host_;
    scores.first.clear();
    scores.second.clear();
    for (auto it = gm_.begin(); it != gm_.end(); ++it) {
      scores.first.push_back(it->first);
      scores.second.push_back(std::log(gm_.pseudocount(it->first, it->second)) + row[it->second.data_]);
    }
  }

  float score_assignment() const override { sync(); return gm_.score_assignment(); }
  using common::entity_based_state_object::score_likelihood;
  float score_likelihood(size_t c, common::ident_t gid, common::rng_t &) const override {
    sync();
    if (c >= hypers_.size()) throw std::runtime_error("invalid component");
    const size_t slot = gm_.group(gid).data_;
    const_cast<mixture_state *>(this)->push_params();
    check(msc_score_data(st_, sd_dev_));
    float v = 0.f;
    check(msc_device_download(ctx_, &v, sd_dev_ + c * kmax_ + slot, 4));
    return v;
  }
  // every group of a component with one device pass and one copy (the per-id form above costs a pass each)
  float score_likelihood(size_t c, common::rng_t &) const override {
    sync();
    if (c >= hypers_.size()) throw std::runtime_error("invalid component");
    const_cast<mixture_state *>(this)->push_params();
    check(msc_score_data(st_, sd_dev_));
    std::vector<float> v(kmax_);
    check(msc_device_download(ctx_, v.data(), sd_dev_ + c * kmax_, 4 * kmax_));
    float total = 0.f;
    for (auto it = gm_.begin(); it != gm_.end(); ++it) total += v[it->second.data_];
    return total;
  }
  // log p(X, z | hp, alpha) = score_assignment() + the sum over the components of score_likelihood(c), what the
  // reference's users plot to judge burn-in (entity_state.hpp:76-83) -- in double on the device (msc_score_joint): one
  // launch and one copy of eight bytes, where the float virtuals above round every term to float, download every slot
  // and add on the host.  Every group the partition holds counts, empty ones included, as in score_likelihood.
  double score_joint() const {
    sync();
    mixture_state *self = const_cast<mixture_state *>(this);
    self->push_params(true);
    partition_slots slots(*self);
    double *out_dev = nullptr;
    check(msc_device_alloc(ctx_, 8 * (hypers_.size() + 3), reinterpret_cast<void **>(&out_dev)));
    double total = 0.0;
    int rc = msc_score_joint(st_, nullptr, 0, slots.p, out_dev);
    if (rc == MSC_OK) rc = msc_device_download(ctx_, &total, out_dev, 8);
    msc_device_free(ctx_, out_dev);
    check(rc);
    return total;
  }

  // ---- the supply of empty groups ----
  size_t create_group(common::rng_t &rng) override {
    sync();
    return create_group_unsynced(rng);
  }
  void delete_group(size_t gid) override {
    sync();
    const size_t slot = gm_.group(gid).data_;
    gm_.delete_group(gid);                                // (throws unless the group is empty: its device column is all zero then)
    free_slots_.push_back(slot);
  }

  // ---- batched calls (extension) ----
  // the whole partition at once: entity e joins group gids[e] (groups are created as needed); replaces
  // N add_value calls by one accumulate pass
  void assign_all(const std::vector<size_t> &labels, common::rng_t &rng) {
    sync();
    if (labels.size() != n_) throw std::runtime_error("one label per entity expected");
    for (size_t e = 0; e < n_; e++)
      if (gm_.assignments()[e] != -1) throw std::runtime_error("assign_all wants every entity unassigned");
    std::map<size_t, size_t> label_gid;
    for (size_t e = 0; e < n_; e++) {
      auto it = label_gid.find(labels[e]);
      if (it == label_gid.end()) it = label_gid.emplace(labels[e], create_group(rng)).first;
      z_host_[e] = int32_t(gm_.add_value(it->second, e));
    }
    push_params();
    check(msc_device_upload(ctx_, z_dev_, z_host_.data(), 4 * n_));
    check(msc_accumulate(st_, view_, nullptr, 0, n_, z_dev_, MSC_ACC_RESET));
  }

  // Grid hyper-parameter inference (msc_hp_grid_*): what downstream's grid_feature_hp / grid_cluster_hp do point by
  // point, one device pass per call.  `blocks` = npoints hp blocks back to back in the msc_state_set_hp layout of the
  // component; `logprior` = npoints values or empty (flat).  The likelihood sums over every group the partition holds,
  // empty ones included, as score_likelihood does.
  std::vector<double> score_likelihood_grid(size_t c, const std::vector<float> &blocks) const {
    sync();
    mixture_state *self = const_cast<mixture_state *>(this);
    self->push_params();
    hp_grid g(*self, uint32_t(c), blocks, std::vector<double>());
    std::vector<double> out(g.npoints);
    double *out_dev = nullptr;
    check(msc_device_alloc(ctx_, 8 * out.size(), reinterpret_cast<void **>(&out_dev)));
    const int rc = msc_hp_grid_score(g.h, g.slots, out_dev);
    if (rc == MSC_OK) check(msc_device_download(ctx_, out.data(), out_dev, 8 * out.size()));
    msc_device_free(ctx_, out_dev);
    check(rc);
    return out;
  }
  // one grid Gibbs step of component c: draws a point from the softmax of prior + likelihood (Philox(seed, sweep, ...),
  // msc_hp_grid_gibbs) and installs it on the device and in the component's hypers object; returns its index
  size_t grid_component_hp(size_t c, const std::vector<float> &blocks, const std::vector<double> &logprior, uint64_t seed,
                           uint64_t sweep) {
    sync();
    if (c >= hypers_.size()) throw std::runtime_error("invalid component");
    push_params();
    hp_grid g(*this, uint32_t(c), blocks, logprior);
    uint32_t k = 0;
    check(msc_hp_grid_gibbs(st_, &g.h, 1, g.slots, seed, sweep, &k, nullptr));
    const size_t nf = blocks.size() / g.npoints;
    install_component_hp(c, std::vector<float>(blocks.begin() + k * nf, blocks.begin() + (k + 1) * nf));
    return k;
  }
  // the same for the CRP concentration: `alphas` (> 0) and their log-prior; gm_'s alpha follows
  size_t grid_cluster_hp(const std::vector<float> &alphas, const std::vector<double> &logprior, uint64_t seed,
                         uint64_t sweep) {
    sync();
    push_params();
    hp_grid g(*this, MSC_HP_CLUSTER, alphas, logprior);
    uint32_t k = 0;
    check(msc_hp_grid_gibbs(st_, &g.h, 1, g.slots, seed, sweep, &k, nullptr));
    gm_.get_hp_mutator("alpha").set<float>(alphas[k]);
    alpha_pushed_ = alphas[k];                           // (the device took it in the same call)
    return k;
  }

  // Slice sampling (msc_hp_slice / msc_theta_slice): downstream's hp and theta kernels, one device call each.  The targets
  // count every group the partition holds, empty ones included, as the grid steps do.
  // one slice step of each of component c's coordinates, in order (`coords`: msc_slice_coord entries, their feature
  // field ignored); the component's hypers object follows.  Returns the values installed, one per entry.
  std::vector<float> slice_component_hp(size_t c, std::vector<msc_slice_coord> coords, uint64_t seed, uint64_t sweep) {
    sync();
    if (c >= hypers_.size()) throw std::runtime_error("invalid component");
    if (coords.empty()) return {};
    push_params();
    for (auto &e : coords) e.feature = uint32_t(c);
    std::vector<float> values(coords.size());
    partition_slots slots(*this);
    check(msc_hp_slice(st_, coords.data(), uint32_t(coords.size()), slots.p, seed, sweep, values.data(), nullptr));
    std::vector<float> blk(hp_pushed_[c].size());
    check(msc_state_get_hp(st_, uint32_t(c), blk.data(), blk.size()));
    install_component_hp(c, blk);
    return values;
  }
  // the same for the CRP concentration: prior MSC_PRIOR_* with parameters (a, b), width w; gm_'s alpha follows
  float slice_cluster_hp(uint32_t prior, float a, float b, float w, uint64_t seed, uint64_t sweep) {
    sync();
    push_params(true);
    msc_slice_coord e{MSC_HP_CLUSTER, 0, w, prior, a, b, 0};
    float alpha = 0.f;
    check(msc_hp_slice(st_, &e, 1, nullptr, seed, sweep, &alpha, nullptr));
    gm_.get_hp_mutator("alpha").set<float>(alpha);
    alpha_pushed_ = alpha;                               // (the device took it in the same call)
    return alpha;
  }
  // one slice step of the p of every group of bbnc component c (width w); get_suffstats shows the new p.  Returns
  // the evaluations the step took.
  uint64_t slice_theta(size_t c, float w, uint64_t seed, uint64_t sweep) {
    sync();
    if (c >= hypers_.size()) throw std::runtime_error("invalid component");
    push_params();
    partition_slots slots(*this);
    const uint32_t f = uint32_t(c);
    uint64_t evals = 0;
    check(msc_theta_slice(st_, &f, &w, 1, slots.p, seed, sweep, &evals));
    return evals;
  }

  // One synchronous Gibbs sweep over all entities on the device: every entity is scored leave-one-out against the
  // tables as they stand, with the CRP prior (every free slot is an empty group on offer and they share alpha,
  // which is the prior of "a new group" however many empty groups the host has created), re-drawn with the
  // counter-based uniform Philox(seed, sweep, entity), and the tables are rebuilt.  The host partition follows the new
  // assignment vector the next time something looks at it (sync(): slots that gained their first member get a group
  // id, groups that lost every member stay as empty groups -- delete_group them if unwanted), so a run of sweeps costs
  // the host nothing.
  void gibbs_sweep(uint64_t seed, uint64_t sweep, common::rng_t &rng) {
    if (any_nonconj_) {
      sync();                                           // (which slots are free is host knowledge)
      refresh_free_slots(rng);
    }
    if (!stale_)                                        // (after a sweep every entity is assigned)
      for (size_t e = 0; e < n_; e++)
        if (gm_.assignments()[e] == -1) throw std::runtime_error("gibbs_sweep wants every entity assigned");
    push_params(true);
    check(msc_sweep_step(st_, view_, nullptr, 0, n_, 0, z_dev_, seed, sweep));
    stale_ = true;      // the host partition follows when somebody looks at it: sweep after sweep costs the host nothing
  }

  // nsweeps SEQUENTIAL Gibbs sweeps over all entities on the device (msc_sweep_sequential): the reference's own chain --
  // each entity leaves its group, is scored against the tables as the entity before it left them (CRP prior, every
  // free slot an empty group on offer), re-drawn with Philox(seed, sweep + s, entity) and joins -- in one call.  Entities
  // not yet assigned are seated.  As gibbs_sweep, the host partition follows the assignment vector lazily (sync()).
  // A non-conjugate component throws: free slots' parameters are drawn between sweeps only (refresh_free_slots), and a
  // slot emptied mid-sweep would be offered with a stale one; niw and dm components throw as the library refuses them.
  void gibbs_sweep_sequential(uint64_t seed, uint64_t sweep, common::rng_t &rng, uint32_t nsweeps = 1) {
    (void)rng;                                          // (conjugate components only: nothing to draw on the host)
    if (any_nonconj_) throw std::runtime_error("gibbs_sweep_sequential takes conjugate components only");
    push_params(true);
    check(msc_sweep_sequential(st_, view_, nullptr, 0, n_, 0, z_dev_, nullptr, nsweeps, seed, sweep, nullptr));
    stale_ = true;
  }

  // nsweeps BLOCKED Gibbs sweeps over all entities on the device (msc_sweep_blocked): the truncated stick-breaking
  // sampler -- every slot's parameters and the stick weights drawn from the tables, then every entity's slot drawn
  // independently under them, the tables rebuilt -- exact up to the truncation at the state's slot count and parallel
  // over entities.  The first draw conditions on the tables as they stand; as gibbs_sweep, the host partition follows the
  // assignment vector lazily (sync()).  Non-conjugate (bbnc), niw and dm components throw: the library refuses them.
  void gibbs_sweep_blocked(uint64_t seed, uint64_t sweep, common::rng_t &rng, uint32_t nsweeps = 1) {
    (void)rng;                                          // (every draw is the device's)
    if (any_nonconj_) throw std::runtime_error("gibbs_sweep_blocked takes conjugate components only");
    for (const auto &s : specs_)
      if (s.family == MSC_NIW || s.family == MSC_DM)
        throw std::runtime_error("gibbs_sweep_blocked does not take niw or dm components");
    push_params(true);
    check(msc_sweep_blocked(st_, view_, nullptr, 0, n_, 0, z_dev_, nsweeps, seed, sweep, nullptr, nullptr));
    stale_ = true;
  }

  // nproposals SPLIT-MERGE Metropolis-Hastings proposals over all entities on the device (msc_split_merge): each picks
  // two entities, proposes to split their group in two (into the lowest free slot) or to merge their two groups, from a
  // launch state reached by launch_iters restricted blocked Gibbs passes, and accepts or rejects on the device.  Proposal
  // p uses the sweep counter sweep + p.  Returns what was proposed and accepted; as gibbs_sweep, the host partition
  // follows the assignment vector lazily (sync()).  Non-conjugate (bbnc), niw and dm components throw.
  struct split_merge_counts {
    uint64_t splits = 0, splits_accepted = 0, merges = 0, merges_accepted = 0, voids = 0;
  };
  split_merge_counts split_merge(uint64_t seed, uint64_t sweep, common::rng_t &rng, uint32_t nproposals = 1,
                                 uint32_t launch_iters = 2) {
    (void)rng;                                          // (every draw is the device's)
    if (any_nonconj_) throw std::runtime_error("split_merge takes conjugate components only");
    for (const auto &s : specs_)
      if (s.family == MSC_NIW || s.family == MSC_DM) throw std::runtime_error("split_merge does not take niw or dm components");
    push_params(true);
    uint64_t c[5] = {0, 0, 0, 0, 0};
    uint64_t *c_dev = nullptr;
    check(msc_device_alloc(ctx_, sizeof c, reinterpret_cast<void **>(&c_dev)));
    int rc = msc_device_upload(ctx_, c_dev, c, sizeof c);
    if (rc == MSC_OK)
      rc = msc_split_merge(st_, view_, nullptr, 0, n_, 0, z_dev_, nproposals, launch_iters, seed, sweep, nullptr, nullptr,
                           nullptr, c_dev);
    if (rc == MSC_OK) rc = msc_device_download(ctx_, c, c_dev, sizeof c);
    msc_device_free(ctx_, c_dev);
    check(rc);
    stale_ = true;
    split_merge_counts out;
    out.splits = c[0], out.splits_accepted = c[1], out.merges = c[2], out.merges_accepted = c[3], out.voids = c[4];
    return out;
  }

  // Posterior predictive draws for new, partly observed rows (downstream's sample_post_pred): each row of `rows` (the
  // state's column layout, with its mask) gets a group drawn from the CRP term plus the scores of its observed entries
  // against the tables as they stand, then its masked entries are drawn from that group's posterior predictive -- ONE
  // msc_sample_predictive call (z NULL, MSC_PRED_MASKED_ONLY; Philox counters of seed and sweep as the header documents).
  // Returns the completed records in `rows`' own layout: observed bytes as they were, masked values converted to their
  // field's type (a vector value with any masked element is drawn whole).  groups (nullable) receives each row's slot.
  std::vector<uint8_t> sample_post_pred(const common::recarray::row_major_dataview &rows, uint64_t seed, uint64_t sweep,
                                        std::vector<int32_t> *groups = nullptr) {
    if (rows.types().size() != specs_.size()) throw std::runtime_error("one column per component model expected");
    const size_t n = rows.size(), nf = specs_.size();
    const auto layout = common::runtime_type::GetOffsetsAndSize(rows.types());
    std::vector<uint8_t> out(n * layout.rowsize_);
    std::memcpy(out.data(), rows.records(), out.size());
    if (groups) groups->assign(n, -1);
    if (n == 0) return out;
    push_params(true);
    msc_dataview *v = rows.to_device(ctx_, &col_types_);
    std::vector<void *> cols(nf, nullptr);
    std::vector<size_t> esize(nf, 0);
    int32_t *z_out = nullptr;
    int rc = msc_device_alloc(ctx_, 4 * n, reinterpret_cast<void **>(&z_out));
    for (size_t f = 0; f < nf && rc == MSC_OK; f++) {
      esize[f] = specs_[f].family == MSC_BB || specs_[f].family == MSC_BBNC ? 1 : 4;    // the header's output types
      rc = msc_device_alloc(ctx_, n * rows.types()[f].n() * esize[f], &cols[f]);
    }
    if (rc == MSC_OK)
      rc = msc_sample_predictive(st_, v, nullptr, 0, n, 0, nullptr, z_out, MSC_PRED_MASKED_ONLY, seed, sweep, cols.data());
    std::vector<std::vector<uint8_t>> host(nf);
    std::vector<int32_t> zh(n);
    for (size_t f = 0; f < nf && rc == MSC_OK; f++) {
      host[f].resize(n * rows.types()[f].n() * esize[f]);
      rc = msc_device_download(ctx_, host[f].data(), cols[f], host[f].size());
    }
    if (rc == MSC_OK) rc = msc_device_download(ctx_, zh.data(), z_out, 4 * n);
    const std::string err = rc == MSC_OK ? std::string() : std::string(msc_last_error());
    for (void *c : cols) msc_device_free(ctx_, c);
    msc_device_free(ctx_, z_out);
    msc_dataview_destroy(v);
    if (rc != MSC_OK) throw std::runtime_error(err);
    // masked values into the records, converted as runtime_cast does
    size_t moff = 0;
    for (size_t f = 0; f < nf; f++) {
      const common::runtime_type &t = rows.types()[f];
      const unsigned cnt = t.n();
      for (size_t i = 0; i < n; i++) {
        const bool *m = rows.mask() ? rows.mask() + i * layout.maskrowsize_ : nullptr;
        bool any = false;
        for (unsigned e = 0; e < cnt && m; e++) any = any || m[moff + e];
        if (!any) continue;
        common::value_mutator vm(out.data() + i * layout.rowsize_ + layout.offsets_[f], t);
        const uint8_t *src = host[f].data() + (i * cnt) * esize[f];
        for (unsigned e = 0; e < cnt; e++) {
          switch (specs_[f].family) {
            case MSC_BB:
            case MSC_BBNC: vm.set<bool>(src[e] != 0, e); break;
            case MSC_GP:
            case MSC_BNB: { uint32_t x; std::memcpy(&x, src + 4 * e, 4); vm.set<uint32_t>(x, e); break; }
            case MSC_DD: { int32_t x; std::memcpy(&x, src + 4 * e, 4); vm.set<int32_t>(x, e); break; }
            default: { float x; std::memcpy(&x, src + 4 * e, 4); vm.set<float>(x, e); break; }
          }
        }
      }
      moff += cnt;
    }
    if (groups) *groups = zh;
    return out;
  }

  // The log posterior predictive density of new rows under the state (downstream's held-out log-likelihood and, as a
  // difference of two such numbers, its conditional queries): log sum over the slots of pseudocount / (n + alpha) times the
  // product of the observed entries' predictive densities -- ONE msc_score_marginal call (no leave-one-out: the rows are
  // not the state's entities); a masked entry contributes nothing, free slots share alpha as empty groups do.
  // map_slots (nullable) receives every row's MAP slot (slot_of(gid) maps a group to its slot; the lowest slot among
  // exact ties), map_logresp (nullable) the log responsibility of that slot (<= 0).
  std::vector<float> log_post_pred(const common::recarray::row_major_dataview &rows, std::vector<int32_t> *map_slots = nullptr,
                                   std::vector<float> *map_logresp = nullptr) {
    if (rows.types().size() != specs_.size()) throw std::runtime_error("one column per component model expected");
    const size_t n = rows.size();
    std::vector<float> out(n);
    if (map_slots) map_slots->assign(n, -1);
    if (map_logresp) map_logresp->assign(n, 0.f);
    if (n == 0) return out;
    push_params(true);
    msc_dataview *v = rows.to_device(ctx_, &col_types_);
    float *logp = nullptr, *lr = nullptr;
    int32_t *mp = nullptr;
    int rc = msc_device_alloc(ctx_, 4 * n, reinterpret_cast<void **>(&logp));
    if (rc == MSC_OK && map_slots) rc = msc_device_alloc(ctx_, 4 * n, reinterpret_cast<void **>(&mp));
    if (rc == MSC_OK && map_logresp) rc = msc_device_alloc(ctx_, 4 * n, reinterpret_cast<void **>(&lr));
    if (rc == MSC_OK) rc = msc_score_marginal(st_, v, nullptr, 0, n, nullptr, 0, logp, mp, lr);
    if (rc == MSC_OK) rc = msc_device_download(ctx_, out.data(), logp, 4 * n);
    if (rc == MSC_OK && mp) rc = msc_device_download(ctx_, map_slots->data(), mp, 4 * n);
    if (rc == MSC_OK && lr) rc = msc_device_download(ctx_, map_logresp->data(), lr, 4 * n);
    const std::string err = rc == MSC_OK ? std::string() : std::string(msc_last_error());
    if (logp) msc_device_free(ctx_, logp);
    if (mp) msc_device_free(ctx_, mp);
    if (lr) msc_device_free(ctx_, lr);
    msc_dataview_destroy(v);
    if (rc != MSC_OK) throw std::runtime_error(err);
    return out;
  }

  // the device handles, for callers that mix in calls of microscopes_hip.h
  msc_state *device_state() const { return st_; }
  msc_dataview *device_view() const { return view_; }
  const int32_t *device_assignments() const { return z_dev_; }
  size_t slot_of(size_t gid) const { sync(); return gm_.group(gid).data_; }

private:
  // After batched sweeps the partition lives in z_dev_ alone; anything that reads or edits the host's view of it
  // calls this first: one download and an O(n + groups) rebuild (slots that gained their first member become
  // groups, groups that lost every member stay as empty groups).
  void sync() const {
    if (!stale_) return;
    mixture_state *self = const_cast<mixture_state *>(this);
    self->stale_ = false;
    check(msc_device_download(ctx_, self->z_host_.data(), z_dev_, 4 * n_));
    std::vector<ssize_t> slot_gid(kmax_, -1);
    for (auto it = gm_.begin(); it != gm_.end(); ++it) slot_gid[it->second.data_] = ssize_t(it->first);
    std::vector<ssize_t> a(n_);
    for (size_t e = 0; e < n_; e++) {
      const size_t slot = size_t(z_host_[e]);
      if (slot >= kmax_) throw std::runtime_error("device drew a slot outside the table");
      if (slot_gid[slot] < 0) {                          // a free slot was drawn: it becomes a group
        const auto pos = std::find(self->free_slots_.begin(), self->free_slots_.end(), slot);
        if (pos == self->free_slots_.end()) throw std::runtime_error("device drew a slot the host does not know");
        std::swap(*pos, self->free_slots_.back());
        common::rng_t rng;
        slot_gid[slot] = ssize_t(self->create_group_unsynced(rng, true));
      }
      a[e] = slot_gid[slot];
    }
    self->gm_.reassign_all(a);
  }
  // keep_record: the slot was on offer during a sweep and rows were scored against (and added to) what it holds --
  // its record already is the group's
  size_t create_group_unsynced(common::rng_t &rng, bool keep_record = false) {
    if (free_slots_.empty()) throw std::runtime_error("all max_groups device slots are in use");
    auto r = gm_.create_group();
    r.second = free_slots_.back();
    free_slots_.pop_back();
    if (!keep_record) init_slot(r.second, rng);
    return r.first;
  }
  // What mixturemodel's create_group does per component (hypers::create_group, base.hpp:48): the model's own initial
  // group goes into the slot.  For the conjugate families that record is all zero, which is what a slot holds once its
  // group has emptied (and what it is created with), so nothing is written; a non-conjugate model draws its
  // parameter here (bbnc: p ~ Beta(alpha, beta), bbnc.cpp:129-133) and the slot must not keep the previous occupant's.
  void init_slot(size_t slot, common::rng_t &rng) {
    for (size_t c = 0; c < hypers_.size(); c++) {
      if (!nonconj_[c]) continue;
      auto g = hypers_[c]->create_group(rng);
      std::vector<uint8_t> rec;
      g->device_record_get(*hypers_[c], rec);
      if (!rec.empty()) check(msc_state_set_ss(st_, uint32_t(c), uint32_t(slot), 1, rec.data(), rec.size()));
    }
  }
  // Every free slot is an empty group on offer in a sweep; for a non-conjugate component each gets a fresh draw of
  // its parameter first (one read-modify-write of the component's table, only for such components).
  void refresh_free_slots(common::rng_t &rng) {
    if (free_slots_.empty()) return;
    for (size_t c = 0; c < hypers_.size(); c++) {
      if (!nonconj_[c]) continue;
      msc_feature_spec spec;
      std::vector<float> hp;
      hypers_[c]->device_spec(spec, hp);
      const size_t rb = msc_ss_bytes(spec.family, spec.dim);
      std::vector<uint8_t> all(rb * kmax_), rec;
      check(msc_state_get_ss(st_, uint32_t(c), 0, uint32_t(kmax_), all.data(), all.size()));
      for (size_t slot : free_slots_) {
        auto g = hypers_[c]->create_group(rng);
        g->device_record_get(*hypers_[c], rec);
        if (rec.size() == rb) std::copy(rec.begin(), rec.end(), all.begin() + rb * slot);
      }
      check(msc_state_set_ss(st_, uint32_t(c), 0, uint32_t(kmax_), all.data(), all.size()));
    }
  }
  mutable bool stale_ = false;

  // the device mask of the slots the partition holds (its groups, empty ones included)
  struct partition_slots {
    msc_context *ctx;
    uint8_t *p = nullptr;
    explicit partition_slots(mixture_state &s) : ctx(s.ctx_) {
      std::vector<uint8_t> mask(s.kmax_, 0);
      for (auto it = s.gm_.begin(); it != s.gm_.end(); ++it) mask[it->second.data_] = 1;
      check(msc_device_alloc(ctx, mask.size(), reinterpret_cast<void **>(&p)));
      check(msc_device_upload(ctx, p, mask.data(), mask.size()));
    }
    ~partition_slots() { msc_device_free(ctx, p); }
    partition_slots(const partition_slots &) = delete;
    partition_slots &operator=(const partition_slots &) = delete;
  };
  // a grid of one call and the device mask of the slots the partition holds
  struct hp_grid {
    msc_hp_grid *h = nullptr;
    partition_slots mask;
    uint8_t *slots;
    uint32_t npoints;
    hp_grid(mixture_state &s, uint32_t feature, const std::vector<float> &blocks, const std::vector<double> &logprior)
        : mask(s), slots(mask.p) {
      const size_t nf = feature == MSC_HP_CLUSTER ? 1 : s.hp_pushed_.at(feature).size();
      if (!nf || blocks.empty() || blocks.size() % nf) throw std::runtime_error("grid blocks do not match the hp size");
      npoints = uint32_t(blocks.size() / nf);
      if (!logprior.empty() && logprior.size() != npoints) throw std::runtime_error("one log-prior value per point expected");
      check(msc_hp_grid_create(s.st_, feature, blocks.data(), nf, npoints, logprior.empty() ? nullptr : logprior.data(), &h));
    }
    ~hp_grid() { msc_hp_grid_destroy(h); }
  };
  // the chosen block into the component's hypers object (its mutators), and what the device now holds
  void install_component_hp(size_t c, const std::vector<float> &blk) {
    msc_feature_spec spec;
    std::vector<float> hp;
    hypers_[c]->device_spec(spec, hp);
    static const char *const two[] = {"alpha", "beta"}, *const gp[] = {"alpha", "inv_beta"},
                             *const bnb[] = {"alpha", "beta", "r"}, *const nich[] = {"mu", "kappa", "sigmasq", "nu"};
    const char *const *keys = nullptr;
    switch (spec.family) {
      case MSC_BB: case MSC_BBNC: keys = two; break;
      case MSC_GP: keys = gp; break;
      case MSC_BNB: keys = bnb; break;
      case MSC_NICH: keys = nich; break;
      case MSC_DD: case MSC_DM: {
        auto m = hypers_[c]->get_hp_mutator("alphas");
        for (size_t i = 0; i < blk.size(); i++) m.set<float>(blk[i], i);
      } break;
      default: throw std::runtime_error("component has no hyper-parameter grid or slice");
    }
    if (keys)
      for (size_t i = 0; i < blk.size(); i++) hypers_[c]->get_hp_mutator(keys[i]).set<float>(blk[i]);
    hp_pushed_[c] = blk;
  }

  // hyper-parameters can change behind our back (mutators are raw pointers), so what the device holds is
  // compared with the hypers objects before every device call; a handful of floats per component
  void push_params(bool need_alpha = false) {
    for (size_t f = 0; f < hypers_.size(); f++) {
      msc_feature_spec spec;
      std::vector<float> hp;
      hypers_[f]->device_spec(spec, hp);
      if (hp != hp_pushed_[f]) {
        if (!hp.empty()) check(msc_state_set_hp(st_, uint32_t(f), hp.data(), hp.size()));
        hp_pushed_[f] = hp;
      }
    }
    const float alpha = gm_.get_hp_mutator("alpha").accessor().get<float>(0);
    // group_manager.hpp:78 asserts alpha > 0 where it is used; the device would otherwise keep its default of 1 and
    // draw under another concentration than the host's pseudocount() / score_assignment()
    if (!(alpha > 0.f)) {
      if (need_alpha) throw std::runtime_error("cluster hyper-parameter alpha must be set (> 0) before scoring or sweeping");
      return;                                           // (membership edits and likelihoods do not read it)
    }
    if (alpha != alpha_pushed_) {
      check(msc_state_set_alpha(st_, alpha));
      alpha_pushed_ = alpha;
    }
  }
  std::shared_ptr<models::group> fetch_group(size_t c, size_t gid) const {
    sync();
    const size_t slot = gm_.group(gid).data_;
    common::rng_t rng;
    auto g = hypers_.at(c)->create_group(rng);
    msc_feature_spec spec;
    std::vector<float> hp;
    hypers_[c]->device_spec(spec, hp);
    std::vector<uint8_t> rec(msc_ss_bytes(spec.family, spec.dim));
    if (!rec.empty()) check(msc_state_get_ss(st_, uint32_t(c), uint32_t(slot), 1, rec.data(), rec.size()));
    g->device_record_set(*hypers_[c], rec);
    return g;
  }
  void store_group(size_t c, size_t gid, const models::group &g) {
    sync();
    const size_t slot = gm_.group(gid).data_;
    std::vector<uint8_t> rec;
    g.device_record_get(*hypers_.at(c), rec);
    if (!rec.empty()) check(msc_state_set_ss(st_, uint32_t(c), uint32_t(slot), 1, rec.data(), rec.size()));
  }

  msc_context *ctx_;
  size_t n_, kmax_;
  common::group_manager<size_t> gm_;                   // group data = the group's device slot
  std::vector<models::hypers_shared_ptr> hypers_;
  std::vector<std::vector<float>> hp_pushed_;
  std::vector<msc_feature_spec> specs_;                // the device families of the components
  std::vector<int32_t> col_types_;                     // the value type each column is converted to on upload
  std::vector<bool> nonconj_;                          // per component: does a new group start from a draw?
  bool any_nonconj_ = false;
  float alpha_pushed_ = -1.f;
  std::vector<size_t> free_slots_;
  std::vector<int32_t> z_host_;                        // the assignment vector as slots, mirror of z_dev_
  msc_dataview *view_ = nullptr;
  msc_state *st_ = nullptr;
  int32_t *z_dev_ = nullptr;
  float *row_dev_ = nullptr, *row_host_ = nullptr, *sd_dev_ = nullptr;
};

}  // namespace hip
}  // namespace microscopes
