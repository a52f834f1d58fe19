// mixture_state::log_post_pred: the log posterior predictive density of new rows, with the MAP slot and its log
// responsibility.  The twin is the host's: for every slot, log pseudocount (free slots share alpha) + the sum over the
// components of score_value of a plugin group fed the state's own suff-stats of that (component, group) -- a fresh group
// for a free slot --, the log-sum-exp over the slots in double, minus log(n + alpha).  Gate (tests/test_gpu_marginal.py):
// E_r + 1e-6 max(1, |want|) with E_r = 1e-6 max_k sum_f max(1, |score_f|), through audit.hpp.  A masked entry contributes
// nothing.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>

#include <microscopes/common/entity_state.hpp>
#include <microscopes/models/distributions.hpp>
#include <microscopes_amd/mixture_state.hpp>

#include "audit.hpp"

using namespace microscopes;
using namespace microscopes::common;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

#pragma pack(push, 1)
struct Row {
  bool b;
  uint32_t c;
  float x;
  int32_t d;
};
#pragma pack(pop)

int main() {
  rng_t rng(3);
  const size_t N = 2000, M = 1500, KMAX = 16, NF = 4;
  const double alpha = 1.5;
  std::mt19937 gen(11);
  auto make = [&](size_t n, std::vector<Row> &rows, std::vector<size_t> *labels) {
    rows.resize(n);
    for (size_t i = 0; i < n; i++) {
      const int comp = int(gen() % 4);
      if (labels) labels->push_back(size_t(comp));
      rows[i].b = std::bernoulli_distribution(0.1 + 0.25 * comp)(gen);
      rows[i].c = uint32_t(std::poisson_distribution<int>(1 + 4 * comp)(gen));
      rows[i].x = float(std::normal_distribution<double>(3.0 * comp, 1.0)(gen));
      rows[i].d = int32_t((comp + gen() % 2) % 4);
    }
  };
  std::vector<Row> rows, fresh;
  std::vector<size_t> labels;
  make(N, rows, &labels);
  make(M, fresh, nullptr);
  const std::vector<runtime_type> types = {runtime_type(TYPE_B), runtime_type(TYPE_U32), runtime_type(TYPE_F32),
                                           runtime_type(TYPE_I32)};
  recarray::row_major_dataview data(reinterpret_cast<const uint8_t *>(rows.data()), nullptr, N, types);
  std::vector<models::model_shared_ptr> mdl = {
      std::make_shared<models::distributions_model<distributions::BetaBernoulli>>(),
      std::make_shared<models::distributions_model<distributions::GammaPoisson>>(),
      std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>(),
      std::make_shared<models::distributions_model_dd128>(4)};
  hip::mixture_state st(mdl, data, KMAX);
  entity_based_state_object &iface = st;
  iface.get_cluster_hp_mutator("alpha").set<float>(float(alpha));
  st.assign_all(labels, rng);
  std::vector<models::hypers_shared_ptr> hy;
  for (auto &m : mdl) hy.push_back(m->create_hypers());

  // the new rows: every feature masked in about a fifth of them
  std::vector<uint8_t> mask(M * NF);
  for (auto &m : mask) m = std::bernoulli_distribution(0.2)(gen);
  recarray::row_major_dataview q(reinterpret_cast<const uint8_t *>(fresh.data()), reinterpret_cast<const bool *>(mask.data()),
                                 M, types);
  std::vector<int32_t> slots;
  std::vector<float> logresp;
  const std::vector<float> logp = st.log_post_pred(q, &slots, &logresp);
  CHECK(logp.size() == M && slots.size() == M && logresp.size() == M);
  const std::vector<float> alone = st.log_post_pred(q);
  CHECK(alone == logp);                                       // the optional outputs change no bit of logp

  // the slots: the groups that hold entities, then the free slots as one empty group each
  std::vector<std::vector<models::group_shared_ptr>> groups;  // per occupied group: a plugin group per component
  std::vector<double> prior;
  std::vector<int32_t> slot;
  size_t total = 0;
  for (size_t gid : iface.groups()) {
    const size_t cnt = iface.groupsize(gid);
    if (!cnt) continue;
    total += cnt;
    std::vector<models::group_shared_ptr> gs;
    for (size_t f = 0; f < NF; f++) {
      gs.push_back(hy[f]->create_group(rng));
      gs.back()->set_ss(iface.get_suffstats(f, gid));
    }
    groups.push_back(gs);
    prior.push_back(std::log(double(cnt)));
    slot.push_back(int32_t(st.slot_of(gid)));
  }
  CHECK(total == N && groups.size() == 4);
  const size_t nfree = KMAX - groups.size();
  std::vector<models::group_shared_ptr> empty;
  for (size_t f = 0; f < NF; f++) empty.push_back(hy[f]->create_group(rng));
  const double norm = std::log(double(N) + alpha);
  size_t decided = 0;
  for (size_t i = 0; i < M; i++) {
    std::vector<double> t;
    double mag = 0;
    for (size_t k = 0; k <= groups.size(); k++) {
      const bool free_slot = k == groups.size();
      double v = free_slot ? std::log(alpha / double(nfree)) : prior[k], m = 0;
      auto acc = q.get(i);
      for (size_t f = 0; f < NF; f++, acc.bump()) {
        if (mask[i * NF + f]) continue;
        const double s = (free_slot ? empty : groups[k])[f]->score_value(*hy[f], acc.get(), rng);
        v += s;
        m += std::max(1.0, std::fabs(s));
      }
      t.push_back(v);
      mag = std::max(mag, m);
    }
    double top = t[0];
    size_t arg = 0;
    for (size_t k = 1; k < t.size(); k++)
      if (t[k] > top) top = t[k], arg = k;
    double sum = 0, second = -INFINITY;
    for (size_t k = 0; k < t.size(); k++) {
      sum += (k + 1 == t.size() ? double(nfree) : 1.0) * std::exp(t[k] - top);     // (the free slots are nfree equal terms)
      if (k != arg) second = std::max(second, t[k]);
    }
    const double lse = top + std::log(sum), want = lse - norm, E = 1e-6 * mag;
    CHECK(audit::check("mixture_state.log_post_pred.logp", std::fabs(logp[i] - want) / (E + 1e-6 * std::fmax(1.0, std::fabs(want))), 1.0));
    const double want_lr = top - lse;
    CHECK(audit::check("mixture_state.log_post_pred.map_logresp", std::fabs(logresp[i] - want_lr) / (E + 1e-6 * std::fmax(1.0, std::fabs(want_lr))), 1.0));
    CHECK(logresp[i] <= 0.f && slots[i] >= 0 && size_t(slots[i]) < KMAX);
    // the MAP slot where the twin decides it: an occupied group clear of the runner-up by more than 2 E_r (among the free
    // slots, all equal, the lowest wins: not a question for the twin)
    if (arg < groups.size() && top - second > 2 * E) {
      CHECK(slots[i] == slot[arg]);
      decided++;
    }
  }
  CHECK(decided > M / 2);
  audit::dump();
  std::printf("test_log_post_pred_gpu ok: %zu rows, %zu MAP slots decided by the twin\n", M, decided);
  return 0;
}
