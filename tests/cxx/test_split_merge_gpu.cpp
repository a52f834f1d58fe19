// mixture_state::split_merge: split-merge proposals through the reference's state interface, on two nich clusters at
// -10 / +10 (sd 1) with a bb column of p = 0.1 / 0.9, 1500 rows.  Checked here: from one group, proposals until one split
// is accepted -- the host partition (rebuilt from the device's assignment vector) then has two groups whose sizes are the
// device's counts; from the truth cut into two groups a cluster, proposals until one merge is accepted -- three groups;
// the counters add up; and score_data of every group before and after against plugin groups fed the state's own
// suff-stats, at the audit gate.  A bbnc component throws.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>

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
  float x;
  bool b;
};
#pragma pack(pop)

static const size_t N = 1500, KMAX = 8;

// every group's score_data of both components against plugin groups fed the state's own suff-stats; the groups' sizes
// against the device's counts
static int check_state(hip::mixture_state &st, std::vector<models::hypers_shared_ptr> &hy, rng_t &rng, size_t want_groups) {
  entity_based_state_object &iface = st;
  std::vector<uint32_t> cnt(KMAX);
  size_t occupied = 0, total = 0;
  for (size_t gid : iface.groups()) occupied += iface.groupsize(gid) > 0;
  CHECK(occupied == want_groups);
  CHECK(msc_state_get_group_counts(st.device_state(), cnt.data(), KMAX) == MSC_OK);
  for (size_t gid : iface.groups()) {
    CHECK(iface.groupsize(gid) == cnt[st.slot_of(gid)]);
    total += iface.groupsize(gid);
    for (size_t f = 0; f < 2; f++) {
      auto own = hy[f]->create_group(rng);
      own->set_ss(iface.get_suffstats(f, gid));
      CHECK(audit::score("split_merge.score_likelihood.component_group", iface.score_likelihood(f, gid, rng),
                         own->score_data(*hy[f], rng)));
    }
  }
  CHECK(total == N);
  return 0;
}

int main() {
  rng_t rng(3);
  std::mt19937 gen(5);
  std::vector<Row> rows(N);
  std::vector<size_t> truth(N);
  for (size_t i = 0; i < N; i++) {
    truth[i] = gen() % 2;
    rows[i].x = float(std::normal_distribution<double>(truth[i] ? 10.0 : -10.0, 1.0)(gen));
    rows[i].b = std::bernoulli_distribution(truth[i] ? 0.9 : 0.1)(gen);
  }
  const std::vector<runtime_type> types = {runtime_type(TYPE_F32), runtime_type(TYPE_B)};
  recarray::row_major_dataview data(reinterpret_cast<const uint8_t *>(rows.data()), nullptr, N, types);
  std::vector<models::model_shared_ptr> mdl = {
      std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>(),
      std::make_shared<models::distributions_model<distributions::BetaBernoulli>>()};
  std::vector<models::hypers_shared_ptr> hy;
  for (auto &m : mdl) hy.push_back(m->create_hypers());

  // one accepted split, from a single group
  {
    hip::mixture_state st(mdl, data, KMAX);
    st.get_cluster_hp_mutator("alpha").set<float>(1.0f);
    st.assign_all(std::vector<size_t>(N, 0), rng);
    if (check_state(st, hy, rng, 1)) return 1;
    hip::mixture_state::split_merge_counts all;
    for (uint64_t p = 0; p < 60 && all.splits_accepted == 0; p++) {
      const auto c = st.split_merge(41, p, rng, 1, 3);
      CHECK(c.splits + c.merges + c.voids == 1 && c.merges == 0 && c.voids == 0);   // one group: every proposal is a split
      CHECK(c.splits_accepted <= c.splits);
      all.splits += c.splits, all.splits_accepted += c.splits_accepted;
    }
    CHECK(all.splits_accepted == 1);
    if (check_state(st, hy, rng, 2)) return 1;
    std::printf("one split accepted after %llu proposals\n", (unsigned long long)all.splits);
  }
  // one accepted merge, from the truth cut into two groups a cluster
  {
    hip::mixture_state st(mdl, data, KMAX);
    st.get_cluster_hp_mutator("alpha").set<float>(1.0f);
    std::vector<size_t> labels(N);
    for (size_t i = 0; i < N; i++) labels[i] = 2 * truth[i] + i % 2;
    st.assign_all(labels, rng);
    if (check_state(st, hy, rng, 4)) return 1;
    hip::mixture_state::split_merge_counts all;
    uint64_t p = 0;
    for (; p < 60 && all.merges_accepted == 0; p++) {
      const auto c = st.split_merge(43, p, rng, 1, 3);
      CHECK(c.splits + c.merges + c.voids == 1 && c.voids == 0);
      all.splits_accepted += c.splits_accepted, all.merges += c.merges, all.merges_accepted += c.merges_accepted;
    }
    CHECK(all.merges_accepted == 1);
    if (check_state(st, hy, rng, 3 + all.splits_accepted)) return 1;
    // several proposals in one call: the counters add up
    const auto c = st.split_merge(43, p, rng, 10, 3);
    CHECK(c.splits + c.merges + c.voids == 10 && c.splits_accepted <= c.splits && c.merges_accepted <= c.merges);
    if (check_state(st, hy, rng, 3 + all.splits_accepted + c.splits_accepted - c.merges_accepted)) return 1;
    std::printf("one merge accepted after %llu proposals\n", (unsigned long long)p);
  }
  // a non-conjugate component: refused before anything runs
  {
    const size_t M = 64;
    std::vector<uint8_t> bits(M);
    for (size_t i = 0; i < M; i++) bits[i] = uint8_t(i % 3 == 0);
    const std::vector<runtime_type> bt = {runtime_type(TYPE_B)};
    recarray::row_major_dataview bdata(bits.data(), nullptr, M, bt);
    std::vector<models::model_shared_ptr> bm = {std::make_shared<models::bbnc_model>()};
    hip::mixture_state bs(bm, bdata, 6);
    bs.get_cluster_hp_mutator("alpha").set<float>(1.f);
    std::vector<size_t> bl(M);
    for (size_t i = 0; i < M; i++) bl[i] = i % 2;
    bs.assign_all(bl, rng);
    bool threw = false;
    try {
      bs.split_merge(1, 0, rng);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    CHECK(threw);
  }
  audit::dump();
  std::printf("test_split_merge_gpu ok\n");
  return 0;
}
