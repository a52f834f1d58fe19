// mixture_state::gibbs_sweep_blocked: the blocked Gibbs sweep through the reference's state interface.  Checked here:
// after three sweeps over 500 rows of bb + nich the host partition (rebuilt from the device's assignment vector) has every
// entity in a group and every group's size equal to the device's count of its slot; a bbnc component throws.
#include <cstdio>
#include <random>
#include <stdexcept>

#include <microscopes/common/entity_state.hpp>
#include <microscopes/models/distributions.hpp>
#include <microscopes_amd/mixture_state.hpp>

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
  float x;
};
#pragma pack(pop)

int main() {
  rng_t rng(3);
  const size_t N = 500, KMAX = 32;
  std::mt19937 gen(5);
  std::vector<Row> rows(N);
  std::vector<size_t> labels;
  for (size_t i = 0; i < N; i++) {
    const int comp = int(gen() % 3);
    labels.push_back(size_t(gen() % 5));               // a poor start: five groups that ignore the components
    rows[i].b = std::bernoulli_distribution(0.1 + 0.4 * comp)(gen);
    rows[i].x = float(std::normal_distribution<double>(4.0 * comp, 1.0)(gen));
  }
  const std::vector<runtime_type> types = {runtime_type(TYPE_B), runtime_type(TYPE_F32)};
  recarray::row_major_dataview data(reinterpret_cast<const uint8_t *>(rows.data()), nullptr, N, types);
  std::vector<models::model_shared_ptr> mdl = {
      std::make_shared<models::distributions_model<distributions::BetaBernoulli>>(),
      std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>()};
  hip::mixture_state st(mdl, data, KMAX);
  entity_based_state_object &iface = st;
  iface.get_cluster_hp_mutator("alpha").set<float>(1.0f);
  st.assign_all(labels, rng);
  auto slots = [&]() {
    std::vector<int32_t> z(N);
    const std::vector<ssize_t> a = iface.assignments();
    for (size_t e = 0; e < N; e++) z[e] = a[e] < 0 ? -1 : int32_t(st.slot_of(size_t(a[e])));
    return z;
  };
  const std::vector<int32_t> z0 = slots();
  st.gibbs_sweep_blocked(31, 5, rng, 3);
  const std::vector<int32_t> z1 = slots();
  std::vector<uint32_t> cnt(KMAX);
  CHECK(msc_state_get_group_counts(st.device_state(), cnt.data(), KMAX) == MSC_OK);
  std::vector<uint32_t> seen(KMAX, 0);
  for (size_t e = 0; e < N; e++) {
    CHECK(z1[e] >= 0 && size_t(z1[e]) < KMAX);
    seen[size_t(z1[e])]++;
  }
  CHECK(seen == cnt);
  for (size_t gid : iface.groups()) CHECK(iface.groupsize(gid) == cnt[st.slot_of(gid)]);
  size_t moved = 0;
  for (size_t e = 0; e < N; e++) moved += z1[e] != z0[e];
  CHECK(moved > 0);

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
      bs.gibbs_sweep_blocked(1, 0, rng);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    CHECK(threw);
  }
  std::printf("test_blocked_gpu ok: %zu of %zu entities moved\n", moved, N);
  return 0;
}
