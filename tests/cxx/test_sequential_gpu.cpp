// mixture_state::gibbs_sweep_sequential: the sequential Gibbs sweep through the reference's state interface.  Checked
// here: afterwards the host partition (rebuilt from the device's assignment vector) has every entity in a group and every
// group's size equal to the device's count of its slot; an entity removed through the per-entity interface is seated.
// With a directory argument the program writes the rows, the assignment before and after and the hypers there, so that
// tests/test_gpu_sequential_cxx.py can make the same call through Python (State.sweep_sequential) and compare.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

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
  uint32_t c;
  float x;
  int32_t d;
};
#pragma pack(pop)

static void put(const std::string &dir, const char *name, const void *p, size_t n) {
  if (dir.empty()) return;
  FILE *f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f) return;
  std::fwrite(p, 1, n, f);
  std::fclose(f);
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : "";
  rng_t rng(3);
  const size_t N = 1500, KMAX = 24, NF = 4;
  std::mt19937 gen(5);
  std::vector<Row> rows(N);
  std::vector<size_t> labels;
  for (size_t i = 0; i < N; i++) {
    const int comp = int(gen() % 4);
    labels.push_back(size_t(gen() % 6));               // a poor start: six groups that ignore the components
    rows[i].b = std::bernoulli_distribution(0.1 + 0.25 * comp)(gen);
    rows[i].c = uint32_t(std::poisson_distribution<int>(1 + 4 * comp)(gen));
    rows[i].x = float(std::normal_distribution<double>(3.0 * comp, 1.0)(gen));
    rows[i].d = int32_t((comp + gen() % 2) % 4);
  }
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
  iface.get_cluster_hp_mutator("alpha").set<float>(1.0f);
  st.assign_all(labels, rng);
  auto slots = [&]() {
    std::vector<int32_t> z(N);
    const std::vector<ssize_t> a = iface.assignments();
    for (size_t e = 0; e < N; e++) z[e] = a[e] < 0 ? -1 : int32_t(st.slot_of(size_t(a[e])));
    return z;
  };
  const std::vector<int32_t> z0 = slots();
  // one entity taken out through the per-entity interface: the sweep seats it
  iface.remove_value(7, rng);
  std::vector<int32_t> zin = slots();
  CHECK(zin[7] == -1);
  const uint64_t seed = 31, sweep = 5;
  st.gibbs_sweep_sequential(seed, sweep, rng, 2);
  // the host partition, rebuilt from the device's assignment vector: every entity in a group, and every group's size
  // the device's count of its slot
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

  if (!dir.empty()) {
    put(dir, "rows.bin", rows.data(), N * sizeof(Row));
    put(dir, "z0.bin", z0.data(), 4 * N);
    put(dir, "z_in.bin", zin.data(), 4 * N);
    put(dir, "z_out.bin", z1.data(), 4 * N);
    msc_state *s = st.device_state();
    for (uint32_t f = 0; f < NF; f++) {
      msc_feature_spec spec = {0, 0};
      spec.family = f == 0 ? MSC_BB : f == 1 ? MSC_GP : f == 2 ? MSC_NICH : MSC_DD;
      spec.dim = f == 3 ? 4 : 0;
      std::vector<float> hp(msc_hp_floats(spec.family, spec.dim));
      CHECK(msc_state_get_hp(s, f, hp.data(), hp.size()) == MSC_OK);
      put(dir, ("hp" + std::to_string(f) + ".bin").c_str(), hp.data(), 4 * hp.size());
    }
  }
  std::printf("test_sequential_gpu ok: %zu of %zu entities moved\n", moved, N);
  return 0;
}
