// mixture_state::sample_post_pred: new, partly observed rows get a group from the CRP term plus their observed scores and
// their masked entries drawn from that group.  Checked here: observed bytes come back unchanged, masked values are of
// their field's range, groups are slots of the table.  With a directory argument the program also writes the rows, the
// answer and the state's device tables there, so that tests/test_gpu_predictive_cxx.py can make the same call through
// Python (State.impute) and compare.
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
  const size_t N = 2000, M = 3000, KMAX = 16, NF = 4;
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
  iface.get_cluster_hp_mutator("alpha").set<float>(1.0f);
  st.assign_all(labels, rng);

  // the new rows: every feature masked in about a third of them
  std::vector<uint8_t> mask(M * NF);
  for (auto &m : mask) m = std::bernoulli_distribution(0.35)(gen);
  recarray::row_major_dataview q(reinterpret_cast<const uint8_t *>(fresh.data()), reinterpret_cast<const bool *>(mask.data()),
                                 M, types);
  std::vector<int32_t> groups;
  const uint64_t seed = 77, sweep = 4;
  const std::vector<uint8_t> out = st.sample_post_pred(q, seed, sweep, &groups);
  CHECK(out.size() == M * sizeof(Row) && groups.size() == M);
  const size_t off[NF] = {0, 1, 5, 9}, sz[NF] = {1, 4, 4, 4};
  size_t drawn = 0;
  for (size_t i = 0; i < M; i++) {
    CHECK(groups[i] >= 0 && size_t(groups[i]) < KMAX);
    const uint8_t *a = out.data() + i * sizeof(Row), *b = reinterpret_cast<const uint8_t *>(&fresh[i]);
    for (size_t f = 0; f < NF; f++) {
      if (!mask[i * NF + f]) {
        CHECK(std::memcmp(a + off[f], b + off[f], sz[f]) == 0);      // observed: the very bytes
        continue;
      }
      drawn++;
      Row r;
      std::memcpy(&r, a, sizeof(Row));
      if (f == 0) CHECK(a[0] == 0 || a[0] == 1);
      if (f == 2) CHECK(std::isfinite(r.x));
      if (f == 3) CHECK(r.d >= 0 && r.d < 4);
    }
  }
  CHECK(drawn > M);
  // the same call twice: the same bytes (counter-based draws)
  std::vector<int32_t> groups2;
  CHECK(st.sample_post_pred(q, seed, sweep, &groups2) == out && groups2 == groups);

  if (!dir.empty()) {
    put(dir, "rows.bin", fresh.data(), M * sizeof(Row));
    put(dir, "mask.bin", mask.data(), mask.size());
    put(dir, "out.bin", out.data(), out.size());
    put(dir, "groups.bin", groups.data(), 4 * M);
    msc_state *s = st.device_state();
    for (uint32_t f = 0; f < NF; f++) {
      msc_feature_spec spec = {0, 0};
      spec.family = f == 0 ? MSC_BB : f == 1 ? MSC_GP : f == 2 ? MSC_NICH : MSC_DD;
      spec.dim = f == 3 ? 4 : 0;
      std::vector<float> hp(msc_hp_floats(spec.family, spec.dim));
      CHECK(msc_state_get_hp(s, f, hp.data(), hp.size()) == MSC_OK);
      std::vector<uint8_t> ss(KMAX * msc_ss_bytes(spec.family, spec.dim));
      CHECK(msc_state_get_ss(s, f, 0, KMAX, ss.data(), ss.size()) == MSC_OK);
      put(dir, ("hp" + std::to_string(f) + ".bin").c_str(), hp.data(), 4 * hp.size());
      put(dir, ("ss" + std::to_string(f) + ".bin").c_str(), ss.data(), ss.size());
    }
    std::vector<uint32_t> cnt(KMAX);
    CHECK(msc_state_get_group_counts(s, cnt.data(), KMAX) == MSC_OK);
    put(dir, "counts.bin", cnt.data(), 4 * KMAX);
  }
  std::printf("test_predictive_gpu ok: %zu masked entries drawn\n", drawn);
  return 0;
}
