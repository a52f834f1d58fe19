// mixture_state::score_joint(): the double log joint of a small mixed state equals msc_score_joint's total on the
// state's device handle bit for bit, and agrees with the float virtuals it replaces (score_assignment + the components'
// score_likelihood) at their float tolerance; a sweep and a membership edit move it, and it follows.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

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
};
#pragma pack(pop)

// msc_score_joint on the handle itself, no mask: the non-empty slots, which are the partition's when it holds no empty group
static int abi_row(hip::mixture_state &st, msc_context *ctx, double *row, size_t w) {
  double *out_dev = nullptr;
  if (msc_device_alloc(ctx, 8 * w, reinterpret_cast<void **>(&out_dev)) != MSC_OK) return 1;
  int rc = msc_score_joint(st.device_state(), nullptr, 0, nullptr, out_dev);
  if (rc == MSC_OK) rc = msc_device_download(ctx, row, out_dev, 8 * w);
  msc_device_free(ctx, out_dev);
  return rc;
}

int main() {
  rng_t rng(3);
  const size_t N = 300, KMAX = 12;
  std::vector<Row> rows(N);
  std::mt19937 gen(11);
  std::vector<size_t> labels(N);
  for (size_t i = 0; i < N; i++) {
    const int comp = int(i % 5);
    labels[i] = size_t(comp);
    rows[i].b = std::bernoulli_distribution(0.1 + 0.18 * comp)(gen);
    rows[i].c = uint32_t(std::poisson_distribution<int>(1 + 2 * comp)(gen));
    rows[i].x = float(std::normal_distribution<double>(1.5 * comp, 1.0)(gen));
  }
  const std::vector<runtime_type> types = {runtime_type(TYPE_B), runtime_type(TYPE_U32), runtime_type(TYPE_F32)};
  recarray::row_major_dataview data(reinterpret_cast<const uint8_t *>(rows.data()), nullptr, N, types);
  std::vector<models::model_shared_ptr> mdl = {
      std::make_shared<models::distributions_model<distributions::BetaBernoulli>>(),
      std::make_shared<models::distributions_model<distributions::GammaPoisson>>(),
      std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>()};
  msc_context *ctx = hip::default_context();
  hip::mixture_state st(mdl, data, KMAX, ctx);
  entity_based_state_object &iface = st;
  iface.get_cluster_hp_mutator("alpha").set<float>(1.75f);
  iface.get_component_hp_mutator(2, "kappa").set<float>(0.375f);
  st.assign_all(labels, rng);

  const size_t W = 3 + 3;
  for (int round = 0; round < 3; round++) {
    const double got = st.score_joint();
    double row[W];
    CHECK(abi_row(st, ctx, row, W) == 0);
    CHECK(std::isfinite(got));
    // (after a sweep the partition may hold a group the sweep emptied, which the call without a mask does not count)
    if (round == 0) CHECK(std::memcmp(&got, &row[0], 8) == 0);
    else CHECK(audit::score("joint.mixture_state.score_joint_vs_abi_total", got, row[0]));
    const double parts = ((row[1] + row[2]) + row[3]) + row[4];
    CHECK(row[5] == 0.0 && parts + row[5] == row[0]);
    // the float virtuals it replaces
    double want = iface.score_assignment(), mag = std::fmax(1.0, std::fabs(want));
    for (size_t c = 0; c < 3; c++) {
      const double l = iface.score_likelihood(c, rng);
      want += l;
      mag += std::fmax(1.0, std::fabs(l)) * double(iface.ngroups());     // (a float sum over the groups each)
    }
    CHECK(audit::sum("joint.mixture_state.score_joint_vs_float_virtuals", got, want, mag));
    CHECK(audit::score("joint.mixture_state.score_assignment", row[1], iface.score_assignment()));
    CHECK(st.score_joint() == got);                            // a call repeats its bits and changes nothing
    if (round == 0) {
      st.gibbs_sweep(5, 1, rng);
      CHECK(st.score_joint() != got);
    } else if (round == 1) {                                   // a membership edit: the number follows
      const size_t gid = size_t(iface.assignments()[7]);
      iface.remove_value(7, rng);
      CHECK(st.score_joint() != got);
      iface.add_value(gid, 7, rng);
    }
  }
  audit::dump();
  std::printf("test_score_joint_gpu ok\n");
  return 0;
}
