// mixture_state's grid hyper-parameter extension: score_likelihood_grid against score_likelihood at each point,
// grid_component_hp installing the chosen point (get_component_hp, and the likelihood the state then reports),
// grid_cluster_hp updating alpha.
#include <cmath>
#include <cstdio>
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

int main() {
  rng_t rng(3);
  const size_t N = 400, KMAX = 16;
  std::vector<Row> rows(N);
  std::mt19937 gen(7);
  std::vector<size_t> labels(N);
  for (size_t i = 0; i < N; i++) {
    const int comp = int(i % 4);
    labels[i] = size_t(comp);
    rows[i].b = std::bernoulli_distribution(0.15 + 0.2 * comp)(gen);
    rows[i].c = uint32_t(std::poisson_distribution<int>(1 + 3 * comp)(gen));
    rows[i].x = float(std::normal_distribution<double>(2.0 * comp, 1.0)(gen));
  }
  const std::vector<runtime_type> types = {runtime_type(TYPE_B), runtime_type(TYPE_U32), runtime_type(TYPE_F32)};
  recarray::row_major_dataview data(reinterpret_cast<const uint8_t *>(rows.data()), nullptr, N, types);
  std::vector<models::model_shared_ptr> mdl = {
      std::make_shared<models::distributions_model<distributions::BetaBernoulli>>(),
      std::make_shared<models::distributions_model<distributions::GammaPoisson>>(),
      std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>()};
  hip::mixture_state st(mdl, data, KMAX);
  entity_based_state_object &iface = st;
  iface.get_cluster_hp_mutator("alpha").set<float>(1.0f);
  st.assign_all(labels, rng);
  const size_t empty_gid = iface.create_group(rng);          // an empty group counts, as in score_likelihood
  (void)empty_gid;

  // bb: 40 (alpha, beta) points; gp: 30; nich: 25 (mu, kappa, sigmasq, nu)
  std::uniform_real_distribution<float> u(0.2f, 6.f);
  const size_t npts[3] = {40, 30, 25};
  const size_t nfl[3] = {2, 2, 4};
  for (size_t c = 0; c < 3; c++) {
    std::vector<float> blocks(npts[c] * nfl[c]);
    for (float &v : blocks) v = u(gen);
    std::vector<double> logprior(npts[c]);
    for (size_t g = 0; g < npts[c]; g++) logprior[g] = -0.1 * double(g % 7);
    const std::vector<double> lik = st.score_likelihood_grid(c, blocks);
    CHECK(lik.size() == npts[c]);
    const size_t k = st.grid_component_hp(c, blocks, logprior, 17, c);
    CHECK(k < npts[c]);
    // the chosen point is the component's hp now ...
    static const char *const keys[3][4] = {{"alpha", "beta"}, {"alpha", "inv_beta"}, {"mu", "kappa", "sigmasq", "nu"}};
    for (size_t i = 0; i < nfl[c]; i++)
      CHECK(iface.get_component_hp_mutator(c, keys[c][i]).accessor().get<float>(0) == blocks[k * nfl[c] + i]);
    // ... and the likelihood the state reports (a float sum over its groups) is the chosen point's grid score
    const double got = iface.score_likelihood(c, rng);
    CHECK(audit::sum("hp_grid.mixture_state.score_likelihood_after_grid_step", got, lik[k], double(iface.ngroups())));
  }

  // alpha
  std::vector<float> alphas(20);
  for (size_t i = 0; i < alphas.size(); i++) alphas[i] = 0.1f * float(i + 1);
  const size_t ka = st.grid_cluster_hp(alphas, std::vector<double>(), 5, 0);
  CHECK(ka < alphas.size());
  CHECK(iface.get_cluster_hp_mutator("alpha").accessor().get<float>(0) == alphas[ka]);
  st.gibbs_sweep(5, 1, rng);                                 // (pushes nothing back: the device already holds the point)
  CHECK(iface.get_cluster_hp_mutator("alpha").accessor().get<float>(0) == alphas[ka]);
  audit::dump();
  std::printf("test_hp_grid_gpu ok\n");
  return 0;
}
