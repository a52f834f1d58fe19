// The C++ surface a downstream microbenchmark of the virtual group API is written against,
// used the ways such code uses it: a boolean row walked with row_accessor, noop and
// Beta-Bernoulli hypers / groups made through the model factories (shared_ptr), and the
// same families as arrays of the concrete distributions_hypers<T> / distributions_group<T>
// types, initialised through their public repr_ and driven through plain base pointers.
// Everything up to the device calls runs on the host; the device loop is compiled and
// linked always and run only with --device (each Beta-Bernoulli call is one launch).
#include <microscopes/common/random_fwd.hpp>
#include <microscopes/common/recarray/dataview.hpp>
#include <microscopes/common/timer.hpp>
#include <microscopes/models/distributions.hpp>
#include <microscopes/models/noop.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <vector>

using namespace distributions;
using namespace microscopes;
using namespace microscopes::common;
using namespace microscopes::common::recarray;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// one add / remove / score pass over every feature of the row, through whatever pointer type the caller holds
template <typename G, typename H>
static float pass(row_accessor &acc, G &groups, H &hypers, rng_t &r) {
  float score = 0.f;
  acc.reset();
  for (size_t i = 0; i < acc.nfeatures(); i++, acc.bump()) groups[i]->add_value(*hypers[i], acc.get(), r);
  acc.reset();
  for (size_t i = 0; i < acc.nfeatures(); i++, acc.bump()) groups[i]->remove_value(*hypers[i], acc.get(), r);
  acc.reset();
  for (size_t i = 0; i < acc.nfeatures(); i++, acc.bump()) score += groups[i]->score_value(*hypers[i], acc.get(), r);
  return score;
}

int main(int argc, char **argv) {
  const bool device = argc > 1 && std::strcmp(argv[1], "--device") == 0;
  rng_t r(73);
  const size_t D = 64;

  // a row of D booleans, stored as the bool array a caller has at hand
  bool row[D];
  size_t ones = 0;
  for (size_t i = 0; i < D; i++) ones += (row[i] = std::bernoulli_distribution(0.5)(r));
  std::vector<runtime_type> types(D, runtime_type(TYPE_B));
  row_accessor acc(reinterpret_cast<const uint8_t *>(&row[0]), nullptr, &types);
  CHECK(acc.nfeatures() == D);
  size_t seen = 0, walked = 0;
  for (acc.reset(); !acc.end(); acc.bump(), walked++) seen += acc.get().get<bool>();
  CHECK(walked == D && seen == ones);

  // factories: shared_ptr hypers and groups
  std::vector<std::shared_ptr<models::hypers>> noop_hp, bb_hp;
  std::vector<std::shared_ptr<models::group>> noop_g, bb_g;
  for (size_t i = 0; i < D; i++) {
    noop_hp.emplace_back(models::noop_model().create_hypers());
    noop_g.emplace_back(noop_hp.back()->create_group(r));
    bb_hp.emplace_back(models::distributions_model<BetaBernoulli>().create_hypers());
    bb_hp.back()->get_hp_mutator("alpha").set<float>(2.0);
    bb_hp.back()->get_hp_mutator("beta").set<float>(2.0);
    bb_g.emplace_back(bb_hp.back()->create_group(r));
  }
  CHECK(pass(acc, noop_g, noop_hp, r) == 0.f);             // the noop model does no work, on the host

  // the concrete types, all D of them in one allocation each, initialised through repr_
  std::unique_ptr<models::distributions_hypers<BetaBernoulli>[]> flat_hp(new models::distributions_hypers<BetaBernoulli>[D]);
  std::unique_ptr<models::distributions_group<BetaBernoulli>[]> flat_g(new models::distributions_group<BetaBernoulli>[D]);
  std::vector<models::hypers *> hp_ptr;
  std::vector<models::group *> g_ptr;
  for (size_t i = 0; i < D; i++) {
    flat_hp[i].get_hp_mutator("alpha").set<float>(2.0);
    flat_hp[i].get_hp_mutator("beta").set<float>(2.0);
    CHECK(flat_hp[i].repr_.alpha == 2.f && flat_hp[i].repr_.beta == 2.f);
    flat_g[i].repr_.heads = 5;
    flat_g[i].repr_.init(flat_hp[i].repr_, r);
    CHECK(flat_g[i].repr_.heads == 0 && flat_g[i].repr_.tails == 0);
    hp_ptr.emplace_back(&flat_hp[i]);
    g_ptr.emplace_back(&flat_g[i]);
  }

  if (device) {
    timer tt;
    const float a = pass(acc, bb_g, bb_hp, r), b = pass(acc, g_ptr, hp_ptr, r);
    // the same suff-stats (empty after add + remove) and hyperparameters on both paths: the same scores
    CHECK(a == b && a < 0.f);
    std::cout << "device passes took " << tt.lap_ms() << " ms" << std::endl;
  }
  std::cout << "test_drop_in_surface ok" << std::endl;
  return 0;
}
