// The host route of posterior predictive sampling, timed per entry: group::sample_value of the C++ plugin layer
// (include/microscopes_amd/hip_models.hpp detail::sampler, driven by the caller's rng_t) on the C3 feature mix
// (16 each of bb, gp, dd(32), nich; K groups with suff-stats of ~rows/K values each), one entry at a time with a random
// (feature, group) per entry, as a downstream imputation loop calls it.  Built and run by tools/bench_predictive.py.
//   bench_host_sample <entries> <K> <rows>   ->   one JSON line {"host_us_per_entry": ...}
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <microscopes/models/distributions.hpp>

using namespace microscopes;
using namespace microscopes::common;

int main(int argc, char **argv) {
  const size_t entries = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 200000;
  const size_t K = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 256;
  const size_t rows = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : (1u << 20);
  rng_t rng(1);
  std::mt19937 gen(2);
  std::vector<models::model_shared_ptr> mdl;
  for (int i = 0; i < 16; i++) {
    mdl.push_back(std::make_shared<models::distributions_model<distributions::BetaBernoulli>>());
    mdl.push_back(std::make_shared<models::distributions_model<distributions::GammaPoisson>>());
    mdl.push_back(std::make_shared<models::distributions_model_dd128>(32));
    mdl.push_back(std::make_shared<models::distributions_model<distributions::NormalInverseChiSq>>());
  }
  std::vector<models::hypers_shared_ptr> hyp;
  std::vector<std::vector<std::shared_ptr<models::group>>> grp(mdl.size());
  std::poisson_distribution<uint32_t> per(double(rows) / double(K));
  for (size_t f = 0; f < mdl.size(); f++) {
    hyp.push_back(mdl[f]->create_hypers());
    for (size_t k = 0; k < K; k++) {
      auto g = hyp[f]->create_group(rng);
      const uint32_t n = per(gen);
      switch (f % 4) {
        case 0: g->get_ss_mutator("heads").set<uint32_t>(n / 3); g->get_ss_mutator("tails").set<uint32_t>(n - n / 3); break;
        case 1: g->get_ss_mutator("count").set<uint32_t>(n); g->get_ss_mutator("sum").set<uint32_t>(3 * n); break;
        case 2:
          for (int i = 0; i < 32; i++) g->get_ss_mutator("counts").set<uint32_t>(n / 32, i);
          g->get_ss_mutator("count_sum").set<uint32_t>(n / 32 * 32);
          break;
        default:
          g->get_ss_mutator("count").set<uint32_t>(n);
          g->get_ss_mutator("mean").set<float>(float(k % 7));
          g->get_ss_mutator("count_times_variance").set<float>(float(n));
      }
      grp[f].push_back(g);
    }
  }
  std::vector<std::pair<uint32_t, uint32_t>> picks(entries);
  for (auto &p : picks) p = {uint32_t(gen() % mdl.size()), uint32_t(gen() % K)};
  uint8_t buf[16];
  double sink = 0.0;
  auto run = [&](size_t n) {
    for (size_t i = 0; i < n; i++) {
      const auto &p = picks[i];
      value_mutator m(buf, mdl[p.first]->get_runtime_type());
      grp[p.first][p.second]->sample_value(*hyp[p.first], m, rng);
      sink += buf[0];
    }
  };
  run(entries / 10);                                      // warm-up
  const auto t0 = std::chrono::steady_clock::now();
  run(entries);
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"host_us_per_entry\": %.5f, \"entries\": %zu, \"sink\": %.1f}\n", us / double(entries), entries, sink);
  return 0;
}
