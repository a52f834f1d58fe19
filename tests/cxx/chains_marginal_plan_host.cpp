// chains_marginal_plan_host.cpp -- the tile plan msc_chains_score_marginal makes for a state (route_calls.hpp
// plan_chains_marginal, host-only code), printed for a feature list given on the command line:
//   chains_marginal_plan_host K family dim vcap [family dim vcap ...]
// -> one line "TG TS lds_floats wide large" and one "f off rows" a feature (off -1: its tables stay in global memory).
// tests/heavy_chain_cases.py asks it which instantiation of k_chains_marginal a heavy state takes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "route_calls.hpp"

int main(int argc, char **argv) {
  using namespace msc;
  if (argc < 5 || (argc - 2) % 3 != 0) {
    std::fprintf(stderr, "usage: %s K family dim vcap [family dim vcap ...]\n", argv[0]);
    return 2;
  }
  const uint32_t K = (uint32_t)std::strtoul(argv[1], nullptr, 10);
  std::vector<RouteFeat> feats;
  for (int i = 2; i + 2 < argc; i += 3) {
    RouteFeat f;
    f.family = std::atoi(argv[i]);
    f.dim = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
    f.vcap = (uint32_t)std::strtoul(argv[i + 2], nullptr, 10);
    feats.push_back(f);
  }
  std::vector<uint32_t> sel(feats.size());
  for (uint32_t i = 0; i < sel.size(); i++) sel[i] = i;
  std::vector<MargFeat> out(feats.size());
  const CmPlan p = plan_chains_marginal(feats.data(), sel.data(), (uint32_t)sel.size(), K, out.data());
  std::printf("%u %u %u %d %d\n", p.TG, p.TS, p.lds_floats, (int)p.wide, (int)p.large);
  for (const MargFeat &m : out) std::printf("%u %d %u\n", m.f, m.off == kCmNotStaged ? -1 : (int)m.off, m.rows);
  return 0;
}
