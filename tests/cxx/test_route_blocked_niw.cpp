// Host test of the niw rule of route_blocked (common_amd/csrc/route_calls.hpp): a state whose only feature is one niw
// column of dim <= 32 takes BlockedKernel::niw1 in the blocked sweep, and nothing else about niw changed -- beyond dim 32 a
// refusal of its own, split-merge and a niw feature beside others refused in the words they always were.  No device.
#include <string>

#include "plan_cases.hpp"
#include "route_calls.hpp"

using namespace cases;

static RouteFacts one_niw(uint32_t dim, uint32_t K = 16) {
  RouteFacts rf;
  rf.K = K, rf.kpad = (K + kGroupTile - 1) / kGroupTile * kGroupTile, rf.nfeat = 1, rf.n_niw = 1;
  rf.feats.assign(1, RouteFeat{MSC_NIW, dim, 0, false});
  return rf;
}

static const char *const kOld = " takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)";

int main() {
  for (uint32_t dim : {1u, 2u, 16u, 17u, 32u}) {
    const BlockedRoute r = route_sweep_blocked(one_niw(dim));
    CHECK(r.rc == MSC_OK && r.why.empty() && r.kernel == BlockedKernel::niw1 && r.block == 256);
    const BlockedRoute q = route_splitmerge(one_niw(dim));
    CHECK(q.rc == MSC_EUNSUPPORTED && q.why == std::string("split-merge") + kOld);
    const SeqRoute s = route_sequential(one_niw(dim));
    CHECK(s.rc == MSC_EUNSUPPORTED &&
          std::string(s.why) == "the sequential sweep takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
  }
  CHECK(blocked::kNiwMaxDim == 32u);
  for (uint32_t dim : {33u, 64u, 128u}) {
    const BlockedRoute r = route_sweep_blocked(one_niw(dim));
    CHECK(r.rc == MSC_EUNSUPPORTED && r.why == "the blocked sweep takes a niw feature of dimension at most 32");
    const BlockedRoute q = route_splitmerge(one_niw(dim));
    CHECK(q.rc == MSC_EUNSUPPORTED && q.why == std::string("split-merge") + kOld);
  }
  // a niw feature beside others, wherever it stands and whatever its dimension: the old refusal from both callers
  for (uint32_t at : {0u, 1u, 2u})
    for (uint32_t dim : {2u, 33u}) {
      RouteFacts rf = one_niw(dim);
      rf.nfeat = 3;
      rf.feats.assign(3, RouteFeat{MSC_BB, 0, 0, false});
      rf.feats[at] = RouteFeat{MSC_NIW, dim, 0, false};
      const BlockedRoute r = route_sweep_blocked(rf), q = route_splitmerge(rf);
      CHECK(r.rc == MSC_EUNSUPPORTED && r.why == std::string("the blocked sweep") + kOld);
      CHECK(q.rc == MSC_EUNSUPPORTED && q.why == std::string("split-merge") + kOld);
    }
  {                                                     // two niw features are "beside others" too; dm and bbnc alone stay refused
    RouteFacts rf = one_niw(2);
    rf.nfeat = 2, rf.n_niw = 2;
    rf.feats.push_back(RouteFeat{MSC_NIW, 2, 0, false});
    CHECK(route_sweep_blocked(rf).rc == MSC_EUNSUPPORTED && route_sweep_blocked(rf).why == std::string("the blocked sweep") + kOld);
    for (int fam : {MSC_DM, MSC_BBNC}) {
      RouteFacts one = one_niw(4);
      one.n_niw = 0, one.feats[0].family = fam;
      CHECK(route_sweep_blocked(one).rc == MSC_EUNSUPPORTED && route_sweep_blocked(one).why == std::string("the blocked sweep") + kOld);
    }
  }
  // the other single-column routes are what they were
  {
    RouteFacts rf = one_niw(0);
    rf.n_niw = 0, rf.feats[0].family = MSC_NICH;
    CHECK(route_sweep_blocked(rf).kernel == BlockedKernel::nich1 && route_splitmerge(rf).kernel == BlockedKernel::nich1);
    rf.feats[0].family = MSC_BB;
    CHECK(route_sweep_blocked(rf).kernel == BlockedKernel::staged);
  }
  if (g_failures) return 1;
  std::printf("route blocked niw ok\n");
  return 0;
}
