// Host test of common_amd/csrc/route_calls.hpp alone (plans come from tile_plan.hpp through plan_cases.hpp): what the
// blocked sweep, split-merge, the sequential sweep, the chain ensembles, the row predictive density and the partition
// summaries choose, against the rules written beside them.  A chip of 256 CUs unless a case says otherwise; no device.
// Every expectation is worked out from the rule (the arithmetic stands beside it), none from a run of the functions.
#include <cmath>
#include <string>
#include <type_traits>

#include "plan_cases.hpp"
#include "route_calls.hpp"

using namespace cases;

// THE SHARD RULE, by signature: the routes that decide bits take no argument that could carry the call's rows, and the
// tile plan takes neither rows nor the number of chains
static_assert(std::is_same<decltype(&route_marginal), MarginalKind (*)(const RouteFacts &, const Switches &)>::value,
              "route_marginal: the facts and the switches, nothing of the call");
static_assert(std::is_same<decltype(&route_chains_marginal), uint32_t (*)(uint32_t, uint64_t, int)>::value,
              "route_chains_marginal: chains, the view's rows, compute units");
static_assert(std::is_same<decltype(&plan_chains_marginal),
                           CmPlan (*)(const RouteFeat *, const uint32_t *, uint32_t, uint32_t, MargFeat *)>::value,
              "plan_chains_marginal: the features, the selection and K");

static RouteFacts facts(const Spec &s, uint32_t K, uint64_t view_rows, const Switches &sw = Switches()) {
  return facts_of(s, plan(s, K, true, sw), K, view_rows);
}
// n features of one family and nothing else: what the blocked and sequential routes read
static RouteFacts bare(uint32_t n, int family, uint32_t K = 16) {
  RouteFacts rf;
  rf.K = K, rf.kpad = (K + kGroupTile - 1) / kGroupTile * kGroupTile, rf.nfeat = n;
  rf.feats.assign(n, RouteFeat{family, 0, 0, false});
  return rf;
}

static void test_blocked() {
  {                                                     // one nich column: the register kernel, for both callers
    const RouteFacts rf = bare(1, MSC_NICH);
    CHECK(route_sweep_blocked(rf).rc == MSC_OK && route_sweep_blocked(rf).kernel == BlockedKernel::nich1);
    CHECK(route_splitmerge(rf).kernel == BlockedKernel::nich1);
    CHECK(route_sweep_blocked(bare(1, MSC_BB)).kernel == BlockedKernel::staged);   // (one column of another family is staged)
  }
  const struct { uint32_t n, block; } staged[] = {{32, 256}, {33, 128}, {64, 128}, {65, 64}};
  for (const auto &c : staged) {
    const BlockedRoute r = route_sweep_blocked(bare(c.n, MSC_BB)), q = route_splitmerge(bare(c.n, MSC_BB));
    CHECK(r.rc == MSC_OK && r.kernel == BlockedKernel::staged && r.block == c.block);
    CHECK(q.rc == MSC_OK && q.kernel == BlockedKernel::staged && q.block == c.block);
  }
  // kBlockedStagedMax = 256, kSplitMergeStagedMax = 255
  CHECK(route_sweep_blocked(bare(255, MSC_BB)).kernel == BlockedKernel::staged && route_splitmerge(bare(255, MSC_BB)).kernel == BlockedKernel::staged);
  CHECK(route_sweep_blocked(bare(256, MSC_BB)).kernel == BlockedKernel::staged && route_splitmerge(bare(256, MSC_BB)).kernel == BlockedKernel::global);
  CHECK(route_sweep_blocked(bare(256, MSC_BB)).block == 64);
  CHECK(route_sweep_blocked(bare(257, MSC_BB)).kernel == BlockedKernel::global && route_splitmerge(bare(257, MSC_BB)).kernel == BlockedKernel::global);
  CHECK(route_sweep_blocked(bare(257, MSC_BB)).rc == MSC_OK);
  for (int fam : {MSC_NIW, MSC_DM, MSC_BBNC}) {
    RouteFacts rf = bare(3, MSC_BB);
    rf.feats[2].family = fam;
    const BlockedRoute r = route_sweep_blocked(rf), q = route_splitmerge(rf);
    CHECK(r.rc == MSC_EUNSUPPORTED && q.rc == MSC_EUNSUPPORTED);
    CHECK(r.why == "the blocked sweep takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
    CHECK(q.why == "split-merge takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
  }
  CHECK(blocked::kStickTag == 32767u);
  CHECK(route_sweep_blocked(bare(32766, MSC_BB)).rc == MSC_OK);
  CHECK(route_sweep_blocked(bare(32767, MSC_BB)).rc == MSC_EUNSUPPORTED);
  CHECK(route_sweep_blocked(bare(32767, MSC_BB)).why == "the blocked sweep takes fewer than 32767 features");
  CHECK(route_splitmerge(bare(40000, MSC_BB)).why == "split-merge takes fewer than 32767 features");
}

static void test_sequential() {
  CHECK(route_sequential(bare(256, MSC_BB, 8192)).rc == MSC_OK && std::string(route_sequential(bare(256, MSC_BB, 8192)).why).empty());
  for (int fam : {MSC_NIW, MSC_DM, MSC_BBNC}) {
    RouteFacts rf = bare(2, MSC_NICH);
    rf.feats[0].family = fam;
    const SeqRoute r = route_sequential(rf);
    CHECK(r.rc == MSC_EUNSUPPORTED);
    CHECK(std::string(r.why) == "the sequential sweep takes bb, gp, bnb, dd, nich and noop features (the state holds niw, dm or bbnc)");
  }
  const SeqRoute f = route_sequential(bare(257, MSC_BB, 8192)), g = route_sequential(bare(256, MSC_BB, 8193));
  CHECK(f.rc == MSC_EUNSUPPORTED && std::string(f.why) == "the sequential sweep takes at most 256 features");
  CHECK(g.rc == MSC_EUNSUPPORTED && std::string(g.why) == "the sequential sweep takes at most 8192 groups");
  // a visit: 16 + 0.02 x 2 x entries + 0.007 K features.  One nich column, K = 16: 14 entries: 16 + 0.56 + 0.112
  CHECK(std::fabs(seq_visit_us(bare(1, MSC_NICH, 16)) - 16.672) < 1e-9);
  {                                                     // bb 4, gp(32) 68, dd(10) 22, nich 14, noop 0: 108 entries, K = 100, 5 features
    RouteFacts rf = bare(5, MSC_BB, 100);
    rf.feats[1] = RouteFeat{MSC_GP, 0, 32, false}, rf.feats[2] = RouteFeat{MSC_DD, 10, 0, false};
    rf.feats[3].family = MSC_NICH, rf.feats[4].family = MSC_NOOP;
    CHECK(std::fabs(seq_visit_us(rf) - (16.0 + 4.32 + 3.5)) < 1e-9);
  }
}

static void test_units_per_launch() {
  // one chain: max(1, min(10000, 20000 / unit_us)) cut to an integer -- the expression msc_sweep_sequential spelled out
  const struct { double us; uint64_t want; } one[] = {{0.5, 10000}, {2.0, 10000}, {16.3, 1226}, {20000.0, 1}, {1e9, 1}};   // 20000 / 16.3 = 1226.99
  for (const auto &c : one)
    for (int cus : {1, 104, 256, 304}) {
      CHECK(units_per_launch(1, cus, c.us) == c.want);
      CHECK(units_per_launch(1, cus, c.us) == (uint64_t)std::max(1.0, std::min(10000.0, 20000.0 / c.us)));
    }
  // the rounds of the grid: 256 chains on 256 CUs run in one, 257 in two (integer division), 513 in three
  CHECK(units_per_launch(256, 256, 16.3) == 1226 && units_per_launch(257, 256, 16.3) == 613 && units_per_launch(513, 256, 16.3) == 408);
  CHECK(units_per_launch(257, 256, 2.0) == 5000 && units_per_launch(257, 256, 4001.0) == 2);      // (20000 / 4001 = 4.99: 4 / 2)
  CHECK(units_per_launch(257, 256, 20000.0) == 1);      // 1 / 2 = 0: at least one
  for (uint32_t n : {1u, 2u, 255u, 256u, 257u, 100000u})
    for (int cus : {0, 1, 104, 256, 304})               // (a context that reports no compute units counts as one)
      for (double us : {1e-3, 0.5, 16.3, 19999.0, 20000.0, 1e12}) CHECK(units_per_launch(n, cus, us) >= 1);
}

static void test_marginal() {
  const Spec nich1 = Spec().nichs(1), roles = Spec().bbs(16).nichs(4);
  Spec tile;
  tile.bbs(4).nichs(8), tile.dd(200);                   // a generic feature: the plain tile kernels (test_route.cpp grid_specs)
  CHECK(route_marginal(facts(nich1, 1024, 100000), Switches()) == MarginalKind::nich1);
  CHECK(route_marginal(facts(nich1, 1024, 10), Switches()) == MarginalKind::nich1);             // (at every view size)
  CHECK(route_marginal(facts(nich1, 1025, 100000), Switches()) == MarginalKind::generic);
  CHECK(facts(tile, 256, 16384).plan.tile_path == MSC_PATH_TILE && facts(roles, 256, 100000).plan.tile_path == MSC_PATH_TILE_ROLES);
  CHECK(route_marginal(facts(tile, 256, 16384), Switches()) == MarginalKind::tile);             // kTailMinRows
  CHECK(route_marginal(facts(tile, 256, 16383), Switches()) == MarginalKind::generic);
  CHECK(route_marginal(facts(tile, 257, 16384), Switches()) == MarginalKind::generic);
  Switches on, off;
  on.marginal_tile = 1, off.marginal_tile = 0;
  CHECK(route_marginal(facts(roles, 256, 100000), Switches()) == MarginalKind::generic);
  CHECK(route_marginal(facts(roles, 256, 100000), on) == MarginalKind::tile);
  CHECK(route_marginal(facts(tile, 256, 100000), off) == MarginalKind::generic);
  CHECK(route_marginal(facts(tile, 256, 16383), on) == MarginalKind::generic);                  // (the switch forces no small view)
  {                                                     // dm, niw, a count beyond its table: generic whatever the switch says
    Spec dm, niw, g;
    dm.bbs(4).nichs(2), dm.dm(4, 40);
    niw.bbs(4), niw.add(MSC_NIW, 2, false, false);
    g.gp(100), g.bbs(4);
    for (const Switches &sw : {Switches(), on}) {
      CHECK(route_marginal(facts(dm, 64, 100000), sw) == MarginalKind::generic);
      CHECK(route_marginal(facts(niw, 64, 100000), sw) == MarginalKind::generic);
      RouteFacts rf = facts(g, 64, 100000);
      CHECK(route_marginal(rf, on) == MarginalKind::tile);
      rf.feats[0].beyond_table = true;
      CHECK(route_marginal(rf, sw) == MarginalKind::generic);
    }
  }
}

static void test_chains_marginal_cut() {
  // 256 CUs: 1024 workgroups wanted.  4100 rows are 17 blocks: ceil(1024 / 17) = 61 slices asked, ceil(71 / 61) = 2 chains
  // a slice, ceil(71 / 2) = 36 slices.  33000 rows are 129 blocks: ceil(1024 / 129) = 8, ceil(9 / 8) = 2, ceil(9 / 2) = 5.
  CHECK(route_chains_marginal(71, 4100, 256) == 36);
  CHECK(route_chains_marginal(9, 33000, 256) == 5);
  CHECK(route_chains_marginal(70, 65, 256) == 70);      // one block: a slice a chain
  for (uint32_t n : {1u, 2u, 3u, 70u, 2000u}) {
    CHECK(route_chains_marginal(n, 261888, 256) == std::min(n, 2u));     // 1023 blocks: ceil(1024 / 1023) = 2 ways
    CHECK(route_chains_marginal(n, 261889, 256) == 1);                   // 1024 blocks fill the chip
  }
  CHECK(route_chains_marginal(2000, 1, 256) == 1000);   // 1024 slices asked, 2 chains a slice: 1000, within the 1024
  CHECK(route_chains_marginal(1024, 1, 256) == 1024 && route_chains_marginal(1025, 1, 256) == 513);
  for (uint32_t n : {1u, 2u, 3u, 9u, 70u, 71u, 255u, 1023u, 1024u, 1025u, 2000u, 4097u})
    for (uint64_t view : {0ull, 1ull, 65ull, 256ull, 257ull, 4100ull, 33000ull, 100000ull, 261888ull, 261889ull, 10000000ull})
      for (int cus : {1, 104, 256, 304}) {
        const uint32_t s = route_chains_marginal(n, view, cus), per = (n + s - 1) / s;   // (the launcher's chains a slice)
        CHECK(s >= 1 && s <= std::min(n, 1024u));
        CHECK((uint64_t)(s - 1) * per < n && (uint64_t)s * per >= n);   // every slice but the last full, the last not empty
      }
}

static CmPlan plan_all(const std::vector<RouteFeat> &fs, uint32_t K, std::vector<MargFeat> &out) {
  std::vector<uint32_t> sel(fs.size());
  for (uint32_t i = 0; i < sel.size(); i++) sel[i] = i;
  out.assign(fs.size(), MargFeat());
  return plan_chains_marginal(fs.data(), sel.data(), (uint32_t)sel.size(), K, out.data());
}
static void test_chains_marginal_plan() {
  const RouteFeat nich{MSC_NICH, 0, 0, false}, dd120{MSC_DD, 120, 0, false}, bb{MSC_BB, 0, 0, false}, noop{MSC_NOOP, 0, 0, false};
  std::vector<MargFeat> o;
  {                                                     // one nich column, K = 40: rows 2 + 6 = 8; (10240 - 32) / 8 - 1 = 1275 -> 40 -> whole batches of 32
    const CmPlan p = plan_all({nich}, 40, o);
    CHECK(p.TG == 32 && p.TS == 33 && p.wide && !p.large && p.lds_floats == 8 * 33 + 32 && p.lds_floats == 296);
    CHECK(o[0].f == 0 && o[0].off == 2 * 33 && o[0].off == 66 && o[0].rows == 6);
  }
  {                                                     // dd(120) x 3, nich, K = 40 (min tile 33 floats a row):
    const CmPlan p = plan_all({dd120, dd120, dd120, nich}, 40, o);
    CHECK(o[0].off == 2 * 33 && o[1].off == 122 * 33);  // (2 + 120) x 33 + 32 = 4058, (122 + 120) x 33 + 32 = 8018: staged
    CHECK(o[2].off == kCmNotStaged && o[2].rows == 120);   // (242 + 120) x 33 + 32 = 11978 > 10240
    CHECK(o[3].off == 242 * 33 && o[3].rows == 6);      // (242 + 6) x 33 + 32 = 8216: staged after it
    CHECK(p.TG == 32 && p.TS == 33 && p.wide && p.lds_floats == 248 * 33 + 32 && p.lds_floats == 8216);   // 10208 / 248 - 1 = 40 -> 32
  }
  {                                                     // K = 1: a tile of one group, one float a row
    const CmPlan p = plan_all({nich, bb}, 1, o);
    CHECK(p.TG == 1 && p.TS == 1 && !p.wide && p.lds_floats == 10 + 32 && o[0].off == 2 && o[1].off == 8);
  }
  {                                                     // a count column at the table's cap: the large-count forms; 1026 x 33 > 10240: not staged
    const CmPlan p = plan_all({RouteFeat{MSC_GP, 0, kGpMaxTable, true}, nich}, 40, o);
    CHECK(p.large && o[0].off == kCmNotStaged && o[0].rows == kGpMaxTable && o[1].off == 66);
    CHECK(!plan_all({RouteFeat{MSC_BNB, 0, kGpMaxTable - 1, false}}, 40, o).large);
    CHECK(plan_all({RouteFeat{MSC_BNB, 0, kGpMaxTable, false}}, 40, o).large);
  }
  {                                                     // noop: nothing to stage, nothing to read
    const CmPlan p = plan_all({noop, nich}, 40, o);
    CHECK(o[0].off == 0 && o[0].rows == 0 && o[1].off == 66 && p.lds_floats == 296);
  }
  {                                                     // a selection: the plan is of the selected features, by their state indices
    const std::vector<RouteFeat> fs = {dd120, nich, dd120, bb};
    const uint32_t sel[] = {1, 3};
    MargFeat out[2];
    const CmPlan p = plan_chains_marginal(fs.data(), sel, 2, 40, out);
    CHECK(out[0].f == 1 && out[0].off == 66 && out[1].f == 3 && out[1].off == 8 * 33 && out[1].rows == 2 && p.lds_floats == 10 * 33 + 32);
  }
  // the invariants, over feature lists and K
  std::vector<std::vector<RouteFeat>> lists = {{nich}, {bb}, {noop}, {dd120, dd120, dd120, nich}, {RouteFeat{MSC_GP, 0, kGpMaxTable, true}},
                                               {RouteFeat{MSC_DD, 300, 0, false}, nich}, {RouteFeat{MSC_GP, 0, 1000, false}, RouteFeat{MSC_BNB, 0, 5, false}}};
  lists.push_back(std::vector<RouteFeat>(40, bb));
  lists.push_back(std::vector<RouteFeat>(256, nich));
  {
    std::vector<RouteFeat> c3;                          // C3's mix
    for (int i = 0; i < 16; i++) c3.push_back(bb), c3.push_back(RouteFeat{MSC_GP, 0, 24, false}), c3.push_back(RouteFeat{MSC_DD, 32, 0, false}), c3.push_back(nich);
    lists.push_back(c3);
  }
  for (const auto &fs : lists)
    for (uint32_t K : {1u, 7u, 31u, 32u, 33u, 40u, 64u, 300u, 1000u, 8192u}) {
      const CmPlan p = plan_all(fs, K, o);
      const uint32_t batch = p.wide ? (uint32_t)kCmBatchWide : (uint32_t)kCmBatch;
      CHECK(p.TG >= 1 && p.TG <= K && p.TS == (p.TG | 1u));
      CHECK((uint64_t)p.lds_floats * 4 <= 64u * 1024u);
      CHECK(p.wide == (p.TG >= (uint32_t)kCmBatchWide));
      CHECK(p.TG <= batch || p.TG % batch == 0);        // whole batches once a tile exceeds one batch
      uint32_t end = 2 * p.TS;                          // the prior's two rows
      for (size_t i = 0; i < fs.size(); i++) {
        CHECK(o[i].f == i && o[i].rows == cm_table_rows(fs[i].family, fs[i].dim, fs[i].vcap));
        if (o[i].rows == 0) { CHECK(o[i].off == 0); continue; }
        if (o[i].off == kCmNotStaged) continue;
        CHECK(o[i].off >= end);                         // (staged in order: no block overlaps the one before)
        end = o[i].off + o[i].rows * p.TS;
      }
      CHECK(end <= p.lds_floats - (uint32_t)kCmBatchWide);
    }
}

static void test_chunks_and_batches() {
  // score_chunk: ld = min(kpad, K rounded up to 64); at most 4 GiB of scores; between one row and the call's
  const struct { uint32_t K, ld; } lds[] = {{1, 64}, {64, 64}, {300, 320}, {8192, 8192}};
  for (const auto &c : lds)
    for (uint64_t nrows : {1ull, 2ull, 1000ull, 1ull << 20, 1ull << 24, 1ull << 28, (1ull << 32) - 1}) {
      const uint32_t kpad = (c.K + 255) / 256 * 256;
      const ScoreChunk s = score_chunk(c.K, kpad, nrows);
      CHECK(s.ld == c.ld && s.ld == std::min<uint64_t>(kpad, (c.K + 63) / 64 * 64));
      CHECK(s.chunk >= 1 && s.chunk <= nrows && s.chunk * s.ld * 4 <= (4ull << 30));
      CHECK(s.chunk == nrows || (s.chunk + 1) * s.ld * 4 > (4ull << 30));       // (the whole call, or the largest chunk that fits)
    }
  CHECK(score_chunk(300, 512, 1ull << 28).chunk == 3355443);    // 2^32 / 1280 = 3355443.2
  CHECK(score_chunk(64, 256, 1000).chunk == 1000);
  // pred_chunk: doubles from 4096 while the rows, 2^18 and 256 MiB of [nchains][chunk] floats allow the next size
  CHECK(pred_chunk(1, 1) == 4096 && pred_chunk(1, 4096) == 4096 && pred_chunk(1, 4097) == 8192);
  CHECK(pred_chunk(256, 1000000) == (1u << 18));        // 2 x 131072 x 256 x 4 = 256 MiB: the last doubling
  CHECK(pred_chunk(1024, 1000000) == 65536);            // 2 x 32768 x 1024 x 4 = 256 MiB
  CHECK(pred_chunk(2000, 5000) == 8192);
  for (uint32_t n : {1u, 7u, 256u, 1024u, 2000u, 100000u})
    for (uint64_t nrows : {1ull, 4096ull, 4097ull, 100000ull, 262144ull, 262145ull, (1ull << 32) - 1}) {
      const uint64_t c = pred_chunk(n, nrows);
      const auto goes_on = [&](uint64_t x) { return x < nrows && x < (1ull << 18) && 2 * x * n * 4 <= (256ull << 20); };
      CHECK(c >= 4096 && c <= (1ull << 18) && (c & (c - 1)) == 0 && !goes_on(c));
      for (uint64_t x = 4096; x < c; x *= 2) CHECK(goes_on(x));
    }
  CHECK(chains_draw_batch(63, false) == 8 && chains_draw_batch(64, false) == 32 && chains_draw_batch(8192, false) == 32);
  CHECK(chains_draw_batch(63, true) == 8 && chains_draw_batch(64, true) == 8 && chains_draw_batch(8192, true) == 8);
}

static void test_summaries() {
  // the table in LDS up to 15 x 1024 = 15360 cells
  CHECK(route_pd_table(15, 1024) == PdRoute::lds && route_pd_table(1024, 15) == PdRoute::lds && route_pd_table(120, 128) == PdRoute::lds);
  CHECK(route_pd_table(15, 1025) == PdRoute::global && route_pd_table(121, 127) == PdRoute::global);   // 15375, 15367
  CHECK(route_pd_table(1, 1) == PdRoute::lds && route_pd_table(0, 70000) == PdRoute::lds);
  CHECK(route_pd_table(65536, 65536) == PdRoute::global);       // 2^32 cells: the product is taken in 64 bits
  const struct { uint32_t kcap; int nk; } vi[] = {{32, 1}, {64, 1}, {65, 2}, {128, 2}, {129, 4}, {256, 4}, {257, 8}, {512, 8}, {1024, 8}};
  for (const auto &c : vi) CHECK(route_vi_refine(c.kcap) == c.nk);
}

int main() {
  test_blocked();
  test_sequential();
  test_units_per_launch();
  test_marginal();
  test_chains_marginal_cut();
  test_chains_marginal_plan();
  test_chunks_and_batches();
  test_summaries();
  if (g_failures) return 1;
  std::printf("route calls ok\n");
  return 0;
}
