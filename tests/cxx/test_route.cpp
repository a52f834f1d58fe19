// Host test of common_amd/csrc/route.hpp alone (plans come from tile_plan.hpp through plan_cases.hpp): the score and sweep
// routes against the rules written beside them -- THE SHARD RULE over a grid of plans, group counts and view sizes, then
// each route's conditions one by one.  A chip of 256 CUs; no device.  Every expectation is worked out from the rule
// (the arithmetic stands beside it), none from a run of the routes.
#include "plan_cases.hpp"

using namespace cases;

static Switches forced_tail(uint64_t min_rows) {
  Switches sw;
  sw.tail_forced = true, sw.tail_min_rows = min_rows;
  return sw;
}
static RouteFacts facts(const Spec &s, uint32_t K, uint64_t view_rows, const Switches &sw = Switches()) {
  return facts_of(s, plan(s, K, true, sw), K, view_rows);
}

static bool same_but_wave_rows(const SweepRoute &a, const SweepRoute &b) {
  return a.kind == b.kind && a.lanes == b.lanes && a.table_rows == b.table_rows && a.transposed == b.transposed &&
         a.shape.pair == b.shape.pair && a.shape.last == b.shape.last && a.shape.nich1 == b.shape.nich1 && a.tail_ld == b.tail_ld &&
         a.tail_pair == b.tail_pair;
}

// the plans of test_tile_plan.cpp, one of every path and family mix
static std::vector<Spec> grid_specs() {
  std::vector<Spec> v;
  v.push_back(Spec().bbs(8).nichs(8));                  // NICH_PACK
  v.push_back(Spec().bbs(16).nichs(4));                 // TILE_ROLES
  v.push_back(Spec().bbs(32));                          // LOOKUPS
  v.push_back(Spec().bbs(8));
  v.push_back(Spec().nichs(2));
  v.push_back(Spec().nichs(16));
  v.push_back(Spec().nichs(1));                         // the single-nich kernels
  { Spec s; s.bbs(4).nichs(2), s.dm(4, 40); v.push_back(s); }
  { Spec s; s.bbs(4).nichs(8), s.dd(200); v.push_back(s); }           // a generic feature: TILE
  { Spec s; s.nich(1.0f, true), s.nichs(3), s.bbs(4, true); v.push_back(s); }
  { Spec s; for (int i = 0; i < 16; i++) s.dd(32); v.push_back(s); }
  { Spec s; for (int i = 0; i < 16; i++) s.bb(), s.gp(24), s.dd(32), s.nich(); v.push_back(s); }     // C3's mix
  { Spec s; s.gp(100), s.nichs(2); v.push_back(s); }
  { Spec s; s.add(MSC_NIW, 2, false, false); v.push_back(s); }        // the fused single-niw kernel
  { Spec s; s.add(MSC_NIW, 2, false, false), s.bbs(4); v.push_back(s); }
  return v;
}

static void test_shard_rule() {
  const uint32_t Ks[] = {8, 32, 64, 100, 128, 200, 256, 300, 384, 512, 1500};
  const uint64_t views[] = {1000, 16383, 16384, 65535, 65536, 1000000};
  const Switches sws[] = {Switches(), forced_tail(0), forced_tail(50000), [] { Switches s; s.no_narrow_tail = true; return s; }()};
  const std::vector<Spec> specs = grid_specs();
  for (const Switches &sw : sws)
    for (size_t si = 0; si < specs.size(); si++)
      for (uint32_t K : Ks) {
        const Planned pl = plan(specs[si], K, true, sw);
        for (uint64_t view_rows : views) {
          RouteFacts rf = facts_of(specs[si], pl, K, view_rows);
          for (int beyond = 0; beyond < 2; beyond++) {
            if (beyond) {                               // ... and with a count column beyond its table, where the plan has one
              bool any = false;
              for (RouteFeat &f : rf.feats) if (is_count_family(f.family)) f.beyond_table = any = true;
              if (!any) break;
            }
            const uint64_t rows[] = {1, 100, 20000, view_rows};
            const SweepRoute w0 = route_sweep(rf, sw, rows[3]);
            const ScoreRoute s0 = route_score(rf, sw, rows[3]);
            for (uint64_t nrows : rows) {
              const SweepRoute w = route_sweep(rf, sw, nrows);
              if (!same_but_wave_rows(w, w0)) {
                std::printf("FAIL shard rule, sweep: spec %zu K %u view %llu nrows %llu: kind %d against %d\n", si, K,
                            (unsigned long long)view_rows, (unsigned long long)nrows, (int)w.kind, (int)w0.kind);
                g_failures++;
              }
              const ScoreRoute s = route_score(rf, sw, nrows);
              if (s.lanes != s0.lanes || s.table_rows != s0.table_rows || s.path != s0.path) {
                std::printf("FAIL shard rule, score: spec %zu K %u view %llu nrows %llu\n", si, K, (unsigned long long)view_rows,
                            (unsigned long long)nrows);
                g_failures++;
              }
            }
          }
        }
      }
}

static void test_single_nich() {
  const Spec s = Spec().nichs(1);
  for (uint32_t K : {8u, 256u, 1024u, 1025u, 1500u, 32768u})
    for (uint64_t view_rows : {1000ull, 16383ull, 16384ull, 1000000ull}) {      // 64 rows x 256 CUs = 16384
      const RouteFacts rf = facts(s, K, view_rows);
      Switches sw;
      const SweepRoute r = route_sweep(rf, sw, 100);
      CHECK(r.kind == (K > 1024 ? SweepKind::nich1_rows : SweepKind::nich1));
      CHECK(r.transposed == (view_rows >= 16384));
      sw.sweep_nich1 = 1;
      CHECK(!route_sweep(rf, sw, 100).transposed);
      sw.sweep_nich1 = 2;
      CHECK(route_sweep(rf, sw, 100).transposed);
      CHECK(route_score(rf, Switches(), 100).path == MSC_PATH_NICH1);
    }
  CHECK(route_sweep(facts(s, 32769, 1000000), Switches(), 100).kind == SweepKind::generic);    // beyond the rows kernel's groups
}

static void test_narrow() {
  const Spec two = Spec().nichs(2);
  // two nich features: 120 us a million rows at 16 lanes; the nich-only tiles 6 + 1.3 x 2 = 8.6 us a round, x 30.52 rounds
  // (10^6 / 128 / 256) x 0.62 (PAIR) = 162.7, x 1.25 = 203: taken.  Tables: 12 rows x 16 lanes x 16 bytes.
  {
    uint32_t rows = 0;
    CHECK(narrow_lanes(facts(two, 64, 10000), Switches(), &rows) == 16 && rows == 12);
    CHECK(narrow_lanes(facts(two, 32, 10000), Switches(), &rows) == 8);
    CHECK(narrow_lanes(facts(two, 16, 10000), Switches(), &rows) == 4);
    CHECK(narrow_lanes(facts(two, 65, 10000), Switches(), &rows) == 0);                  // K <= 64
    CHECK(route_sweep(facts(two, 64, 10000), Switches(), 100).kind == SweepKind::narrow);
    CHECK(route_score(facts(two, 64, 10000), Switches(), 100).lanes == 16);
  }
  {                                                     // the view below kNarrowMaxRows rows, or the tail not allowed
    uint32_t rows = 0;
    CHECK(narrow_lanes(facts(two, 64, 65535), Switches(), &rows) == 16);
    CHECK(narrow_lanes(facts(two, 64, 65536), Switches(), &rows) == 0);
    Switches no_tail;
    no_tail.no_narrow_tail = true;
    CHECK(narrow_lanes(facts(two, 64, 65536, no_tail), no_tail, &rows) == 16);
    CHECK(narrow_lanes(facts(two, 64, 65536, forced_tail(0)), forced_tail(0), &rows) == 16);
  }
  {                                                     // the tables in 64 KiB: rows x 16 lanes x 16 bytes, 256 rows at the most
    Spec d2, d3;
    d2.dd(100), d2.dd(100);                             // 100 us against 1.25 x (0.75 x (6 + 0.9 + 2.4)) x 30.52 x 0.62 = 165
    d3.dd(100), d3.dd(100), d3.dd(100);                 // 150 us against 1.25 x (0.75 x (6 + 1.35 + 3.6)) x 30.52 x 0.62 = 194: the price would pass
    uint32_t rows = 0;
    CHECK(narrow_lanes(facts(d2, 64, 10000), Switches(), &rows) == 16 && rows == 200);
    CHECK(narrow_lanes(facts(d3, 64, 10000), Switches(), &rows) == 0);
    CHECK(narrow_lanes(facts(d3, 32, 10000), Switches(), &rows) == 8 && rows == 300);    // 8 lanes: 512 rows fit; 75 us
  }
  {                                                     // the price: eight bool columns are 240 us here, two fused lookups on the tiles
    uint32_t rows = 0;                                  // 1.25 x (0.75 x (6 + 0.9 + 0.384)) x 30.52 x 0.62 = 129
    CHECK(narrow_lanes(facts(Spec().bbs(8), 64, 10000), Switches(), &rows) == 0);
  }
  {                                                     // never with niw or dm, or a count beyond its table
    uint32_t rows = 0;
    Spec dm, niw, g;
    dm.nichs(2), dm.dm(4, 40);
    niw.nichs(2), niw.add(MSC_NIW, 2, false, false);
    g.gp(20), g.nichs(2);                               // 170 us against 1.25 x (6 + 2.6 + 3.0) x 30.52 x 0.62 = 274
    CHECK(narrow_lanes(facts(dm, 64, 10000), Switches(), &rows) == 0);
    CHECK(narrow_lanes(facts(niw, 64, 10000), Switches(), &rows) == 0);
    RouteFacts rf = facts(g, 64, 10000);
    CHECK(narrow_lanes(rf, Switches(), &rows) == 16 && rows == 32);
    rf.feats[0].beyond_table = true;
    CHECK(narrow_lanes(rf, Switches(), &rows) == 0);
    CHECK(route_sweep(rf, Switches(), 100).kind == SweepKind::generic);
  }
}

static void test_roles_tail() {
  const Spec roles = Spec().bbs(16).nichs(4), pack = Spec().bbs(8).nichs(8);
  const Switches on = forced_tail(0);                   // (the lane <-> row kernel "pays" at every view size)
  for (uint32_t K : {256u, 257u, 300u, 320u, 321u, 384u, 385u, 512u}) {
    const SweepRoute r = route_sweep(facts(roles, K, 100000, on), on, 100), q = route_sweep(facts(pack, K, 100000, on), on, 100);
    const bool want = K > 256 && K <= 384;
    CHECK((r.kind == SweepKind::roles_tail) == want && (q.kind == SweepKind::roles_tail) == want);
    if (!want) {
      CHECK(r.kind == (K <= 256 ? SweepKind::mixed : SweepKind::generic));
      continue;
    }
    CHECK(r.tail_ld == (K <= 320 ? 64u : 128u) && q.tail_ld == r.tail_ld);
    CHECK(r.tail_pair == (K > 320));                    // TILE_ROLES and tail_ld 128
    CHECK(!q.tail_pair);                                // NICH_PACK: the lane <-> row kernel scores the tail
  }
  {                                                     // a TILE plan, a plan without the tail, a niw feature, a view of few rows
    Spec tile, niw;
    tile.bbs(4).nichs(8), tile.dd(200);
    niw.bbs(16).nichs(4), niw.add(MSC_NIW, 2, false, false);
    CHECK(route_sweep(facts(tile, 300, 100000, on), on, 100).kind == SweepKind::generic);
    Switches off = on;
    off.no_narrow_tail = true;
    CHECK(route_sweep(facts(roles, 300, 100000, off), off, 100).kind == SweepKind::generic);
    CHECK(route_sweep(facts(niw, 300, 100000, on), on, 100).kind == SweepKind::generic);
    CHECK(route_sweep(facts(roles, 300, 16383), Switches(), 100).kind == SweepKind::generic);   // below kTailMinRows
  }
}

static void test_generic_and_niw1() {
  Spec one, mixed;
  one.add(MSC_NIW, 2, false, false);
  mixed.add(MSC_NIW, 2, false, false), mixed.bbs(4);
  CHECK(route_sweep(facts(one, 256, 100000), Switches(), 100).kind == SweepKind::niw1);
  CHECK(route_sweep(facts(one, 257, 100000), Switches(), 100).kind == SweepKind::generic);      // (niw1_max_groups: 256)
  CHECK(route_sweep(facts(mixed, 8, 100000), Switches(), 100).kind == SweepKind::generic);
  CHECK(!sweep_plain(facts(mixed, 8, 100000)) && sweep_plain(facts(Spec().bbs(4), 8, 100000)));
  Spec g;
  g.gp(100), g.bbs(4);
  RouteFacts rf = facts(g, 256, 100000);
  CHECK(route_sweep(rf, Switches(), 100).kind == SweepKind::mixed);
  rf.feats[0].beyond_table = true;
  CHECK(!sweep_plain(rf) && route_sweep(rf, Switches(), 100).kind == SweepKind::generic);
}

static void test_forced_tail() {
  const Spec s = Spec().bbs(8);                         // (not the narrow tiling: its price, test_narrow)
  const Switches sw = forced_tail(50000);
  CHECK(route_sweep(facts(s, 64, 49999, sw), sw, 100).kind == SweepKind::mixed);
  CHECK(route_sweep(facts(s, 64, 50000, sw), sw, 100).kind == SweepKind::rows);
  CHECK(route_sweep(facts(s, 65, 50000, sw), sw, 100).kind == SweepKind::rows_sampler);
  CHECK(route_sweep(facts(s, 128, 50000, sw), sw, 100).kind == SweepKind::rows_sampler);
  CHECK(route_sweep(facts(s, 129, 50000, sw), sw, 100).kind == SweepKind::mixed);            // kTailMaxGroups
  CHECK(route_sweep(facts(s, 128, 49999, sw), sw, 100).kind == SweepKind::mixed);
  // a score pass goes by the CALL's rows (every last-tile kernel gives the tile kernels' bits)
  CHECK(route_score(facts(s, 100, 1000000, sw), sw, 49999).shape.last == LastTile::tiles);
  CHECK(route_score(facts(s, 100, 1000000, sw), sw, 50000).shape.last == LastTile::rows);
}

int main() {
  test_shard_rule();
  test_single_nich();
  test_narrow();
  test_roles_tail();
  test_generic_and_niw1();
  test_forced_tail();
  if (g_failures) return 1;
  std::printf("route ok\n");
  return 0;
}
