// Host test of common_amd/csrc/table_validity.hpp alone: the flags after every event, as literal tables read off the
// code the type replaced (the flag writes abi.cpp made by hand), from two starts -- everything valid with a current draw,
// everything stale -- on three features, so that a per-feature event is seen to leave the other features alone; a
// snapshot round trip; and which events drop a blocked draw.
#include "table_validity.hpp"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

using msc::TableValidity;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      failures++;                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
    }                                                     \
  } while (0)

constexpr int NF = 3;
// the flags as the queries show them: per feature "RAD" = raw, additive, derived valid ('-' stale), then counts'
// additive, crp, draw -- e.g. "RAD R-D RA- C-D"
static std::string show(const TableValidity &v) {
  std::string s;
  for (int f = 0; f < NF; f++) {
    s += v.raw_stale(f) ? '-' : 'R';
    s += v.additive_stale(f) ? '-' : 'A';
    s += v.derived_stale(f) ? '-' : 'D';
    s += ' ';
  }
  s += v.counts_additive_stale() ? '-' : 'C';
  s += v.crp_stale() ? '-' : 'P';
  s += v.draw_current() ? 'W' : '-';
  return s;
}

static TableValidity all_valid() {
  TableValidity v;
  v.created(NF);
  v.kept_current();
  v.drawn();
  return v;
}
static TableValidity all_stale() {
  TableValidity v;
  v.created(NF);
  v.accumulated();                                  // raw stale
  for (int f = 0; f < NF; f++) v.fields_written(f);   // additive, derived stale
  v.counts_changed();                               // counts' additive, crp stale, no draw
  return v;
}

struct Event {
  const char *name;
  std::function<void(TableValidity &)> run;
  const char *from_valid, *from_stale;   // show() after the event from all_valid() / all_stale()
  bool drops_draw;
};

int main() {
  CHECK(show(all_valid()) == "RAD RAD RAD CPW", "all_valid: %s", show(all_valid()).c_str());
  CHECK(show(all_stale()) == "--- --- --- ---", "all_stale: %s", show(all_stale()).c_str());
  {
    TableValidity v;
    v.created(NF);
    CHECK(show(v) == "RA- RA- RA- C--", "created: %s", show(v).c_str());
  }
  const std::vector<Event> events = {
      // per-feature events on feature 1: features 0 and 2 stay as they were
      {"fields_written(1)", [](TableValidity &v) { v.fields_written(1); }, "RAD R-- RAD CP-", "--- --- --- ---", true},
      {"hp_changed(1)", [](TableValidity &v) { v.hp_changed(1); }, "RAD RA- RAD CP-", "--- --- --- ---", true},
      {"derived_dropped(1)", [](TableValidity &v) { v.derived_dropped(1); }, "RAD RA- RAD CPW", "--- --- --- ---", false},
      {"alpha_changed", [](TableValidity &v) { v.alpha_changed(); }, "RAD RAD RAD C--", "--- --- --- ---", true},
      {"counts_changed", [](TableValidity &v) { v.counts_changed(); }, "RAD RAD RAD ---", "--- --- --- ---", true},
      {"additive_lifted", [](TableValidity &v) { v.additive_lifted(); }, "RAD RAD RAD CPW", "-A- -A- -A- C--", false},
      {"accumulated", [](TableValidity &v) { v.accumulated(); }, "-AD -AD -AD CP-", "-A- -A- -A- C--", true},
      {"additive_rewritten", [](TableValidity &v) { v.additive_rewritten(); }, "RAD RAD RAD CP-", "--- --- --- ---", true},
      {"committed", [](TableValidity &v) { v.committed(); }, "RA- RA- RA- C--", "R-- R-- R-- ---", true},
      {"committed_and_prepared", [](TableValidity &v) { v.committed_and_prepared(); }, "RAD RAD RAD CP-", "R-D R-D R-D -P-",
       true},
      {"prepared", [](TableValidity &v) { v.prepared(); }, "RAD RAD RAD CPW", "--D --D --D ---", false},
      {"crp_prepared", [](TableValidity &v) { v.crp_prepared(); }, "RAD RAD RAD CPW", "--- --- --- -P-", false},
      {"kept_current", [](TableValidity &v) { v.kept_current(); }, "RAD RAD RAD CP-", "RAD RAD RAD CP-", true},
      {"step_began", [](TableValidity &v) { v.step_began(); }, "RAD RAD RAD CP-", "--- --- --- ---", true},
      {"drawn", [](TableValidity &v) { v.drawn(); }, "RAD RAD RAD CPW", "--- --- --- --W", false},
  };
  for (const Event &e : events) {
    TableValidity a = all_valid(), b = all_stale();
    e.run(a);
    e.run(b);
    CHECK(show(a) == e.from_valid, "%s from all valid: %s, expected %s", e.name, show(a).c_str(), e.from_valid);
    CHECK(show(b) == e.from_stale, "%s from all stale: %s, expected %s", e.name, show(b).c_str(), e.from_stale);
    // the draw: made from the tables as they stand, then the event
    TableValidity c = all_stale();
    c.drawn();
    e.run(c);
    CHECK(c.draw_current() == !e.drops_draw, "%s: the draw is %s afterwards", e.name, c.draw_current() ? "current" : "stale");
    // a snapshot taken before the event, and before every other event after it, restores to what compares equal
    TableValidity d = all_valid();
    const TableValidity::Snapshot before = d.snapshot();
    e.run(d);
    for (const Event &o : events) o.run(d);
    d.restore(before);
    CHECK(d.snapshot() == before && show(d) == "RAD RAD RAD CPW", "%s: restore gave %s", e.name, show(d).c_str());
  }
  // the per-feature events at the other features
  for (int f = 0; f < NF; f++) {
    TableValidity v = all_valid();
    v.fields_written(f);
    for (int g = 0; g < NF; g++)
      CHECK(v.additive_stale(g) == (g == f) && v.derived_stale(g) == (g == f) && !v.raw_stale(g), "fields_written(%d) at %d", f, g);
    v = all_valid();
    v.hp_changed(f);
    for (int g = 0; g < NF; g++)
      CHECK(!v.additive_stale(g) && v.derived_stale(g) == (g == f) && !v.raw_stale(g), "hp_changed(%d) at %d", f, g);
    CHECK(v.any_derived_stale() && !v.any_raw_stale(), "hp_changed(%d): any_*", f);
  }
  // snapshots compare by every flag
  {
    const TableValidity v = all_valid();
    for (const Event &e : events) {
      TableValidity w = all_valid();
      e.run(w);
      CHECK((w.snapshot() == v.snapshot()) == (show(w) == show(v)), "%s: snapshot equality disagrees with the flags", e.name);
      CHECK((w.snapshot() != v.snapshot()) == (show(w) != show(v)), "%s: snapshot inequality disagrees with the flags", e.name);
    }
    CHECK(!all_valid().any_raw_stale() && !all_valid().any_derived_stale(), "all_valid: any_*");
    CHECK(all_stale().any_raw_stale() && all_stale().any_derived_stale(), "all_stale: any_*");
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("table_validity ok: %zu events\n", events.size());
  return 0;
}
