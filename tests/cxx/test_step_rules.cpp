// Host test of common_amd/csrc/step_rules.hpp alone.  RngMirror after every event, as literal tables read off the field
// writes the type replaced (abi.cpp and predict.cpp made them by hand), from a fresh mirror and from a held pair; the two
// ways a step fails half way; the snapshot round trip; the wrap of the sweep index.  step_action over the full grid of
// its inputs, held to the rules as properties; and the steps of tests/test_gpu_sweep_step.py's
// test_steps_equal_the_two_calls walked as plain inputs, doing to a model of the state what msc_sweep_step does.
#include "step_rules.hpp"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

using msc::RngMirror;
using msc::StepAction;
using msc::StepInputs;
using msc::StepKey;

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

// the mirror as its queries show it: "V" valid or "-", seed, sweep, "O" owed (mid-step) or "-" -- e.g. "V 7 11 -"
static std::string show(const RngMirror &m) {
  return std::string(m.valid() ? "V " : "- ") + std::to_string(m.seed()) + " " + std::to_string(m.sweep()) +
         (m.mid_step() ? " O" : " -");
}
static RngMirror held() {
  RngMirror m;
  m.set(7, 10);
  return m;
}

struct Event {
  const char *name;
  std::function<void(RngMirror &)> run;
  const char *from_fresh, *from_held;   // show() after the event from RngMirror() / held()
};

static void test_mirror() {
  CHECK(show(RngMirror()) == "- 0 0 -", "fresh: %s", show(RngMirror()).c_str());
  CHECK(show(held()) == "V 7 10 -", "held: %s", show(held()).c_str());
  CHECK(!RngMirror().holds(0, 0), "a fresh mirror holds nothing, (0, 0) included");
  const std::vector<Event> events = {
      {"set(3, 4)", [](RngMirror &m) { m.set(3, 4); }, "V 3 4 -", "V 3 4 -"},
      {"advanced", [](RngMirror &m) { m.advanced(); }, "- 0 1 -", "V 7 11 -"},
      {"tail_owes", [](RngMirror &m) { m.tail_owes(); }, "- 0 0 -", "- 7 10 -"},
      {"tail_owes, tail_paid", [](RngMirror &m) { m.tail_owes(); m.tail_paid(); }, "V 0 1 -", "V 7 11 -"},
      {"deferred", [](RngMirror &m) { m.deferred(); }, "- 0 0 O", "- 7 10 O"},
      {"deferred, deferred_paid", [](RngMirror &m) { m.deferred(); m.deferred_paid(); }, "V 0 1 -", "V 7 11 -"},
      {"invalidate", [](RngMirror &m) { m.invalidate(); }, "- 0 0 -", "- 7 10 -"},
  };
  for (const Event &e : events) {
    RngMirror a, b = held();
    e.run(a);
    e.run(b);
    CHECK(show(a) == e.from_fresh, "%s from fresh: %s, expected %s", e.name, show(a).c_str(), e.from_fresh);
    CHECK(show(b) == e.from_held, "%s from held: %s, expected %s", e.name, show(b).c_str(), e.from_held);
    for (const RngMirror *m : {&a, &b}) {
      // holds: valid and both equal, nothing else
      CHECK(m->holds(m->seed(), m->sweep()) == m->valid(), "%s: holds(own pair) is not valid()", e.name);
      CHECK(!m->holds(m->seed() + 1, m->sweep()) && !m->holds(m->seed(), m->sweep() + 1) && !m->holds(m->seed(), m->sweep() - 1),
            "%s: holds another pair", e.name);
    }
    // a snapshot taken before the event, and before every other event after it, restores to what compares equal
    RngMirror d = held();
    const RngMirror before = d.snapshot();
    e.run(d);
    CHECK((d == before) == (show(d) == show(before)), "%s: equality disagrees with the queries", e.name);
    CHECK((d != before) == (show(d) != show(before)), "%s: inequality disagrees with the queries", e.name);
    for (const Event &o : events) o.run(d);
    d.restore(before);
    CHECK(d == before && show(d) == "V 7 10 -" && d.holds(7, 10), "%s: restore gave %s", e.name, show(d).c_str());
  }
  // a step whose accumulate fails: tail_owes without tail_paid leaves the mirror invalid, whatever is asked of it; the next
  // sweep sets the pair afresh
  {
    RngMirror m = held();
    m.tail_owes();
    CHECK(!m.holds(7, 10) && !m.holds(7, 11) && !m.mid_step(), "tail_owes alone: %s", show(m).c_str());
    m.set(7, 10);
    CHECK(m.holds(7, 10) && !m.mid_step(), "set after a failed tail: %s", show(m).c_str());
  }
  // msc_sweep_step_begin without its msc_state_commit_reduce: invalid and mid-step until the commit, which moves the
  // mirror to the sweep index after the one begun -- whatever set the pair in between
  {
    RngMirror m = held();
    m.deferred();
    CHECK(!m.holds(7, 10) && !m.holds(7, 11) && m.mid_step(), "deferred alone: %s", show(m).c_str());
    m.set(9, 40);
    CHECK(m.holds(9, 40) && m.mid_step(), "set while mid-step: %s", show(m).c_str());
    m.deferred_paid();
    CHECK(show(m) == "V 9 11 -", "deferred_paid after a set: %s", show(m).c_str());
  }
  // the next index is part of the value: two mirrors that differ in it alone are not equal
  {
    RngMirror a = held(), b = held();
    a.deferred();
    b.advanced();
    b.advanced();
    b.deferred();
    b.set(7, 10);
    a.set(7, 10);
    CHECK(show(a) == show(b) && a != b, "mirrors owing different indices compare equal");
  }
  // the sweep index wraps as uint64_t does
  {
    RngMirror m;
    m.set(1, UINT64_MAX);
    m.advanced();
    CHECK(m.holds(1, 0), "advanced at 2^64 - 1: %s", show(m).c_str());
    m.set(1, UINT64_MAX);
    m.tail_owes();
    m.tail_paid();
    CHECK(m.holds(1, 0), "tail_paid at 2^64 - 1: %s", show(m).c_str());
    m.set(1, UINT64_MAX);
    m.deferred();
    m.deferred_paid();
    CHECK(m.holds(1, 0), "deferred_paid at 2^64 - 1: %s", show(m).c_str());
  }
}

static const char *name_of(StepAction a) {
  switch (a) {
    case StepAction::eager: return "eager";
    case StepAction::rekey: return "rekey";
    case StepAction::count: return "count";
    case StepAction::replay: return "replay";
    case StepAction::capture: return "capture";
  }
  return "?";
}

// every combination of the seven switches with seen in {0, 1, 2, 3}: each action exactly where its rule says
static void test_rule_grid() {
  int n[5] = {0, 0, 0, 0, 0};
  for (int bits = 0; bits < 128; bits++)
    for (int seen = 0; seen < 4; seen++) {
      StepInputs in;
      in.graph_on = bits & 1;
      in.disabled = bits & 2;
      in.has_exec = bits & 4;
      in.same_key = bits & 8;
      in.holds = bits & 16;
      in.flags_equal = bits & 32;
      in.fused = bits & 64;
      in.seen = seen;
      const StepAction a = msc::step_action(in);
      n[(int)a]++;
      const bool live = in.graph_on && !in.disabled;                             // rule 2
      const bool exec = live && in.same_key && in.has_exec;                      // rule 3: a new key has no executable
      const bool ready = in.holds && in.flags_equal;
      CHECK((a == StepAction::rekey) == (live && !in.same_key), "bits %d seen %d: %s", bits, seen, name_of(a));
      CHECK((a == StepAction::replay) == (exec && ready), "bits %d seen %d: %s", bits, seen, name_of(a));                 // rule 4
      CHECK((a == StepAction::eager) == (!live || (exec && !ready)), "bits %d seen %d: %s", bits, seen, name_of(a));      // 2, 4
      CHECK((a == StepAction::capture) == (live && in.same_key && !in.has_exec && seen >= 2 && in.holds && in.fused),
            "bits %d seen %d: %s", bits, seen, name_of(a));                                                               // rule 6
      CHECK((a == StepAction::count) == (live && in.same_key && !in.has_exec && (seen < 2 || !in.holds || !in.fused)),
            "bits %d seen %d: %s", bits, seen, name_of(a));                                                               // rule 5
    }
  CHECK(n[(int)StepAction::eager] == 408 && n[(int)StepAction::rekey] == 64 && n[(int)StepAction::count] == 28 &&
            n[(int)StepAction::replay] == 8 && n[(int)StepAction::capture] == 4,
        "the grid's totals: eager %d rekey %d count %d replay %d capture %d", n[0], n[1], n[2], n[3], n[4]);
}

static void test_key() {
  int view_a = 0, view_b = 0, z_a = 0, z_b = 0;
  const StepKey k{&view_a, &z_a, 3, 0, 1000, 0, 1.1f, {0, 1, 2}};
  std::vector<StepKey> others(8, k);
  others[0].view = &view_b;
  others[1].z = &z_b;
  others[2].view_serial = 4;
  others[3].row0 = 1;
  others[4].nrows = 999;
  others[5].row_id0 = 1;
  others[6].alpha = 0.4f;
  others[7].cols = {0, 2, 1};
  CHECK(k == StepKey(k), "a key equals its copy");
  for (size_t i = 0; i < others.size(); i++) CHECK(!(k == others[i]), "a key equals one that differs in field %zu", i);
  CHECK(!(k == StepKey()), "a key equals the empty key");
}

// what msc_sweep_step keeps, and what it does with each action (abi.cpp), without the device
struct Model {
  bool has_exec = false, disabled = false;
  int seen = 0;
  StepKey key;
  RngMirror rng;
  unsigned long long n_eager = 0, n_replayed = 0, n_captures = 0;

  void eager(uint64_t seed, uint64_t sweep) {
    n_eager++;
    if (!rng.holds(seed, sweep)) rng.set(seed, sweep);   // (sweep_assign_impl)
    rng.tail_owes();
    rng.tail_paid();
  }
  StepAction step(const StepKey &k, uint64_t seed, uint64_t sweep, bool flags_equal = true) {
    StepInputs in;
    in.graph_on = true;
    in.disabled = disabled;
    in.has_exec = has_exec;
    in.same_key = k == key;
    in.holds = rng.holds(seed, sweep);
    in.flags_equal = flags_equal;
    in.seen = seen;
    in.fused = true;
    const StepAction a = msc::step_action(in);
    switch (a) {
      case StepAction::eager: eager(seed, sweep); break;
      case StepAction::rekey:
        has_exec = false;
        key = k;
        seen = 0;
        [[fallthrough]];
      case StepAction::count:
        seen++;
        eager(seed, sweep);
        break;
      case StepAction::replay:
        n_replayed++;
        rng.advanced();
        break;
      case StepAction::capture:
        eager(seed, sweep);
        n_eager--;                                       // (recorded, not run)
        has_exec = true;
        n_captures++;
        n_replayed++;
        break;
    }
    return a;
  }
};

static void test_walk() {
  int view = 0, z = 0;
  StepKey k{&view, &z, 1, 0, 5000, 0, 1.1f, {0}};
  Model m;
  std::string got;
  auto walk = [&](uint64_t seed, uint64_t sweep, bool flags_equal = true) {
    got += name_of(m.step(k, seed, sweep, flags_equal));
    got += ' ';
    CHECK(m.rng.holds(seed, sweep + 1), "after step (%llu, %llu): %s", (unsigned long long)seed, (unsigned long long)sweep,
          show(m.rng).c_str());
  };
  for (uint64_t sweep = 0; sweep < 8; sweep++) walk(77, sweep);
  CHECK(got == "rekey count capture replay replay replay replay replay ", "the first eight steps: %s", got.c_str());
  CHECK(m.n_eager == 2 && m.n_replayed == 6, "stats after eight steps: (%llu, %llu)", m.n_eager, m.n_replayed);
  got.clear();
  walk(77, 8, false);   // a call in between changed what is current on the device: not replayed, the executable kept
  walk(77, 20);         // a jump in the sweep index
  walk(77, 21);
  walk(5, 22);          // a new seed
  walk(5, 23);
  walk(5, 24);
  CHECK(got == "eager eager replay eager replay replay ", "the interruptions: %s", got.c_str());
  CHECK(m.n_captures == 1 && m.has_exec && m.seen == 2, "an interruption dropped or re-captured the executable");
  got.clear();
  k.alpha = 0.4f;       // a new alpha is a new key
  for (uint64_t sweep = 25; sweep < 30; sweep++) walk(5, sweep);
  CHECK(got == "rekey count capture replay replay ", "under the new key: %s", got.c_str());
  CHECK(m.n_captures == 2, "captures: %llu", m.n_captures);
  CHECK(m.n_eager == 7 && m.n_replayed == 12, "stats at the end: (%llu, %llu)", m.n_eager, m.n_replayed);
  // a pair that does not hold is counted but never captured: the capture waits for the first step that continues
  Model w;
  got.clear();
  for (uint64_t sweep : {0, 2, 4, 6, 7}) got += std::string(name_of(w.step(k, 1, sweep))) + ' ';
  CHECK(got == "rekey count count count capture ", "every other sweep index: %s", got.c_str());
  // after a failed capture every step is eager
  w.disabled = true;
  w.has_exec = false;
  CHECK(w.step(k, 1, 8) == StepAction::eager && w.step(k, 1, 9) == StepAction::eager, "a disabled state still tracks its steps");
}

int main() {
  test_mirror();
  test_rule_grid();
  test_key();
  test_walk();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("step_rules ok\n");
  return 0;
}
