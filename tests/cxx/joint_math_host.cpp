// Host build of common_amd/csrc/joint_math.hpp for tests/test_joint_cpu.py: the order of a joint row's total, the rule
// by which a sample replaces the best one kept, and the shape checks of the three entry points -- a program of its own
// that includes nothing else of the library, run plain and under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "joint_math.hpp"

using namespace msc::joint;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      failures++;                                                      \
    }                                                                  \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a chain's trace through the rule, as JointTracker drives msc_chains_keep_best: -> the iteration kept, -1 for none
static long long run_best(const std::vector<double> &totals, double *best_out) {
  double best = -std::numeric_limits<double>::infinity();
  long long at = -1;
  for (size_t i = 0; i < totals.size(); i++)
    if (keep_best_wins(totals[i], best)) best = totals[i], at = (long long)i;
  *best_out = best;
  return at;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

  // ---- the layout ----
  CHECK(joint_row(0) == 3 && joint_row(5) == 8 && joint_prior_at(5) == 7 && joint_prior_at(0) == 2);
  CHECK(joint_row(0xffffffffu) == 0x100000002ull);          // (no wrap in 32 bits)

  // ---- the total: the written order, one rounding an addition ----
  {
    // a + d0 loses d0 entirely when a is large; the written order is then visible in the bits
    const double row[] = {0.0, 1e16, 1.0, 1.0, -1e16, 0.5};   // F = 3: a, d0, d1, d2, p
    const double t = joint_total(row, 3);
    volatile double w = row[1];
    w = w + row[2];
    w = w + row[3];
    w = w + row[4];
    w = w + row[5];
    CHECK(same_bits(t, w));
    CHECK(t == 0.5);                                          // ((1e16 + 1) + 1) - 1e16 = 0 in double, + 0.5
    CHECK(!same_bits(t, row[1] + row[4] + row[2] + row[3] + row[5]));   // another order gives 2.5
    const double none[] = {0.0, -3.25, 0.0};                  // F = 0: a, p
    CHECK(joint_total(none, 0) == -3.25);
    const double neg0[] = {0.0, -0.0, -0.0, -0.0};            // F = 1
    CHECK(std::signbit(joint_total(neg0, 1)));                // -0.0 + -0.0 + -0.0 stays -0.0
    const double withinf[] = {0.0, -1.0, -inf, 2.0, 0.0};     // F = 2: an empty support
    CHECK(joint_total(withinf, 2) == -inf);
    const double clash[] = {0.0, inf, -inf, 0.0};
    CHECK(std::isnan(joint_total(clash, 1)));
    const double withnan[] = {0.0, 1.0, nan, 0.0};
    CHECK(std::isnan(joint_total(withnan, 1)));
  }

  // ---- the keep-best rule ----
  CHECK(keep_best_wins(1.0, 0.5) && !keep_best_wins(0.5, 1.0));
  CHECK(!keep_best_wins(1.0, 1.0));                           // a tie keeps the earlier sample
  CHECK(!keep_best_wins(0.0, -0.0) && !keep_best_wins(-0.0, 0.0));
  CHECK(!keep_best_wins(nan, -inf) && !keep_best_wins(nan, 0.0) && !keep_best_wins(nan, nan));
  CHECK(!keep_best_wins(0.0, nan) && !keep_best_wins(inf, nan));   // (why a tracker never starts from NaN)
  CHECK(keep_best_wins(-1e308, -inf) && !keep_best_wins(-inf, -inf));
  CHECK(keep_best_wins(inf, 1e308) && !keep_best_wins(inf, inf));
  CHECK(keep_best_wins(std::nextafter(1.0, 2.0), 1.0));
  {
    double best;
    CHECK(run_best({-5.0, -3.0, nan, -3.0, -4.0}, &best) == 1 && best == -3.0);   // the first of equal maxima
    CHECK(run_best({nan, nan}, &best) == -1 && best == -inf);
    CHECK(run_best({-inf, -inf}, &best) == -1);
    CHECK(run_best({}, &best) == -1);
    CHECK(run_best({-0.0, 0.0}, &best) == 0 && std::signbit(best));
    CHECK(run_best({1.0, inf, inf, nan}, &best) == 1 && best == inf);
  }

  // ---- the shape checks ----
  {
    JointCheck c = check_score_joint("f", true, false, 0, 5, 8, false, 0, 32);
    CHECK(c.ok && c.message[0] == 0);
    CHECK(check_score_joint("f", true, true, 3, 5, 100, true, 0, 32).ok);       // one mask for all chains
    CHECK(check_score_joint("f", true, true, 3, 5, 8, true, 32, 32).ok);
    CHECK(check_score_joint("f", true, false, 0, 5, 8, false, 7, 32).ok);       // (no mask: its stride is not read)
    c = check_score_joint("who", false, false, 0, 5, 8, false, 0, 32);
    CHECK(!c.ok && std::strstr(c.message, "who") && std::strstr(c.message, "null output"));
    c = check_score_joint("who", true, false, 2, 5, 8, false, 0, 32);
    CHECK(!c.ok && std::strstr(c.message, "2 coordinates"));
    c = check_score_joint("who", true, false, 0, 5, 7, false, 0, 32);
    CHECK(!c.ok && std::strstr(c.message, "ld_out 7 < nfeatures + 3 = 8"));
    c = check_score_joint("who", true, false, 0, 5, 8, true, 31, 32);
    CHECK(!c.ok && std::strstr(c.message, "ld_slots 31"));
    c = check_score_joint("who", true, false, 0, 0xffffffffu, 0xffffffffull, false, 0, 1);
    CHECK(!c.ok);                                             // nfeatures + 3 does not wrap
    std::vector<char> longname(500, 'x');
    longname.back() = 0;
    c = check_score_joint(longname.data(), false, false, 0, 5, 8, false, 0, 32);   // the message is cut, not overrun
    CHECK(!c.ok && std::strlen(c.message) == sizeof c.message - 1);

    CHECK(check_keep_best("k", true, 8, 100, 100, 100).ok);
    CHECK(check_keep_best("k", true, 1, 0, 0, 0).ok);
    c = check_keep_best("k", false, 8, 100, 100, 100);
    CHECK(!c.ok && std::strstr(c.message, "null argument"));
    c = check_keep_best("k", true, 0, 100, 100, 100);
    CHECK(!c.ok && std::strstr(c.message, "ld_joint"));
    c = check_keep_best("k", true, 8, 100, 99, 100);
    CHECK(!c.ok && std::strstr(c.message, "ld_z 99 < nrows 100"));
    c = check_keep_best("k", true, 8, 100, 100, 99);
    CHECK(!c.ok && std::strstr(c.message, "ld_best 99 < nrows 100"));
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("joint math ok\n");
  return 0;
}
