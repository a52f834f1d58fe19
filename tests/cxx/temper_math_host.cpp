// Host build of common_amd/csrc/temper_math.hpp for tests/test_temper_cpu.py: the likelihood sum of a joint row, the swap
// log ratio and the accept rule of an exchange, the pairing by parity, the permutation check, a ladder's walk, the
// annealing increment and the shape checks -- a program of its own that includes nothing else of the library, run plain
// and under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "temper_math.hpp"

using namespace msc::temper;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      failures++;                                                      \
    }                                                                  \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a uniform per pair from a table: what the kernel takes from Philox
struct TableUniform {
  const float *u;
  float operator()(uint32_t j) const { return u[j]; }
};

// joint rows of F = 2 features with likelihoods l[i] (split over the two entries), a and p filled with values that
// must not be read
static std::vector<double> rows_of(const std::vector<double> &l, uint64_t ld) {
  std::vector<double> j(l.size() * ld, 777.0);
  for (size_t i = 0; i < l.size(); i++) {
    j[i * ld + 2] = l[i];
    j[i * ld + 3] = 0.0;
  }
  return j;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

  // ---- the likelihood: entries [2, 2 + F) in the written order, neither a nor p ----
  {
    const double row[] = {9.0, 1e16, 1e16, 1.0, 1.0, -1e16, 5.0};     // F = 4: total, a, d0 .. d3, p
    volatile double w = row[2];
    w = w + row[3];
    w = w + row[4];
    w = w + row[5];
    CHECK(same_bits(chain_loglik(row, 4), w) && chain_loglik(row, 4) == 0.0);   // ((1e16 + 1) + 1) - 1e16
    CHECK(!same_bits(chain_loglik(row, 4), row[2] + row[5] + row[3] + row[4]));
    CHECK(chain_loglik(row, 0) == 0.0 && chain_loglik(row, 1) == 1e16);
    const double neg[] = {0.0, 0.0, -inf, 1.0, 0.0};
    CHECK(chain_loglik(neg, 2) == -inf);
    const double clash[] = {0.0, 0.0, -inf, inf, 0.0};
    CHECK(std::isnan(chain_loglik(clash, 2)));
  }

  // ---- the swap ratio: its sign, antisymmetry, exact widening ----
  CHECK(swap_log_ratio(1.0f, 0.5f, -10.0, -4.0) == 3.0);       // the hotter chain fits better: the swap is favoured
  CHECK(swap_log_ratio(1.0f, 0.5f, -4.0, -10.0) == -3.0);
  CHECK(swap_log_ratio(0.5f, 1.0f, -10.0, -4.0) == -swap_log_ratio(1.0f, 0.5f, -10.0, -4.0));   // in the temperatures
  CHECK(swap_log_ratio(1.0f, 0.5f, -4.0, -10.0) == -swap_log_ratio(1.0f, 0.5f, -10.0, -4.0));   // in the likelihoods
  CHECK(swap_log_ratio(0.3f, 0.3f, -4.0, -10.0) == 0.0);
  CHECK(same_bits(swap_log_ratio(0.1f, 0.7f, 1.0, 2.0), (double)0.1f - (double)0.7f));
  CHECK(std::isnan(swap_log_ratio(1.0f, 0.5f, -inf, -inf)));   // inf - inf
  CHECK(std::isnan(swap_log_ratio(0.5f, 0.5f, -inf, 0.0)));    // 0 * inf
  CHECK(std::isnan(swap_log_ratio(1.0f, 0.5f, nan, 0.0)));
  CHECK(swap_log_ratio(1.0f, 0.5f, -inf, 0.0) == inf && swap_log_ratio(1.0f, 0.5f, 0.0, -inf) == -inf);

  // ---- the accept rule: log u < r, a non-finite r rejects ----
  CHECK(swap_accepts(std::log(0.5), 0.0) && swap_accepts(std::log(0.5), 3.0));
  CHECK(!swap_accepts(std::log(0.5), -1.0) && swap_accepts(std::log(0.5), -0.5));
  CHECK(!swap_accepts(-0.5, -0.5));                            // strictly below
  CHECK(swap_accepts(-inf, -700.0));                           // u == 0 accepts whatever is finite
  CHECK(!swap_accepts(-1.0, nan) && !swap_accepts(-inf, nan));
  CHECK(!swap_accepts(-1.0, inf) && !swap_accepts(-1.0, -inf) && !swap_accepts(-inf, -inf));

  // ---- the pairing: even and odd parity, odd and even R; both parities cover every pair once ----
  for (uint32_t R = 1; R <= 7; R++) {
    CHECK(ladder_pairs(R) == R - 1);
    for (uint64_t parity : {0ull, 1ull, 6ull, 7ull, ~0ull}) {
      uint32_t last = ~0u;
      for (uint32_t j = 0; j + 1 < R; j++) {
        if (!pair_active(j, parity)) continue;
        CHECK(j % 2 == parity % 2);
        CHECK(last == ~0u || j >= last + 2);                   // disjoint
        last = j;
      }
    }
    for (uint32_t j = 0; j + 1 < R; j++) CHECK(pair_active(j, 0) != pair_active(j, 1));
  }
  CHECK(ladder_pairs(0) == 0);
  CHECK(pair_active(0, 0) && !pair_active(1, 0) && pair_active(2, 4) && pair_active(3, 5) && !pair_active(3, 4));

  // ---- the permutation check and the holder ----
  {
    const int32_t ok[] = {2, 0, 3, 1}, twice[] = {2, 0, 2, 1}, out[] = {0, 1, 2, 4}, neg[] = {0, -1, 2, 1};
    CHECK(ladder_is_permutation(ok, 4) && !ladder_is_permutation(twice, 4) && !ladder_is_permutation(out, 4) &&
          !ladder_is_permutation(neg, 4));
    CHECK(ladder_is_permutation(ok, 0));
    const int32_t one[] = {0}, notone[] = {1};
    CHECK(ladder_is_permutation(one, 1) && !ladder_is_permutation(notone, 1));
    CHECK(rung_holder(ok, 4, 0) == 1 && rung_holder(ok, 4, 3) == 2 && rung_holder(twice, 4, 3) == 4);
  }

  // ---- a ladder's walk ----
  for (uint32_t R : {4u, 5u}) {
    const uint64_t ld = 6;                                    // F = 2, one column of padding
    std::vector<double> l(R);
    for (uint32_t i = 0; i < R; i++) l[i] = -10.0 + 3.0 * i;  // chain i: -10, -7, ...
    const std::vector<double> joint = rows_of(l, ld);
    for (uint64_t parity : {0ull, 1ull}) {
      std::vector<float> beta(R), u(R, 0.5f);
      std::vector<int32_t> rung(R);
      for (uint32_t i = 0; i < R; i++) {
        rung[i] = (int32_t)((i + 1) % R);                     // chain i holds rung i + 1, the last chain rung 0
        beta[i] = 1.0f - 0.125f * (float)rung[i];
      }
      const std::vector<float> beta0 = beta;
      const std::vector<int32_t> rung0 = rung;
      std::vector<uint32_t> prop(R - 1, 10), acc(R - 1, 20);
      CHECK(exchange_ladder(joint.data(), ld, 2, R, beta.data(), rung.data(), parity, TableUniform{u.data()}, prop.data(),
                            acc.data()));
      CHECK(ladder_is_permutation(rung.data(), R));
      for (uint32_t j = 0; j + 1 < R; j++) {
        const bool active = j % 2 == parity % 2;
        CHECK(prop[j] == 10u + active);
        const uint32_t a = rung_holder(rung0.data(), R, j), b = rung_holder(rung0.data(), R, j + 1);
        const double r = swap_log_ratio(beta0[a], beta0[b], l[a], l[b]);
        const bool swapped = active && swap_accepts(std::log(0.5), r);
        CHECK(acc[j] == 20u + swapped);
        if (!active) continue;                                // (its two chains may have moved in the pairs beside it)
        CHECK(rung[a] == (int32_t)(swapped ? j + 1 : j) && rung[b] == (int32_t)(swapped ? j : j + 1));
        CHECK(beta[a] == (swapped ? beta0[b] : beta0[a]) && beta[b] == (swapped ? beta0[a] : beta0[b]));
      }
      for (uint32_t i = 0; i < R; i++) CHECK(beta[i] == 1.0f - 0.125f * (float)rung[i]);   // beta follows the rung
    }
    // a NaN and a -inf likelihood: pairs that involve the NaN reject; -inf against a finite one is decided by the sign
    {
      std::vector<double> lbad = l;
      lbad[0] = nan;                                          // holds rung 1
      lbad[2] = -inf;                                         // holds rung 3
      const std::vector<double> jbad = rows_of(lbad, ld);
      for (uint64_t parity : {0ull, 1ull}) {
        std::vector<float> beta(R), u(R, 0.25f);
        std::vector<int32_t> rung(R);
        for (uint32_t i = 0; i < R; i++) {
          rung[i] = (int32_t)((i + 1) % R);
          beta[i] = 1.0f - 0.125f * (float)rung[i];
        }
        std::vector<uint32_t> prop(R - 1, 0), acc(R - 1, 0);
        CHECK(exchange_ladder(jbad.data(), ld, 2, R, beta.data(), rung.data(), parity, TableUniform{u.data()}, prop.data(),
                              acc.data()));
        CHECK(rung[0] == 1);                                  // the NaN chain never moved
        CHECK(acc[0] == 0 && acc[1] == 0);                    // pairs (0, 1) and (1, 2) hold it
        if (parity == 0) CHECK(prop[2] == 1 && acc[2] == 0);  // rung 2 (finite) above rung 3 (-inf): r = -inf
        for (uint32_t i = 0; i < R; i++) CHECK(beta[i] == 1.0f - 0.125f * (float)rung[i]);
      }
    }
    // a broken permutation: false, nothing changed
    {
      std::vector<float> beta(R, 0.5f), u(R, 0.0f);
      std::vector<int32_t> rung(R, 0);
      std::vector<uint32_t> prop(R - 1, 3), acc(R - 1, 4);
      CHECK(!exchange_ladder(joint.data(), ld, 2, R, beta.data(), rung.data(), 0, TableUniform{u.data()}, prop.data(),
                             acc.data()));
      for (uint32_t i = 0; i < R; i++) CHECK(rung[i] == 0 && beta[i] == 0.5f);
      for (uint32_t j = 0; j + 1 < R; j++) CHECK(prop[j] == 3 && acc[j] == 4);
    }
  }
  {   // one rung: nothing to propose, and the arrays of no pair are not touched
    const std::vector<double> joint = rows_of({-1.0}, 5);
    float beta = 1.0f, u = 0.5f;
    int32_t rung = 0;
    CHECK(exchange_ladder(joint.data(), 5, 2, 1, &beta, &rung, 0, TableUniform{&u}, nullptr, nullptr));
    CHECK(beta == 1.0f && rung == 0);
  }

  // ---- the annealing step ----
  {
    double w = 1.5;
    CHECK(anneal_step(0.25f, 0.5f, -8.0, &w) && w == -0.5);
    CHECK(anneal_step(0.5f, 0.25f, -8.0, &w) && w == 1.5);    // a step back takes it off again
    CHECK(!anneal_step(0.5f, 0.5f, -inf, &w) && w == 1.5);    // equal temperatures: untouched, no 0 * inf
    CHECK(!anneal_step(0.5f, 0.5f, nan, &w) && w == 1.5);
    CHECK(anneal_step(0.0f, 0.5f, -inf, &w) && w == -inf);    // a state the data rule out has no weight
    w = 0.0;
    CHECK(anneal_step(0.0f, 1.0f, nan, &w) && std::isnan(w));
    w = 2.0;
    volatile double d = (double)0.7f - (double)0.1f, want = d * 3.0;
    want = 2.0 + want;
    CHECK(anneal_step(0.1f, 0.7f, 3.0, &w) && same_bits(w, want));
  }

  // ---- the shape checks ----
  {
    msc::joint::JointCheck c = check_exchange("x", true, 4, 12, 8, 5);
    CHECK(c.ok && c.message[0] == 0);
    CHECK(check_exchange("x", true, 1, 7, 3, 0).ok && check_exchange("x", true, 5, 0, 8, 5).ok);
    c = check_exchange("who", false, 4, 12, 8, 5);
    CHECK(!c.ok && std::strstr(c.message, "who") && std::strstr(c.message, "null argument"));
    c = check_exchange("who", true, 0, 12, 8, 5);
    CHECK(!c.ok && std::strstr(c.message, "nrungs is 0"));
    c = check_exchange("who", true, 5, 12, 8, 5);
    CHECK(!c.ok && std::strstr(c.message, "12 chains") && std::strstr(c.message, "5 rungs"));
    c = check_exchange("who", true, 4, 12, 7, 5);
    CHECK(!c.ok && std::strstr(c.message, "ld_joint 7 < nfeatures + 3 = 8"));
    CHECK(!check_exchange("who", true, 1, 1, 0xffffffffull, 0xffffffffu).ok);   // nfeatures + 3 does not wrap
    CHECK(check_anneal_weights("a", true, 8, 5).ok);
    c = check_anneal_weights("who", false, 8, 5);
    CHECK(!c.ok && std::strstr(c.message, "null argument"));
    c = check_anneal_weights("who", true, 7, 5);
    CHECK(!c.ok && std::strstr(c.message, "ld_joint 7"));
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("temper math ok\n");
  return 0;
}
