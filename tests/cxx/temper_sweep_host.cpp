// Host build of the tempered sweep's arithmetic in common_amd/csrc/temper_math.hpp for tests/test_temper_sweep_cpu.py:
// temper::tempered_add -- how a score partial goes onto a slot's score at a temperature -- and temper::beta_ok -- which
// temperatures a chain can be swept at.  A program of its own that includes nothing else of the library, run plain and
// under the address and undefined-behaviour sanitizers.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

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

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// xorshift64*: the test's own stream
static uint64_t rng_state = 0x853C49E6748FEA9Bull;
static uint64_t next_u64() {
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
// a finite float of a score's size: sign, a magnitude between 2^-20 and 2^12, a full random mantissa
static float next_score() {
  const uint64_t r = next_u64();
  const uint32_t bits = (uint32_t)(r & 0x807FFFFFu) | ((107u + (uint32_t)((r >> 40) % 33u)) << 23);
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

  // ---- beta = 1: the bits of the untempered add, over random scores ----
  for (int i = 0; i < 200000; i++) {
    const float p = next_score(), sk = next_score();
    volatile float sum = sk + p;
    CHECK(same_bits(tempered_add(1.0f, p, sk), sum));
  }
  // ... and where a slot cannot hold the row (-inf partial) or is closed (-inf sum)
  for (int i = 0; i < 1000; i++) {
    const float x = next_score();
    CHECK(same_bits(tempered_add(1.0f, -inf, x), -inf));
    CHECK(same_bits(tempered_add(1.0f, x, -inf), -inf));
    volatile float a = x + -inf, b = -inf + x;
    CHECK(same_bits(tempered_add(1.0f, -inf, x), a) && same_bits(tempered_add(1.0f, x, -inf), b));
  }
  CHECK(same_bits(tempered_add(1.0f, -inf, -inf), -inf));
  CHECK(same_bits(tempered_add(1.0f, 0.0f, -0.0f), 0.0f) && same_bits(tempered_add(1.0f, -0.0f, -0.0f), -0.0f));

  // ---- a temperature in between: ONE rounding, where sk + beta * p has two ----
  {
    const float beta = 0.3f;
    int differ = 0, total = 0;
    for (int i = 0; i < 200000; i++) {
      const float p = next_score(), sk = next_score();
      volatile float prod = beta * p;                        // (rounded here: the compiler may not fuse it)
      volatile float two = sk + prod;
      const float one = tempered_add(beta, p, sk);
      // the fused form is the double expression rounded once: a float product is exact in double, and the double sum of
      // two such numbers rounds to float as the exact sum does except at a double rounding, which costs an ulp at most
      const double exact = (double)beta * (double)p + (double)sk;
      CHECK(std::fabs((double)one - exact) <= std::fabs((double)two - exact));
      differ += !same_bits(one, two);
      total++;
    }
    std::printf("beta 0.3: the single rounding shows in %d of %d inputs\n", differ, total);
    CHECK(differ > 0);
    CHECK(same_bits(tempered_add(beta, -inf, 1.5f), -inf) && same_bits(tempered_add(beta, 2.0f, -inf), -inf));
    CHECK(same_bits(tempered_add(2.0f, 1.5f, 0.25f), 3.25f));
  }

  // ---- the temperatures a chain can be swept at ----
  CHECK(beta_ok(0.0f) && beta_ok(-0.0f) && beta_ok(0.25f) && beta_ok(1.0f) && beta_ok(1.7f) && beta_ok(FLT_MAX));
  CHECK(beta_ok(FLT_MIN) && beta_ok(std::numeric_limits<float>::denorm_min()));
  CHECK(!beta_ok(nan) && !beta_ok(-nan) && !beta_ok(-1e-30f) && !beta_ok(-inf) && !beta_ok(inf));
  CHECK(!beta_ok(-1.0f) && !beta_ok(-FLT_MAX) && !beta_ok(-std::numeric_limits<float>::denorm_min()));

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("temper sweep math ok\n");
  return 0;
}
