// Host test of common_amd/csrc/host_checks.hpp alone: require_permutation, the check msc_zmatrix_counts / _result,
// msc_zmatrix_partition_refine and msc_partition_refine_vi make of a caller's visiting order -- the status and the entry
// the message names.
#include "host_checks.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

// order: null when `null`, else the entries given; want_ok / want_entry: what the check must find
static void expect(const char *name, bool null, std::vector<uint32_t> order, uint32_t m, bool want_ok, uint32_t want_entry) {
  const msc::PermutationCheck c = msc::require_permutation(null ? nullptr : order.data(), m, "who");
  bool good = c.ok == want_ok;
  if (want_ok) {
    good = good && c.message[0] == 0;
  } else {
    char want[192];
    std::snprintf(want, sizeof want, "who: order is not a permutation of [0, %u): entry %u is %u", m, want_entry,
                  order[want_entry]);
    good = good && c.entry == want_entry && std::strcmp(c.message, want) == 0;
  }
  if (!good) {
    failures++;
    std::printf("FAIL %s: ok = %d, entry = %u, message = \"%s\"\n", name, (int)c.ok, c.entry, c.message);
  }
}

int main() {
  expect("m = 1", false, {0}, 1, true, 0);
  expect("m = 1, entry equal to m", false, {1}, 1, false, 0);
  expect("identity", false, {0, 1, 2, 3, 4}, 5, true, 0);
  expect("reversed", false, {4, 3, 2, 1, 0}, 5, true, 0);
  expect("repeated entry", false, {0, 3, 1, 3, 2}, 5, false, 3);         // the second 3, not the first
  expect("repeated first entry", false, {2, 2, 0, 1, 4}, 5, false, 1);
  expect("entry equal to m", false, {0, 1, 5, 3, 4}, 5, false, 2);
  expect("entry equal to m, last", false, {0, 1, 2, 3, 5}, 5, false, 4);
  expect("entry far beyond m", false, {0, 0xffffffffu, 2, 3, 4}, 5, false, 1);
  expect("out of range before a repeat", false, {1, 7, 1, 0, 2}, 5, false, 1);   // the first fault is the one named
  expect("null order", true, {}, 5, true, 0);
  expect("null order, m = 1", true, {}, 1, true, 0);
  if (failures) return 1;
  std::printf("host_checks ok\n");
  return 0;
}
