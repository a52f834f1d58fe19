// host_checks.hpp -- checks of host arrays that several entry points make, each written once.  Host only: no HIP header,
// nothing of the library, builds with the plain host compiler (tests/cxx/test_host_checks.cpp).
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

namespace msc {

// What require_permutation found: ok, or the first entry that is out of range or repeats an earlier one, with the
// message that names it.
struct PermutationCheck {
  bool ok = true;
  uint32_t entry = 0;
  char message[192] = "";
};

// Is host_order a permutation of [0, m)?  A null order stands for the identity and is accepted.  who: the entry point, as
// the message names it.
inline PermutationCheck require_permutation(const uint32_t *host_order, uint32_t m, const char *who) {
  PermutationCheck c;
  if (!host_order) return c;
  std::vector<uint8_t> seen(m, 0);
  for (uint32_t a = 0; a < m; a++) {
    if (host_order[a] >= m || seen[host_order[a]]) {
      c.ok = false;
      c.entry = a;
      std::snprintf(c.message, sizeof c.message, "%s: order is not a permutation of [0, %u): entry %u is %u", who, m, a,
                    host_order[a]);
      return c;
    }
    seen[host_order[a]] = 1;
  }
  return c;
}

}  // namespace msc
