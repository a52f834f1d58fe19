// Host test of common_amd/csrc/row_range.hpp alone: the row-range test bind_view makes, at the ranges whose end wraps in
// uint64 (row0 + nrows <= view_rows accepted every one of them).
#include "row_range.hpp"

#include <cstdio>

int main() {
  const uint64_t top = ~uint64_t(0);                       // 2^64 - 1
  struct Case { uint64_t row0, nrows, view_rows; bool within; };
  const Case cases[] = {
      {0, 0, 0, true},         {0, 10, 10, true},       {10, 0, 10, true},  {3, 7, 10, true},
      {top, 0, top, true},     {0, top, top, true},
      {5, top - 4, 10, false},                             // row0 + nrows wraps to 0
      {11, top, 10, false},                                // ... to 10
      {1, 10, 10, false},      {11, 0, 10, false},      {0, 11, 10, false},
      {top, 2, top, false},                                // ... to 1
      {top, top, top, false},  {1, 0, 0, false},
  };
  int failures = 0;
  for (const Case &c : cases)
    if (msc::rows_within(c.row0, c.nrows, c.view_rows) != c.within) {
      failures++;
      std::printf("FAIL rows_within(%llu, %llu, %llu) != %d\n", (unsigned long long)c.row0, (unsigned long long)c.nrows,
                  (unsigned long long)c.view_rows, (int)c.within);
    }
  if (failures) return 1;
  std::printf("row_range ok\n");
  return 0;
}
