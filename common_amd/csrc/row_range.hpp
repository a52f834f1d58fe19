// row_range.hpp -- whether rows [row0, row0 + nrows) lie within a view of view_rows rows, computed without wrapping
// (row0 + nrows <= view_rows wraps in uint64: row0 = 2^64 - 5, nrows = 10 passed it).  Host only: no HIP header, builds
// with the plain host compiler (tests/cxx/test_row_range.cpp).
#pragma once

#include <cstdint>

namespace msc {

inline bool rows_within(uint64_t row0, uint64_t nrows, uint64_t view_rows) {
  return nrows <= view_rows && row0 <= view_rows - nrows;
}

}  // namespace msc
