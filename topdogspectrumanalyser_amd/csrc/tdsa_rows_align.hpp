// tdsa_rows_align.hpp - which load path a kernel over [rows][n] float32 rows may take.  Plain C++ (no HIP): the launcher
// includes it, and tests/peaks_align_host.cpp enumerates it on the host.
#pragma once
#include <stdint.h>

namespace tdsa {

// Row r starts at rows + r * n floats.  EVERY row starts on 16 bytes exactly when the base does and n is a multiple of
// four floats; only then may a kernel read a row as 16-byte vectors.  (n % 4 == 0 alone is not enough: the base may be any
// float of a larger buffer.)
inline bool rows_take_vec16(const void* rows, int n) {
  return reinterpret_cast<uintptr_t>(rows) % 16 == 0 && n % 4 == 0;
}

}  // namespace tdsa
