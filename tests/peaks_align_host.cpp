// The predicate launch_marker_peaks chooses its load path by (tdsa_rows_align.hpp), enumerated on the host: it must hold
// exactly when every row of [rows][n] floats starts on a 16-byte boundary.  Prints one line per wrong answer; exit 0 = none.
#include <cstdio>

#include "tdsa_rows_align.hpp"

int main() {
  int wrong = 0, yes = 0;
  for (uintptr_t base = 4096; base < 4096 + 64; ++base) {              // every byte offset, the ones a float cannot have too
    for (int n = 1; n <= 70; ++n) {
      bool every_row = true;
      for (int r = 0; r < 9; ++r) every_row = every_row && (base + uintptr_t(r) * n * sizeof(float)) % 16 == 0;
      const bool got = tdsa::rows_take_vec16(reinterpret_cast<const void*>(base), n);
      yes += got;
      if (got != every_row) {
        std::printf("base %% 16 = %d, n = %d: predicate %d, rows aligned %d\n", int(base % 16), n, int(got), int(every_row));
        ++wrong;
      }
    }
  }
  std::printf("%d combinations take the 16-byte loads, %d wrong\n", yes, wrong);
  return wrong != 0 || yes != 4 * 17;
}
