// tdsa_constellation.hpp - launchers of the constellation analysis (tdsa_constellation.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr int kCstBlock = 8192;      // numpy's add.reduce folds consecutive blocks of this many elements
constexpr int kCstMaxPoints = 64;    // reference points a table may hold
constexpr int kCstMaxBins = 128;     // histogram bins per axis (the reference's _resolution)

// One reference table as the symbol pass reads it: separable tables (the point set is X x Y) hold the level sets,
// others every point.  T = float or double, the dtype of the reference's _CONST_REFS entry.
struct CstTable {
  int n_points = 0;    // 0: no table (the reference's EVM is None)
  int is_f64 = 0;
  int separable = 0;
  int nx = 0, ny = 0;  // separable: level counts of x and y
  const void* dev = nullptr;   // T[2][kCstMaxPoints]: separable {xs, ys}, else {px, py}
};

struct CstLaunch {
  const void* in = nullptr;    // segment s = samples [s * hop, s * hop + seg_len) of the input
  int fmt = 0;                 // TDSA_IN_I8 / _U8 / _C64
  long long seg_len = 0, hop = 0;
  int n_seg = 0;
  float* bs_pow = nullptr;     // [n_seg][nblk] per-block pairwise sums of |x|^2
  void* bs_evm = nullptr;      // [n_seg][nblk] per-block pairwise sums of the minimum distances (T)
  float* rms = nullptr;        // [n_seg]
  double* evm = nullptr;       // [n_seg] (NaN when the table is empty)
  unsigned* counts = nullptr;  // [n_seg][bins][bins] or null: no histogram (the power pass zeroes it)
  float* tail = nullptr;       // segment 0: the last n_tail normalised i, then q (float32), or null
  int n_tail = 0;
  int bins = kCstMaxBins;
  double range = 1.5, step = 0.0;   // edges = linspace(-range, range, bins + 1): k * step - range, last = range
  CstTable tab;
};

// the three passes in stream order: power sums, symbol pass (AGC, distances, histogram, tail), EVM fold
hipError_t launch_constellation(const CstLaunch& a, hipStream_t s);

}  // namespace tdsa
