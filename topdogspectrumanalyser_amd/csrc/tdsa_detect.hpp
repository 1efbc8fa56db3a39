// tdsa_detect.hpp - launcher of the signal detection (tdsa_detect.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tdsa {

constexpr int kDetThreads = 256;
constexpr int kDetMaxBins = 16384;                    // the row lives in LDS
constexpr int kDetMaxSignals = 64;                    // S, signal records per row
constexpr int kDetWords = kDetMaxBins / 64;           // 64-bit mask words of a row: one per thread
constexpr int kDetMaxGrid = 2048;                     // workgroups of a launch; each strides over the rows
// mask and stop words, the digit histogram, the runs of the first S, the scans' scratch and the row's scalars
constexpr int kDetStaticLdsBytes = 2 * kDetWords * 8 + 256 * 4 + kDetMaxSignals * 8 + 64;
constexpr int kDetMaxLdsBytes = kDetMaxBins * 4 + kDetStaticLdsBytes;   // ~69 KiB: two workgroups per CU

constexpr int kDetFlagNanFloor = 1;                   // the floor is a NaN: no threshold, no signal, no occupancy

// one row's record and one signal's, as tdsa_detect_process* hand them back (include/tdsa_hip.h)
struct DetRow {
  float floor, thr;
  int32_t n_found, n_over, flags;
  int32_t reserved[3];
};
struct DetSignal {
  int32_t start, stop, peak_bin, x_lo, x_hi;
  float peak_db;
  double power, moment;
};
static_assert(sizeof(DetRow) == 32 && sizeof(DetSignal) == 40, "record layout");

struct DetLaunch {
  const float* rows = nullptr;   // [n_rows][n]
  size_t n_rows = 0;
  int n = 0;
  int lo = 0, hi = 0, rank = 0;  // the search range, inclusive, and the order statistic within it
  float margin = 0.0f, xdb = 0.0f;
  int min_width = 1, max_gap = 0, S = 1;
  DetRow* row_rec = nullptr;     // [n_rows]
  DetSignal* sig_rec = nullptr;  // [n_rows][S]
  unsigned* occ = nullptr;       // [n]
};

hipError_t detect_prepare();     // on the current device, before the first launch: the kernel's dynamic LDS limit
hipError_t launch_detect(const DetLaunch& a, hipStream_t s);

}  // namespace tdsa
