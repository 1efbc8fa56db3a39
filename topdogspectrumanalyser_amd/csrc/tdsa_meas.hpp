// tdsa_meas.hpp - launcher of the channel measurements (tdsa_meas.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tdsa {

constexpr int kMeasThreads = 256;
constexpr int kMeasMaxBins = 16384;                   // the row lives in LDS
constexpr int kMeasMaxChannels = 16;                  // C, channel records per row
constexpr int kMeasOwn = 64;                          // consecutive bins a thread owns in the occupied-bandwidth scan
constexpr int kMeasMaxGrid = 2048;                    // workgroups of a launch; each strides over the rows
// The row in LDS is padded by one float per 64 bins (bin i at float i + i / 64), so that the 64 threads of a wave, each
// walking its own 64 consecutive bins, read 64 distinct banks.
constexpr int kMeasRowFloats = kMeasMaxBins + kMeasMaxBins / kMeasOwn;
// the folds' scratch (four waves of pairs, doubles, integers), the scan's wave totals, the crossing words, the scalars
constexpr int kMeasStaticLdsBytes = 512;
constexpr int kMeasMaxLdsBytes = kMeasRowFloats * 4 + kMeasStaticLdsBytes;   // ~65.5 KiB: two workgroups per CU

constexpr int kMeasFlagEmpty = 1;                     // the occupied-bandwidth range holds no power: T is not > 0
constexpr int kMeasFlagInf = 2;                       // ... or a +inf bin: T = +inf
constexpr int kMeasFlagMaskFail = 4;                  // a bin above its limit

// one row's record and one channel's, as tdsa_meas_process* hand them back (include/tdsa_hip.h)
struct MeasRow {
  double obw_total, x_lo, x_hi;
  int32_t k_lo, k_hi, xdb_lo, xdb_hi, peak_bin, n_nan, n_fail, worst_bin, first_fail, last_fail, flags;
  float peak_db, worst_margin;
  int32_t reserved;
};
struct MeasChannel {
  double power;
  float peak_db;
  int32_t peak_bin, n_nan, reserved;
};
static_assert(sizeof(MeasRow) == 80 && sizeof(MeasChannel) == 24, "record layout");

struct MeasLaunch {
  const float* rows = nullptr;   // [n_rows][n]
  size_t n_rows = 0;
  int n = 0;
  int C = 1;                     // channels, inclusive bin ranges
  int16_t ch_lo[kMeasMaxChannels] = {}, ch_hi[kMeasMaxChannels] = {};
  int obw_lo = 0, obw_hi = 0;    // the range of the occupied bandwidth and of the x-dB width
  double f = 0.0;                // the fraction: the targets are T (1 - f) / 2 and T (1 + f) / 2
  float xdb = 0.0f;
  const float* limit = nullptr;  // [n] or null: no limit line
  int relative = 0;              // the limit is relative to channel 0's peak_db
  MeasRow* row_rec = nullptr;    // [n_rows]
  MeasChannel* ch_rec = nullptr; // [n_rows][C]
};

hipError_t meas_prepare();       // on the current device, before the first launch: the kernel's dynamic LDS limit
hipError_t launch_meas(const MeasLaunch& a, hipStream_t s);

}  // namespace tdsa
