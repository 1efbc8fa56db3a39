// tdsa_modq.hpp - launcher of the modulation quality stage (tdsa_modq.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_modq_math.hpp"

namespace tdsa {

constexpr int kModqThreads = 256;
constexpr int kModqWaves = kModqThreads / 64;
constexpr int kModqSums = 4;                         // the most float64 sums one reduction folds side by side
// the table and r_abs, the counts of the two rounds, a reduction's wave sums (float64, and the peak's pair)
constexpr int kModqStaticLdsBytes = kModqMaxPoints * (8 + 4) + 2 * kModqMaxPoints * 4 + kModqWaves * kModqSums * 8 + kModqWaves * 8;
// a segment's symbols and their indices beside them: under 38 KiB of the CU's 160
constexpr int kModqMaxLdsBytes = kModqMaxSymbols * (8 + 1) + kModqStaticLdsBytes;

// one segment's record, as tdsa_modq_process* hand it back (include/tdsa_hip.h: tdsa_modq_record)
struct ModqRecord {
  float a_re, a_im, c_re, c_im;
  double s_y[2], s_yy, s_ry[2], s_cy[2];
  double err_sumsq, ref_sumsq, mag_sumsq, phase_sumsq;
  float err_peak;
  uint32_t err_peak_k, changed, flags;
  uint32_t reserved[2];
};
static_assert(sizeof(ModqRecord) == 128, "record layout");

// what tdsa_modq_set_points uploads: the table, |r_i| in float32, 1 / rms of the table
struct ModqTable {
  float2 r[kModqMaxPoints];
  float r_abs[kModqMaxPoints];
  float inv_rho;
  int T;
};

struct ModqLaunch {
  const float2* in = nullptr;    // segment s = symbols [s * in_stride, s * in_stride + K)
  long long in_stride = 0;
  int n_seg = 0, K = 0;
  const ModqTable* table = nullptr;   // device
  uint8_t* idx = nullptr;        // [n_seg][out_stride] the indices of the second round
  float2* err = nullptr;         // the same shape, the error vectors, or null
  long long out_stride = 0;
  ModqRecord* rec = nullptr;     // [n_seg]
};

hipError_t launch_modq(const ModqLaunch& a, hipStream_t s);

}  // namespace tdsa
