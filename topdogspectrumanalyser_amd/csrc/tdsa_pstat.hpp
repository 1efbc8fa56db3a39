// tdsa_pstat.hpp - launcher of the power statistics (tdsa_pstat.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tdsa {

constexpr int kPstatThreads = 256;
constexpr int kPstatMaxStreams = 256;                 // C, streams of a handle
constexpr int kPstatTile = 8192;                      // samples of one stream a workgroup takes at a time
constexpr int kPstatMaxGrid = 2048;                   // workgroups of a launch, all streams together; each strides over the tiles
constexpr int kPstatBinsPerOctave = 32;               // the five leading mantissa bits
constexpr int kPstatOctaves = 64;
constexpr int kPstatBins = kPstatOctaves * kPstatBinsPerOctave;   // 2048
constexpr int kPstatExponents = 256;                  // words of msum: one per biased exponent
constexpr int kPstatExpLoMin = -126;
constexpr int kPstatExpLoMax = 64;
// A launch brings at most this many samples per stream, so that a workgroup's 32-bit LDS counts cannot wrap whatever the
// grid is; the launcher cuts a longer call into launches (a C3 second is one).  A multiple of the tile, so every
// launch's tiles keep the stream's 16-byte alignment.
constexpr long long kPstatMaxLaunchSamples = 1ll << 26;
// the LDS of a workgroup: the histogram (32-bit counts), the mantissa sums, the uint8 table, the class counts and bounds
constexpr int kPstatLdsBytes = kPstatBins * 4 + kPstatExponents * 8 + 256 * 4 + 8 * 4;

// one stream's record, as tdsa_pstat_read hands it back (include/tdsa_hip.h); the kernel adds into it
struct PstatRecord {
  unsigned long long n_total, n_nan, n_gated, n_inf, n_zero, n_under, n_over;
  unsigned max_bits, min_bits;
  unsigned reserved[2];
};
static_assert(sizeof(PstatRecord) == 72, "record layout");

struct PstatLaunch {
  const void* in = nullptr;      // stream c at in + c * in_stride samples of the format
  int fmt = 0;                   // TDSA_IN_I8 / _U8 / _C64
  int C = 1;
  size_t n = 0;                  // samples per stream
  size_t in_stride = 0;
  int bin_base = 0;              // (exp_lo + 127) << 5: the float bits >> 18 of the window's first edge
  float gate = 0.0f;
  PstatRecord* rec = nullptr;               // [C]
  unsigned long long* msum = nullptr;       // [C][kPstatExponents]
  unsigned long long* hist = nullptr;       // [C][kPstatBins]
};

hipError_t launch_pstat(const PstatLaunch& a, hipStream_t s);

}  // namespace tdsa
