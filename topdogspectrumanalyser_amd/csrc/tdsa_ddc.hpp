// tdsa_ddc.hpp - launcher of the zoom front end (tdsa_ddc.hip): unpack, NCO, mixer and
// decimating FIR in one pass over raw IQ, with the filter history kept on the device between calls.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr int kDdcMinDecimation = 2;
constexpr int kDdcMaxDecimation = 4096;
constexpr int kDdcMaxTapsPerPhase = 64;   // T <= 64 D
constexpr int kDdcBlock = 8;              // outputs per thread, and phases per register block (taps padded to it)
constexpr int kDdcNcoTable = 4096;        // exp(-2 pi j k / 4096): the rotator's top 12 phase bits

// taps per phase rounded up to the register block: the padded tap table is [ddc_phases(T, D)][D] and the history
// holds the last ddc_phases(T, D) * D mixed samples
inline int ddc_phases(int n_taps, int D) {
  const int q = (n_taps + D - 1) / D;
  return (q + kDdcBlock - 1) / kDdcBlock * kDdcBlock;
}

struct DdcLaunch {
  const void* in = nullptr;        // this call's raw input, n_in samples (TDSA_IN_I8 / _U8 / _C64)
  int fmt = 0;
  long long n_in = 0;
  long long n0 = 0;                // absolute index of in[0] (inputs delivered since the last reset)
  unsigned p0 = 0;                 // NCO phase at n0
  unsigned step = 0;               // NCO phase step per input
  const float2* nco = nullptr;     // [kDdcNcoTable] (cos, -sin) of 2 pi k / 4096, rounded from float64
  const float* taps = nullptr;     // [phases][D], zero beyond the T real taps
  int D = 2, n_taps = 1, phases = 8;
  const float2* hist = nullptr;    // mixed inputs [n0 - phases * D, n0) (zero before index 0)
  float2* hist_out = nullptr;      // ... the same window ending at n0 + n_in, written for the next call
  float2* out = nullptr;           // out[i] = y[m_first + i], i < n_out
  long long m_first = 0, n_out = 0;
};

// FIR (when n_out > 0) then the history update, in stream order
hipError_t launch_ddc(const DdcLaunch& a, hipStream_t s);

}  // namespace tdsa
