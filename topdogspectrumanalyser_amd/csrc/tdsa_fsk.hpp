// tdsa_fsk.hpp - launcher of the FSK analysis (tdsa_fsk.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_seg.hpp"

namespace tdsa {

constexpr int kFskMaxBoxcar = 64;                    // B
constexpr int kFskMaxLag = 64;                       // L
constexpr int kFskTile = 1024;                       // stage 2: differences e_j per tile, a multiple of the workgroup
constexpr int kFskTileB = kFskTile + kFskMaxLag;     // ... the b_j they need ...
constexpr int kFskTileD = kFskTileB + kFskMaxBoxcar; // ... and the d_j those need (one spare)
// the two reductions' scratch (16 bytes a thread each), the tile's d and b, the segment's scalars
constexpr int kFskStaticLdsBytes = 2 * kSegThreads * 16 + (kFskTileB + kFskTileD) * 4 + 64;
constexpr int kFskMaxLdsBytes = kSegMaxSymbols * 4 + kFskStaticLdsBytes;   // v[K] beside them: under 34 KiB of the CU's 160

constexpr int kFskIq = 0, kFskFreq = 1;              // the input kinds (include/tdsa_hip.h: TDSA_FSK_IQ, _FREQ)
constexpr unsigned kFskFlagNonFinite = 1u;           // P, C or a v_k is not finite: NaN levels, zero indices, a zero record
constexpr unsigned kFskFlagOneLevel = 2u;            // a round of the fit found every symbol on one level: o, g kept

// one segment's record, as tdsa_fsk_process* hand it back (include/tdsa_hip.h: tdsa_fsk_record)
struct FskRecord {
  uint64_t delta_fx;
  float c_re, c_im, p;
  float offset, dev;
  float lo, hi;
  float err_peak;
  double err_sumsq;
  int32_t err_peak_k, sum_l;
  uint32_t flags, reserved;
};
static_assert(sizeof(FskRecord) == 64, "record layout");

// n_b, the boxcar's outputs of a segment: n_d - B + 1 with n_d = seg_len - 1 (IQ) or seg_len (FREQ); may be <= 0
inline long long fsk_boxcar_outputs(uint64_t seg_len, int kind, int boxcar) {
  return (long long)seg_len - (kind == kFskIq ? 1 : 0) - boxcar + 1;
}
// K = floor((n_b - 4) 2^32 / step) - 1, or a negative number where the segment is shorter than that
inline long long fsk_symbols_per_segment(uint64_t step, uint64_t seg_len, int kind, int boxcar) {
  if (seg_len > (uint64_t(1) << 40) || step == 0) return -1;
  const long long nb = fsk_boxcar_outputs(seg_len, kind, boxcar);
  if (nb < 4) return -1;
  return (long long)(((unsigned __int128)(nb - 4) << 32) / step) - 1;
}

struct FskLaunch {
  const void* in = nullptr;      // segment s = samples [s * hop, s * hop + seg_len): float2 (IQ) or float (FREQ)
  long long seg_len = 0, hop = 0;
  int n_seg = 0;
  int kind = kFskIq;
  uint64_t step = 0;             // samples per symbol, 32.32
  uint32_t nu = 0;               // the symbol clock's phase step per sample
  int levels = 2;                // M: 2, 4, 8
  int boxcar = 1, lag = 1;       // B, L
  int fixed = 0;                 // timing: 1 = delta_fx below instead of stage 2's
  uint64_t delta_fx = 0;
  int K = 0;
  const float2* nco = nullptr;   // [kSegNcoTable] (cos, -sin) of 2 pi k / 4096
  float* out = nullptr;          // [n_seg][out_stride] the levels v
  uint8_t* idx = nullptr;        // the same shape, the indices i of the second round, or null
  long long out_stride = 0;
  FskRecord* rec = nullptr;      // [n_seg]
};

hipError_t launch_fsk(const FskLaunch& a, hipStream_t s);

}  // namespace tdsa
