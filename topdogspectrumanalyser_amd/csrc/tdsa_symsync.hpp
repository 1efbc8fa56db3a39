// tdsa_symsync.hpp - launcher of the symbol recovery (tdsa_symsync.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_seg.hpp"

namespace tdsa {

constexpr int kSymMaxGrid = 2 * kSegMaxSymbols;      // G, the carrier transform's length
constexpr int kSymStaticLdsBytes = kSegThreads * 16 + 64;     // the reduction's scratch and the segment's scalars
constexpr int kSymMaxLdsBytes = (kSegMaxSymbols + kSymMaxGrid) * 8 + kSymStaticLdsBytes;   // ~100 KiB of the CU's 160

constexpr unsigned kSymFlagNonFinite = 1u;           // P or C is not finite: NaN symbols, a zero record
constexpr unsigned kSymFlagCarrier = 2u;             // the carrier transform's peak is not finite: step_f = theta_fx = 0

// one segment's record, as tdsa_symsync_process* hand it back (include/tdsa_hip.h: tdsa_symsync_record)
struct SymRecord {
  uint64_t delta_fx;
  float c_re, c_im, p;
  int32_t g;
  uint32_t step_f, theta_fx;
  float peak, mean;
  uint32_t flags, reserved;
};
static_assert(sizeof(SymRecord) == 48, "record layout");

// K = floor((seg_len - 4) 2^32 / step) - 1, or a negative number where the segment is shorter than that
inline long long sym_symbols_per_segment(uint64_t step, uint64_t seg_len) {
  if (seg_len < 4 || step == 0) return -1;
  return (long long)(((unsigned __int128)(seg_len - 4) << 32) / step) - 1;
}
inline int sym_log2_grid(int K) {   // G = 2 * 2^ceil(log2 K)
  int l = 0;
  while ((1 << l) < K) ++l;
  return l + 1;
}

struct SymLaunch {
  const float2* in = nullptr;    // segment s = samples [s * hop, s * hop + seg_len)
  long long seg_len = 0, hop = 0;
  int n_seg = 0;
  uint64_t step = 0;             // samples per symbol, 32.32
  uint32_t nu = 0;               // the symbol clock's phase step per sample
  int order = 0;                 // 0 (carrier off), 2, 4, 8
  float ref = 0.0f;              // arg of sum p^M over the reference points, in half turns
  int fixed = 0;                 // timing: 1 = delta_fx below instead of stage 1's
  uint64_t delta_fx = 0;
  int K = 0, log2G = 0;
  const float2* nco = nullptr;   // [kSegNcoTable] (cos, -sin) of 2 pi k / 4096
  float2* sym = nullptr;         // [n_seg][out_stride]
  float2* raw = nullptr;         // the same shape, the symbols before derotation, or null
  long long out_stride = 0;
  SymRecord* rec = nullptr;      // [n_seg]
};

hipError_t symsync_prepare();   // on the current device, before the first launch: the kernel's dynamic LDS limit
hipError_t launch_symsync(const SymLaunch& a, hipStream_t s);

}  // namespace tdsa
