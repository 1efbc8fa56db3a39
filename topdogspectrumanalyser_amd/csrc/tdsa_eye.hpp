// tdsa_eye.hpp - launcher of the eye diagrams (tdsa_eye.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_fsk.hpp"
#include "tdsa_seg.hpp"
#include "tdsa_symsync.hpp"

namespace tdsa {

constexpr int kEyeThreads = 256;
constexpr int kEyeMaxBins = 8192;                    // P H of one eye
constexpr int kEyeMinRows = 8;                       // H ...
constexpr int kEyeMaxRows = 256;
constexpr int kEyeMinPoints = 4;                     // P, a power of two ...
constexpr int kEyeMaxPoints = 64;
constexpr int kEyeMaxBoxcar = kFskMaxBoxcar;         // B
constexpr int kEyeMinSymbols = 3;                    // K: symbols 1 .. K - 2 are drawn
constexpr int kEyeTile = 1024;                       // samples of the series a work item holds in LDS
constexpr int kEyeTileD = kEyeTile + kEyeMaxBoxcar;  // ... and the d_j their boxcar needs (one spare)
constexpr int kEyeTotals = 10;                       // per eye {points, under, over, nan}, then {segments, skipped}
// the tile (complex64 for IQ; b and d for FM and REAL), the workgroup's ten totals
constexpr int kEyeStaticLdsBytes = (kEyeTile + kEyeTileD) * 4 + 64;
constexpr int kEyeMaxLdsBytes = 2 * kEyeMaxBins * 4 + kEyeStaticLdsBytes;   // two uint32 images beside them: 72.6 KiB of the CU's 160
// A workgroup's uint32 bins take at most kEyeItemsPerGroup work items of at most kEyeTile / 4 symbols of 64 points:
// below 2^31.  The launcher splits a call that brings more.
constexpr int kEyeMaxGroups = 2048;
constexpr long long kEyeItemsPerGroup = 1ll << 17;

constexpr int kEyeIq = 0, kEyeFm = 1, kEyeReal = 2;  // the kinds (include/tdsa_hip.h: TDSA_EYE_IQ, _FM, _REAL)

// one segment's clock (include/tdsa_hip.h: tdsa_eye_clock)
struct EyeClock {
  uint64_t delta_fx;
  uint32_t step_f, theta_fx;
};
static_assert(sizeof(EyeClock) == 16, "clock layout");

inline int eye_count(int kind) { return kind == kEyeIq ? 2 : 1; }
// n, the length of the series of a segment; may be <= 0
inline long long eye_series_len(uint64_t seg_len, int kind, int boxcar) {
  return kind == kEyeIq ? (long long)seg_len : fsk_boxcar_outputs(seg_len, kind == kEyeFm ? kFskIq : kFskFreq, boxcar);
}
// K, the producer's own: the symbol recovery's (IQ) or the FSK analysis'
inline long long eye_symbols_per_segment(uint64_t step, uint64_t seg_len, int kind, int boxcar) {
  if (kind == kEyeIq) return seg_len > (uint64_t(1) << 40) ? -1 : sym_symbols_per_segment(step, seg_len);
  return fsk_symbols_per_segment(step, seg_len, kind == kEyeFm ? kFskIq : kFskFreq, boxcar);
}
// the most symbols of a work item: their points' taps span at most kEyeTile - 1 samples of the series
inline int eye_symbols_per_item(uint64_t step) { return int((uint64_t(kEyeTile - 5) << 32) / step); }
// The symbols of a work item for a call of n_seg segments on `groups` workgroups: as many as give every workgroup an
// item (a one-segment tick spreads over the device), at least four points per thread - below that an item's barriers and
// a workgroup's merge cost more than its points -, at most what the tile holds; then
// evened out over the items of a segment.  The image does not depend on it.
inline int eye_plan_item(uint64_t step, int K, int log2p, long long n_seg, long long groups) {
  const long long most = eye_symbols_per_item(step), least = (4 * kEyeThreads) >> log2p;   // four points a thread
  long long spi = (n_seg * (K - 2) + groups - 1) / groups;
  spi = spi < least ? least : spi;
  spi = spi > most ? most : spi;
  const long long ips = (K - 2 + spi - 1) / spi;
  return int((K - 2 + ips - 1) / ips);
}
// workgroups per CU: what the LDS holds of them, four at most
inline int eye_groups_per_cu(size_t dynamic_lds) {
  const size_t fit = size_t(160 * 1024) / (dynamic_lds + size_t(kEyeStaticLdsBytes));
  return fit > 4 ? 4 : fit < 1 ? 1 : int(fit);
}

struct EyeLaunch {
  const void* in = nullptr;      // segment s = samples [s * hop, s * hop + seg_len): float2 (IQ, FM) or float (REAL)
  long long seg_len = 0, hop = 0;
  int n_seg = 0;
  int kind = kEyeIq;
  uint64_t step = 0;
  int boxcar = 1;
  int log2p = 5, rows = 128;     // P = 1 << log2p, H
  float lo = -1.0f, scale = 64.0f;
  int K = 0;
  const EyeClock* clocks = nullptr;   // [n_seg], device
  const float2* nco = nullptr;        // [kSegNcoTable] (cos, -sin) of 2 pi k / 4096
  void* traces = nullptr;             // [n_seg][K - 2][P] float (FM, REAL) or float2 (IQ), or null
  unsigned long long* counts = nullptr;   // [eyes][H][P]
  unsigned long long* totals = nullptr;   // [kEyeTotals]
  int num_cu = 256;
};

hipError_t eye_allow_lds();      // once per device, before the first launch: the opt-in for the dynamic LDS
hipError_t launch_eye(const EyeLaunch& a, hipStream_t s);

}  // namespace tdsa
