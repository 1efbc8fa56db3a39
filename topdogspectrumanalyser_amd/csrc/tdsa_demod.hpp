// tdsa_demod.hpp - launcher of the analog demodulator (tdsa_demod.hip): FM / AM discriminator,
// real decimating FIR and one-pole section over C complex64 channel streams, with the filter history, the pole state
// and the measurements kept on the device between calls.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr int kDemodMaxChannels = 256;
constexpr int kDemodMaxDecimation = 64;
constexpr int kDemodMaxTapsPerPhase = 64;      // T <= 64 R
constexpr int kDemodBlock = 8;                 // outputs per thread, taps per register block and residue lanes per output
constexpr int kDemodTile = 256;                // consecutive outputs of one channel per workgroup: 32 groups x 8 outputs
constexpr int kDemodPoleBlock = 64;            // outputs per block of the one-pole section: one wave
constexpr int kDemodStaticLdsBytes = 4096;     // demod_post_kernel: a chunk, its sums, the pole tables and the reduction
constexpr int kDemodMaxLdsBytes = 160 * 1024;

constexpr int kDemodFM = 0, kDemodAM = 1;
constexpr int kDemodPoleOff = 0, kDemodPoleLow = 1, kDemodPoleHigh = 2;

// phases of the filter, Q = ceil(T / R): tap k = qR + r; the history holds the last Q R discriminator values
inline int demod_phases(int n_taps, int R) { return (n_taps + R - 1) / R; }
// ... rounded up to the register block: the padded tap table is [demod_tap_rows(T, R)][R]
inline int demod_tap_rows(int n_taps, int R) {
  return (demod_phases(n_taps, R) + kDemodBlock - 1) / kDemodBlock * kDemodBlock;
}
// staged row j of a tile sits at row j + j / 8: a pad row every 8 rows puts a wave's 8 output groups on other banks
__host__ __device__ inline int demod_prow(int j) { return j + j / kDemodBlock; }
// padded rows of one residue group of a tile's kDemodTile + Q - 1 staged rows; odd, so that the groups start on
// different banks
__host__ __device__ inline int demod_stage_rows(int Q) { return (demod_prow(kDemodTile + Q - 2) + 1) | 1; }
// dynamic LDS of one workgroup of the audio kernel, in floats: ceil(R / 8) residue groups of [demod_stage_rows(Q)][8]
inline int demod_lds_floats(int R, int Q) {
  return (R + kDemodBlock - 1) / kDemodBlock * demod_stage_rows(Q) * kDemodBlock;
}

struct DemodLaunch {
  int mode = kDemodFM;
  int C = 1, R = 1, n_taps = 1;
  const float2* in = nullptr;      // channel c's n_in samples of this call at in + c * in_stride
  long long in_stride = 0;
  long long n_in = 0;
  long long n0 = 0;                // absolute index of in[0] (inputs delivered since the last reset)
  const float* taps = nullptr;     // [demod_tap_rows][R], tap qR + r at [q][r], zero beyond the T real taps
  const float* hist = nullptr;     // per channel (stride hist_stride): d[n0 - Q R .. n0), zero before index 0
  float* hist_out = nullptr;       // ... the same window ending at n0 + n_in, written for the next call
  const float2* last = nullptr;    // [C] x[n0 - 1]
  float2* last_out = nullptr;      // [C] x[n0 + n_in - 1]
  long long hist_stride = 0;
  float* out = nullptr;            // out[c * out_stride + i]: a[m_first + i] after the audio kernel, the output after post
  long long out_stride = 0;
  long long m_first = 0, n_out = 0;
  // one-pole section and measurements (demod_post_kernel)
  int pole_mode = kDemodPoleOff;
  float scale = 1.0f;
  const float* pole_w = nullptr;   // [kDemodPoleBlock] (1 - c) c^i, rounded once from float64
  const float* pole_cp = nullptr;  // [kDemodPoleBlock] c^(i + 1)
  float* pole_y = nullptr;         // [C] the last output of the last complete block
  float* pole_pend = nullptr;      // [C][kDemodPoleBlock] a[] of the block the last call ended in
  long long* m_count = nullptr;    // [C] measurements over a[]
  float* m_max = nullptr;
  float* m_min = nullptr;
  double* m_sum = nullptr;
  double* m_sumsq = nullptr;
};

// the audio kernel and the post kernel (when n_out > 0), then the history update, in stream order
hipError_t launch_demod(const DemodLaunch& a, hipStream_t s);

}  // namespace tdsa
