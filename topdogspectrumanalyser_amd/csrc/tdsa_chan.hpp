// tdsa_chan.hpp - launcher of the polyphase channelizer (tdsa_chan.hip): unpack, branch FIR,
// circular shift and M-point inverse DFT in one pass over raw IQ, every fs / M channel at once, with the filter history
// kept on the device between calls.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr int kChanMinChannels = 4;
constexpr int kChanMaxChannels = 256;
constexpr int kChanBlock = 8;                // output instants per thread, and taps per register block (taps padded to it)
constexpr int kChanMaxTapsPerBranch = 40;    // T <= 40 M: the default prototype has 34 taps per branch
constexpr int kChanTilePoints = 2048;        // a workgroup owns kChanTilePoints / M consecutive output instants
constexpr int kChanStaticLdsBytes = 2048;    // the uint8 table and the twiddles
constexpr int kChanMaxLdsBytes = 160 * 1024;

// taps per branch, P = ceil(T / M) ...
inline int chan_branch_taps(int n_taps, int M) { return (n_taps + M - 1) / M; }
// ... and rounded up to the register block: the padded tap table is [chan_tap_rows(T, M)][M]
inline int chan_tap_rows(int n_taps, int M) {
  return (chan_branch_taps(n_taps, M) + kChanBlock - 1) / kChanBlock * kChanBlock;
}

// staged samples of a tile live at s + (s / (8 D)) * pad: below 64 channels several thread groups share a wave, and
// the pad puts their windows on different banks
__host__ __device__ inline int chan_stage_pad(int M) { return M < 64 ? M : 0; }
// row stride of the transform tile [F][M + skew]: the channel-major store reads a column of it
__host__ __device__ inline int chan_row(int M) { return M + (M > 64 ? M / 64 : 1); }

// dynamic LDS of one workgroup, in complex samples: the staged inputs, later overlaid by the transform tile
inline int chan_lds_samples(int M, int os, int P) {
  const int D = M / os, F = kChanTilePoints / M;
  const int staged = (F + P * os - 1) * D;
  const int padded = staged + (staged / (kChanBlock * D)) * chan_stage_pad(M);
  const int tile = F * chan_row(M);
  return padded > tile ? padded : tile;
}

struct ChanLaunch {
  const void* in = nullptr;        // this call's raw input, n_in samples (TDSA_IN_I8 / _U8 / _C64)
  int fmt = 0;
  long long n_in = 0;
  long long n0 = 0;                // absolute index of in[0] (inputs delivered since the last reset)
  const float* taps = nullptr;     // [chan_tap_rows][M], tap q M + r at [q][r], zero beyond the T real taps
  const float2* tw = nullptr;      // [M / 2] exp(+2 pi j k / M), rounded from float64, exact at quarter turns
  int M = 4, log2M = 2, os = 1, P = 1;
  const float2* hist = nullptr;    // unpacked inputs [n0 - P M, n0) (zero before index 0)
  float2* hist_out = nullptr;      // ... the same window ending at n0 + n_in, written for the next call
  float2* out = nullptr;           // out[c * out_stride + i] = y_c[m_first + i], i < n_out
  long long out_stride = 0;
  long long m_first = 0, n_out = 0;
  int branches = 0;                // 1: store the shifted branch sums W_m[p] instead of y_c[m]
};

// the filter bank (when n_out > 0) then the history update, in stream order
hipError_t launch_chan(const ChanLaunch& a, hipStream_t s);

}  // namespace tdsa
