// tdsa_chan.hip - polyphase channelizer: every fs / M channel of a capture in one pass.
//
// y_c[m] = sum_{k < T} h[k] x[mD - k] exp(-2 pi j c (mD - k) / M), D = M / os, evaluated as
//   w_m[r] = sum_{q < P} h[qM + r] x[mD - qM - r]          branch sums, P = ceil(T / M)
//   W_m[p] = w_m[r] at p = (r - mD) mod M                   circular shift
//   y_c[m] = sum_p W_m[p] exp(+2 pi j c p / M)              unnormalised inverse DFT of M points
//
// chan_bank_kernel: one workgroup of 256 threads per tile of F = 2048 / M consecutive output instants.  It stages the
// unpacked inputs the tile needs in LDS once, (F - 1) D + P M samples in input order.  Thread (r, g) then holds branch
// r of the 8 instants 8g .. 8g + 7: it slides over its column of the staged samples in register blocks of 8 taps x 8
// instants (packed FMAs over (re, im)), so a staged sample is read once per block and a tap is shared by 8 instants.
// The shifted branch sums overlay the staging area as an [F][M] tile, F radix-2 decimation-in-frequency transforms run
// on it in place, and the tile is stored channel-major (channel c's F outputs are one run of 8 F bytes); the store
// reads the tile in bit-reversed channel order, so no reordering pass is needed.
//
// Summation order of an output (what makes any split of the input give the same bits): one fma chain over q = 0 .. P-1
// per branch, then the butterflies of the transform, whose order depends on M alone.  Neither depends on the tile, the
// call or the position of the output within either.
//
// chan_history_kernel: the last P M unpacked inputs for the next call (from this call's input and, for a short call,
// the previous history), into the other half of a ping-pong pair.
#include <hip/hip_runtime.h>

#include "tdsa_chan.hpp"
#include "tdsa_unpack.hpp"

// every rounding below is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kThreads = 256;
constexpr int kB = kChanBlock;

typedef float f2v __attribute__((ext_vector_type(2)));

// x[n0 + k]: fmt and in are read from the launch here, behind the callers' branches, not ahead of them
__device__ inline float2 chan_unpack(const ChanLaunch& a, long long k, const float* lut) {
  return unpack_iq(a.fmt, a.in, k, lut);
}

// input n (absolute): this call's input, the history before it, zero after it
__device__ inline float2 chan_fetch(const ChanLaunch& a, long long n, const float* lut) {
  if (n >= a.n0 + a.n_in) return make_float2(0.f, 0.f);
  if (n >= a.n0) return chan_unpack(a, n - a.n0, lut);
  const long long H = (long long)a.P * a.M;
  const long long k = n - (a.n0 - H);
  return k >= 0 ? a.hist[k] : make_float2(0.f, 0.f);
}

template <int OS>
__global__ __launch_bounds__(kThreads) void chan_bank_kernel(ChanLaunch a) {
  extern __shared__ float2 lds[];     // the staged inputs, then the transform tile [F][chan_row(M)]
  __shared__ float lut[256];
  __shared__ float2 tw[kChanMaxChannels / 2];
  constexpr int WIN = kB + (kB - 1) * OS;   // staged rows one register block slides over
  const int tid = threadIdx.x;
  const int M = a.M, D = M / OS, P = a.P;
  const int F = kChanTilePoints / M;
  const int log2blk = a.log2M + 3 - (OS - 1);   // log2(8 D)
  const int pad = chan_stage_pad(M);
  fill_lut(a.fmt, lut);
  if (tid < M / 2) tw[tid] = a.tw[tid];
  __syncthreads();

  // ---- stage x[n_lo .. n_lo + rows D): row j holds x[(j_lo + j) D - D + 1 .. (j_lo + j) D]
  const long long m_a = a.m_first + (long long)blockIdx.x * F;
  const int rows = F + P * OS - 1;
  const long long n_lo = (m_a - (long long)P * OS + 1) * D - D + 1;
  for (int s = tid; s < rows * D; s += kThreads) lds[s + (s >> log2blk) * pad] = chan_fetch(a, n_lo + s, lut);
  __syncthreads();

  // ---- branch sums: thread (r, g), instants i0 .. i0 + 7; x[(m_a + i) D - q M - r] is staged row
  //      i - q OS - rh + P OS - 1, column D - 1 - rc, with r = rh D + rc
  const int r = tid & (M - 1);
  const int i0 = (tid >> a.log2M) * kB;
  const int rh = OS == 2 && r >= D ? 1 : 0;
  const int col = D - 1 - (r - rh * D);
  const int row0 = i0 - rh + P * OS - 1;     // of instant i0, tap 0
  f2v acc[kB];
#pragma unroll
  for (int i = 0; i < kB; ++i) acc[i] = f2v{0.f, 0.f};
  for (int qb = 0; qb < P; qb += kB) {
    f2v w[WIN];
    const int rlo = row0 - OS * (qb + kB - 1);   // negative only for taps beyond P, which the k < kc below leaves out
#pragma unroll
    for (int d = 0; d < WIN; ++d) {
      const int rw = rlo + d < 0 ? 0 : rlo + d;
      const int s = rw * D + col;
      const float2 v = lds[s + (s >> log2blk) * pad];
      w[d] = f2v{v.x, v.y};
    }
    float t[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) t[k] = a.taps[(qb + k) * M + r];
    const int kc = P - qb < kB ? P - qb : kB;
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      if (k < kc) {
        const f2v tk = f2v{t[k], t[k]};
#pragma unroll
        for (int i = 0; i < kB; ++i) acc[i] = __builtin_elementwise_fma(tk, w[i + (kB - 1 - k) * OS], acc[i]);
      }
    }
  }
  __syncthreads();   // every window has been read: the tile may overlay the staging area

  // ---- circular shift: W_m[p] at p = (r - m D) mod M, which is r, or r + M / 2 at odd m when os = 2
  const int ROW = chan_row(M);
#pragma unroll
  for (int i = 0; i < kB; ++i) {
    const long long m = m_a + i0 + i;
    const int p = OS == 2 ? r ^ (int(m & 1) * (M >> 1)) : r;
    lds[(i0 + i) * ROW + p] = make_float2(acc[i].x, acc[i].y);
  }
  __syncthreads();

  // ---- F transforms of M points in place: decimation in frequency, natural order in, bit-reversed order out
  if (!a.branches) {
    const int log2h = a.log2M - 1;     // M / 2 butterflies per transform and stage
    for (int lh = log2h; lh >= 0; --lh) {
      const int h = 1 << lh;
#pragma unroll
      for (int u = 0; u < kChanTilePoints / 2 / kThreads; ++u) {
        const int b = tid + u * kThreads;
        const int inst = b >> log2h, j = b & ((1 << log2h) - 1);
        const int k = j & (h - 1);
        const int e0 = inst * ROW + ((j >> lh) << (lh + 1)) + k;
        const float2 x0 = lds[e0], x1 = lds[e0 + h];
        const float2 c = tw[k << (log2h - lh)];
        const float dr = x0.x - x1.x, di = x0.y - x1.y;
        lds[e0] = make_float2(x0.x + x1.x, x0.y + x1.y);
        lds[e0 + h] = make_float2(fmaf(dr, c.x, -(di * c.y)), fmaf(dr, c.y, di * c.x));
      }
      __syncthreads();
    }
  }

  // ---- channel-major store: F consecutive outputs per channel
  const int log2F = 11 - a.log2M;
  const long long left = a.m_first + a.n_out - m_a;   // instants of this tile the call completes
#pragma unroll
  for (int u = 0; u < kChanTilePoints / kThreads; ++u) {
    const int e = tid + u * kThreads;
    const int pos = e >> log2F, i = e & (F - 1);
    const int c = a.branches ? pos : int(__brev(unsigned(pos)) >> (32 - a.log2M));
    if (i < left) a.out[(long long)c * a.out_stride + (m_a - a.m_first) + i] = lds[i * ROW + pos];
  }
}

__global__ __launch_bounds__(kThreads) void chan_history_kernel(ChanLaunch a) {
  __shared__ float lut[256];
  fill_lut(a.fmt, lut);
  __syncthreads();
  const long long H = (long long)a.P * a.M;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < H; k += (long long)gridDim.x * kThreads) {
    const long long n = a.n0 + a.n_in - H + k;
    a.hist_out[k] = n >= a.n0 ? chan_unpack(a, n - a.n0, lut) : a.hist[k + a.n_in];
  }
}

template <int OS>
hipError_t bank_launch(const ChanLaunch& a, hipStream_t s) {
  const int F = kChanTilePoints / a.M;
  const size_t lds = size_t(chan_lds_samples(a.M, OS, a.P)) * sizeof(float2);
  if (lds + kChanStaticLdsBytes > size_t(kChanMaxLdsBytes)) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {   // a runtime that wants the opt-in gets it; whether the size is accepted is the launch's answer
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&chan_bank_kernel<OS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    (void)hipGetLastError();
  }
  const long long tiles = (a.n_out + F - 1) / F;
  hipLaunchKernelGGL(chan_bank_kernel<OS>, dim3(unsigned(tiles)), dim3(kThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_chan(const ChanLaunch& a, hipStream_t s) {
  if (a.n_out > 0) {
    const hipError_t e = a.os == 2 ? bank_launch<2>(a, s) : bank_launch<1>(a, s);
    if (e != hipSuccess) return e;
  }
  if (a.n_in > 0) {
    const long long H = (long long)a.P * a.M;
    long long grid = (H + kThreads - 1) / kThreads;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(chan_history_kernel, dim3(unsigned(grid)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace tdsa
