// tdsa_demod.hip - analog demodulation of complex64 channel streams.
//
//   d[n] = arg(x[n] conj x[n-1]) / pi  (FM)   or   |x[n]|  (AM)          discriminator, at the input rate
//   a[m] = sum_{k < T} g[k] d[mR - k]                                     real FIR, decimation R
//   y[m] = c y[m-1] + (1 - c) a[m];  out = s a | s y | s (a - y)          one-pole section, scale last
//
// demod_audio_kernel<MODE>: grid (tiles, channels), one workgroup of 256 threads per tile of kDemodTile = 256
// consecutive outputs of one channel.  It stages the (256 - 1) R + Q R discriminator values the tile needs in LDS once
// (Q = ceil(T / R); every input sample is loaded and put through the discriminator once per tile; values older than the
// call come from the history).  Tap k = qR + r splits into a phase q and a residue r.  8 neighbouring lanes hold the
// residues r = 8g + lane, g = 0 .. ceil(R / 8) - 1, of the same 8 outputs, so a tap is shared by the 8 outputs of a
// lane and the residues of one output are summed across the 8 lanes at the end.  The staging is [g][row + row / 8][8]:
// row j holds d[(j_lo + j) R - r], and a lane slides over its column in register blocks of 8 taps x 8 outputs, two
// outputs per packed FMA.  A lane's reads of one instruction fall on 32 different banks at every R.
//
// Summation order of an output (what makes any split of the input give the same bits): per lane one fma chain over
// the residue groups in order and the phases q = 0 .. Q-1 in order, then a butterfly over the 8 lanes.  It depends on
// R and T alone, never on the tile, the call or the position of the output within either.
//
// demod_history_kernel: the last Q R discriminator values and the last raw sample of every channel for the next call
// (from this call's input and, for a short call, the previous history), into the other half of a ping-pong pair.
//
// demod_post_kernel: one workgroup per channel, in place over the a[] the audio kernel stored.  Blocks of
// kDemodPoleBlock = 64 outputs are aligned to the absolute output index; output k of a block is one fma chain
// sum_{j <= k} w[k - j] a[n_b + j] in ascending j, then one fma with c^(k+1) Y, Y the previous block's last output,
// carried serially by one thread.  A call that ends inside a block leaves that block's a[] and Y in device state, and
// the next call's outputs come out as if the block had arrived whole.  The same pass takes count, max, min, sum and
// sum of squares of the call's a[]: the float64 sums by one fixed tree per call, added once to the running totals.
#include <hip/hip_runtime.h>

#include "tdsa_demod.hpp"
#include "tdsa_demod_math.hpp"

// every rounding below is written out: the staging and the history kernel must give a sample the same bits
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kThreads = 256;
constexpr int kB = kDemodBlock;
constexpr int kPB = kDemodPoleBlock;

typedef float f2v __attribute__((ext_vector_type(2)));

// d[n0 + k] of channel ch, 0 <= k < n_in
template <int MODE>
__device__ inline float demod_disc(const DemodLaunch& a, int ch, long long k) {
  const float2* x = a.in + (long long)ch * a.in_stride;
  const float2 v = x[k];
  if (MODE == kDemodAM) return demod_am(v.x, v.y);
  const float2 p = k > 0 ? x[k - 1] : a.last[ch];
  return demod_fm(v.x, v.y, p.x, p.y);
}

// d[n] (absolute n): this call's input, the history before it, zero after it.  Without a branch: every load is made at
// a clamped, valid index and the value is selected afterwards, so the staging loop keeps several loads in flight
template <int MODE>
__device__ inline float demod_fetch(const DemodLaunch& a, int ch, int H, long long n) {
  const float2* x = a.in + (long long)ch * a.in_stride;
  const long long k = n - a.n0;
  const long long kc = k < 0 ? 0 : (k >= a.n_in ? a.n_in - 1 : k);
  const float2 v = x[kc];
  const float2 before = x[kc > 0 ? kc - 1 : 0];
  const float2 p = kc > 0 ? before : a.last[ch];
  const long long kh = k + H;                              // n - (n0 - H)
  const float h = a.hist[(long long)ch * a.hist_stride + (kh < 0 ? 0 : (kh >= H ? H - 1 : kh))];
  const float d = MODE == kDemodAM ? demod_am(v.x, v.y) : demod_fm(v.x, v.y, p.x, p.y);
  return k >= a.n_in ? 0.0f : (k >= 0 ? d : (kh >= 0 ? h : 0.0f));
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void demod_audio_kernel(DemodLaunch a) {
  extern __shared__ float stage[];    // [groups][demod_stage_rows(Q)][8]
  const int tid = threadIdx.x;
  const int ch = blockIdx.y;
  const int R = a.R;
  const int Q = (a.n_taps + R - 1) / R;
  const int groups = (R + kB - 1) / kB;
  const int rows = kDemodTile + Q - 1;
  const int PR = demod_stage_rows(Q);
  const long long m_a = a.m_first + (long long)blockIdx.x * kDemodTile;
  const long long jlo = m_a - Q + 1;

  // ---- stage d[(jlo + j) R - r], r < 8 groups (zero for r >= R): one discriminator per staged value
  const int RP = groups * kB;
#pragma unroll 4
  for (int e = tid; e < rows * RP; e += kThreads) {
    const int j = e / RP, r = e - j * RP;
    const float v = demod_fetch<MODE>(a, ch, Q * R, (jlo + j) * R - (r < R ? r : R - 1));
    stage[((r / kB) * PR + demod_prow(j)) * kB + (r % kB)] = r < R ? v : 0.0f;
  }
  __syncthreads();

  // ---- the FIR: lane rl of output group sg, outputs m_a + 8 sg + i; tap q of output i reads row 8 sg + i + Q - 1 - q
  const int rl = tid % kB;
  const int sg = tid / kB;
  const int base = sg * kB + Q - 1;
  f2v acc[kB / 2];
#pragma unroll
  for (int i = 0; i < kB / 2; ++i) acc[i] = f2v{0.f, 0.f};
  for (int g = 0; g < groups; ++g) {
    const int r = g * kB + rl;
    if (r >= R) continue;
    const float* col = stage + g * PR * kB + rl;
    for (int qb = 0; qb < Q; qb += kB) {
      float w[2 * kB - 1];
#pragma unroll
      for (int d = 0; d < 2 * kB - 1; ++d) {
        const int row = base - qb - (kB - 1) + d;    // negative only for taps beyond Q, which k < kc below leaves out
        w[d] = col[demod_prow(row < 0 ? 0 : row) * kB];
      }
      float t[kB];
#pragma unroll
      for (int k = 0; k < kB; ++k) t[k] = a.taps[(qb + k) * R + r];
      const int kc = Q - qb < kB ? Q - qb : kB;
#pragma unroll
      for (int k = 0; k < kB; ++k) {
        if (k < kc) {
          const f2v tk = f2v{t[k], t[k]};
#pragma unroll
          for (int i = 0; i < kB / 2; ++i)
            acc[i] = __builtin_elementwise_fma(tk, f2v{w[2 * i - k + kB - 1], w[2 * i - k + kB]}, acc[i]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kB / 2; ++i) {
#pragma unroll
    for (int o = kB / 2; o >= 1; o >>= 1) {
      const float ox = __shfl_xor(acc[i].x, o, 64);
      const float oy = __shfl_xor(acc[i].y, o, 64);
      acc[i].x = acc[i].x + ox;   // a + b on one lane, b + a on its partner: the same bits on both
      acc[i].y = acc[i].y + oy;
    }
  }
  // every lane of a group now holds all 8 sums: lane rl stores output rl, so a wave stores 64 consecutive floats
  float v = acc[0].x;
#pragma unroll
  for (int i = 1; i < kB; ++i) {
    const float c = (i & 1) ? acc[i / 2].y : acc[i / 2].x;
    v = rl == i ? c : v;
  }
  const long long m = m_a + tid;
  if (m < a.m_first + a.n_out) a.out[(long long)ch * a.out_stride + (m - a.m_first)] = v;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void demod_history_kernel(DemodLaunch a) {
  const int ch = blockIdx.y;
  const int Q = (a.n_taps + a.R - 1) / a.R;
  const long long H = (long long)Q * a.R;
  const float* hin = a.hist + (long long)ch * a.hist_stride;
  float* hout = a.hist_out + (long long)ch * a.hist_stride;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < H; k += (long long)gridDim.x * kThreads) {
    const long long n = a.n0 + a.n_in - H + k;
    hout[k] = n >= a.n0 ? demod_disc<MODE>(a, ch, n - a.n0) : hin[k + a.n_in];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.last_out[ch] = a.in[(long long)ch * a.in_stride + a.n_in - 1];
}

__global__ __launch_bounds__(kThreads) void demod_post_kernel(DemodLaunch a) {
  __shared__ float av[kThreads];        // a[] of a chunk of four blocks
  __shared__ float sv[kThreads];        // their block sums
  __shared__ float w[kPB], cp[kPB];
  __shared__ float yb[kThreads / kPB];  // Y at the start of each block of the chunk
  __shared__ double red_s[4], red_q[4];
  __shared__ float red_hi[4], red_lo[4];
  __shared__ long long red_n[4];
  const int tid = threadIdx.x;
  const int ch = blockIdx.x;
  const int k = tid % kPB, blk = tid / kPB;
  float* out = a.out + (long long)ch * a.out_stride;
  float* pend = a.pole_pend + (long long)ch * kPB;
  const bool pole = a.pole_mode != kDemodPoleOff;
  const long long m_end = a.m_first + a.n_out;
  const long long b0 = a.m_first - a.m_first % kPB;     // the block the call starts in
  const long long e0 = m_end - m_end % kPB;             // the block it ends in (nothing pending if e0 == m_end)
  if (tid < kPB) {
    w[tid] = a.pole_w[tid];
    cp[tid] = a.pole_cp[tid];
  }
  float Y = a.pole_y[ch];                               // thread 0's copy is the one that is carried
  long long cnt = 0;
  float hi = -INFINITY, lo = INFINITY;
  double sum = 0.0, sumsq = 0.0;
  // a[] of the chunk at cb for this thread: an output of this call, or - first chunk only - the part of the block an
  // earlier call left
  auto fetch = [&](long long cb) {
    const long long m = cb + tid;
    if (m >= a.m_first && m < m_end) return out[m - a.m_first];
    return m < a.m_first ? pend[m - b0] : 0.0f;
  };
  float next = fetch(b0);
  for (long long cb = b0; cb < m_end; cb += kThreads) {
    const long long m = cb + tid;
    const bool mine = m >= a.m_first && m < m_end;      // an output of this call
    const float x = next;
    if (cb + kThreads < m_end) next = fetch(cb + kThreads);   // in flight while this chunk is worked on
    __syncthreads();                                    // the previous chunk's reads of av / sv / yb are done
    av[tid] = x;
    if (mine) {
      ++cnt;
      hi = x > hi ? x : hi;
      lo = x < lo ? x : lo;
      sum += double(x);
      sumsq += double(x) * double(x);
    }
    __syncthreads();
    if (m >= e0 && m < m_end) pend[m - e0] = x;         // the block the call ends in, for the next call
    float r = x;
    if (pole) {
      float s = 0.0f;
      const float* ab = av + blk * kPB;
      for (int j = 0; j <= k; ++j) s = fmaf(w[k - j], ab[j], s);
      sv[tid] = s;
      __syncthreads();
      if (tid == 0) {
        for (int b = 0; b < kThreads / kPB; ++b) {
          yb[b] = Y;
          if (cb + (long long)(b + 1) * kPB <= m_end) Y = fmaf(cp[kPB - 1], Y, sv[b * kPB + kPB - 1]);
        }
      }
      __syncthreads();
      const float y = fmaf(cp[k], yb[blk], s);
      r = a.pole_mode == kDemodPoleLow ? y : x - y;
    }
    if (mine) out[m - a.m_first] = a.scale * r;
  }
  if (pole && tid == 0) a.pole_y[ch] = Y;

  // ---- the five reductions: a fixed tree over the lanes of a wave, then over the four waves
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    const float oh = __shfl_xor(hi, o, 64), ol = __shfl_xor(lo, o, 64);
    hi = oh > hi ? oh : hi;
    lo = ol < lo ? ol : lo;
    sum = sum + __shfl_xor(sum, o, 64);
    sumsq = sumsq + __shfl_xor(sumsq, o, 64);
  }
  if (k == 0) {
    red_n[blk] = cnt;
    red_hi[blk] = hi;
    red_lo[blk] = lo;
    red_s[blk] = sum;
    red_q[blk] = sumsq;
  }
  __syncthreads();
  if (tid == 0) {
    a.m_count[ch] += (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
    const float h4 = fmaxf(fmaxf(red_hi[0], red_hi[1]), fmaxf(red_hi[2], red_hi[3]));
    const float l4 = fminf(fminf(red_lo[0], red_lo[1]), fminf(red_lo[2], red_lo[3]));
    a.m_max[ch] = fmaxf(a.m_max[ch], h4);
    a.m_min[ch] = fminf(a.m_min[ch], l4);
    a.m_sum[ch] += (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    a.m_sumsq[ch] += (red_q[0] + red_q[1]) + (red_q[2] + red_q[3]);
  }
}

template <int MODE>
hipError_t audio_launch(const DemodLaunch& a, hipStream_t s) {
  const int Q = demod_phases(a.n_taps, a.R);
  const size_t lds = size_t(demod_lds_floats(a.R, Q)) * sizeof(float);
  if (lds > size_t(kDemodMaxLdsBytes)) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {   // a runtime that wants the opt-in gets it; whether the size is accepted is the launch's answer
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&demod_audio_kernel<MODE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    (void)hipGetLastError();
  }
  const long long tiles = (a.n_out + kDemodTile - 1) / kDemodTile;
  hipLaunchKernelGGL(demod_audio_kernel<MODE>, dim3(unsigned(tiles), unsigned(a.C)), dim3(kThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_demod(const DemodLaunch& a, hipStream_t s) {
  if (a.n_out > 0) {
    hipError_t e = a.mode == kDemodAM ? audio_launch<kDemodAM>(a, s) : audio_launch<kDemodFM>(a, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(demod_post_kernel, dim3(unsigned(a.C)), dim3(kThreads), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_in > 0) {
    const long long H = (long long)demod_phases(a.n_taps, a.R) * a.R;
    const unsigned grid = unsigned((H + kThreads - 1) / kThreads);
    if (a.mode == kDemodAM)
      hipLaunchKernelGGL(demod_history_kernel<kDemodAM>, dim3(grid, unsigned(a.C)), dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL(demod_history_kernel<kDemodFM>, dim3(grid, unsigned(a.C)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace tdsa
