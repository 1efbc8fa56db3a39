// tdsa_ddc.hip - digital down-conversion for zoom spectra.
//
// y[m] = sum_{k < T} h[k] v[mD - k],  v[n] = x[n] exp(-2 pi j p[n] / 2^32),  p[n] = p0 + (n - n0) step (mod 2^32).
//
// ddc_fir_kernel: one workgroup per tile of MT consecutive outputs.  Tap k = qD + r splits into a phase q and a residue
// r; LANES neighbouring lanes of a wave hold LANES residues of the same MB = 8 outputs, so the residues of one output
// are summed across lanes at the end and a tap is shared by the MB outputs of a lane.  The residues go in groups of
// LANES: for each group the workgroup stages the mixed inputs v[jD - r] of all its outputs' phases in LDS (unpack, NCO
// and mixer once per staged sample), then every lane runs its outputs' phases in register blocks of 8 x 8 packed FMAs
// over a sliding window of 15 staged samples.  Inputs older than this call come from the mixed history.
//
// Summation order of an output (what makes any split of the input give the same bits): per lane, one fma chain over
// the residue groups in order and the phases q = 0 .. Q-1 in order; then a butterfly over the LANES lanes.  It depends
// on D and T alone, never on the tile, the call or the position of the output within either.
//
// ddc_history_kernel: the last phases * D mixed inputs for the next call (from this call's input and, for a short
// call, the previous history), into the other half of a ping-pong pair.
#include <hip/hip_runtime.h>

#include "tdsa_ddc.hpp"
#include "tdsa_unpack.hpp"

// every rounding below is written out: the FIR's staging and the history kernel must mix a sample to the same bits
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kThreads = 256;
constexpr int kMB = kDdcBlock;

typedef float f2v __attribute__((ext_vector_type(2)));

// x[n0 + k] exp(-2 pi j p / 2^32): the top 12 phase bits from the table, the low 20 (an angle below 1.6e-3) by their
// series, the product formed so that the table value takes only the final rounding
__device__ inline float2 ddc_mix(const DdcLaunch& a, long long k, const float* lut) {
  const float2 x = unpack_iq(a.fmt, a.in, k, lut);
  const float xr = x.x, xi = x.y;
  const unsigned p = a.p0 + unsigned(k) * a.step;
  const float2 h = a.nco[p >> 20];
  const float t = float(p & 0xFFFFFu) * 1.46291807926715968e-9f;   // 2 pi / 2^32
  const float t2 = t * t;
  const float sl = fmaf(t * t2, 0.16666667f, -t);   // -sin t
  const float cm1 = t2 * -0.5f;                      // cos t - 1
  const float rr = h.x + fmaf(h.x, cm1, -(h.y * sl));
  const float ri = h.y + fmaf(h.y, cm1, h.x * sl);
  return make_float2(fmaf(xr, rr, -(xi * ri)), fmaf(xr, ri, xi * rr));
}

// mixed input n (absolute): this call's input, the history before it, zero after it
__device__ inline float2 ddc_fetch(const DdcLaunch& a, long long n, const float* lut) {
  if (n >= a.n0 + a.n_in) return make_float2(0.f, 0.f);
  if (n >= a.n0) return ddc_mix(a, n - a.n0, lut);
  return a.hist[n - (a.n0 - (long long)a.phases * a.D)];
}

__host__ __device__ inline int prow(int jl) { return jl + jl / kMB; }   // a pad row every MB rows: subgroups on other banks

template <int LANES>
__global__ __launch_bounds__(kThreads) void ddc_fir_kernel(DdcLaunch a) {
  extern __shared__ float2 stage[];   // [prow(rows)][LANES]
  __shared__ float lut[256];
  constexpr int MT = (kThreads / LANES) * kMB;
  const int tid = threadIdx.x;
  fill_lut(a.fmt, lut);
  const int rl = tid % LANES;         // residue lane
  const int sg = tid / LANES;         // output group: outputs m_a + sg * MB + i
  const long long m_a = a.m_first + (long long)blockIdx.x * MT;
  const int Q = (a.n_taps + a.D - 1) / a.D;
  const int rows = MT + a.phases - 1;
  const long long jlo = m_a - a.phases + 1;
  const int ngroups = (a.D + LANES - 1) / LANES;
  const int base = sg * kMB + a.phases - 1;
  f2v acc[kMB];
#pragma unroll
  for (int i = 0; i < kMB; ++i) acc[i] = f2v{0.f, 0.f};
  for (int g = 0; g < ngroups; ++g) {
    __syncthreads();   // the table is filled / the previous group's reads are done
    for (int e = tid; e < rows * LANES; e += kThreads) {
      const int jl = e / LANES, c = e % LANES;
      const int r = g * LANES + c;
      float2 v = make_float2(0.f, 0.f);
      if (r < a.D) v = ddc_fetch(a, (jlo + jl) * a.D - r, lut);
      stage[prow(jl) * LANES + c] = v;
    }
    __syncthreads();
    const int r = g * LANES + rl;
    if (r >= a.D) continue;
    for (int qb = 0; qb < Q; qb += kMB) {
      f2v w[2 * kMB - 1];
#pragma unroll
      for (int d = 0; d < 2 * kMB - 1; ++d) {
        const float2 s = stage[prow(base - qb - (kMB - 1) + d) * LANES + rl];
        w[d] = f2v{s.x, s.y};
      }
      float t[kMB];
#pragma unroll
      for (int k = 0; k < kMB; ++k) t[k] = a.taps[(qb + k) * a.D + r];
      const int kc = Q - qb < kMB ? Q - qb : kMB;
#pragma unroll
      for (int k = 0; k < kMB; ++k) {
        if (k < kc) {
          const f2v tk = f2v{t[k], t[k]};
#pragma unroll
          for (int i = 0; i < kMB; ++i) acc[i] = __builtin_elementwise_fma(tk, w[i - k + kMB - 1], acc[i]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kMB; ++i) {
#pragma unroll
    for (int o = LANES / 2; o >= 1; o >>= 1) {
      const float ox = __shfl_xor(acc[i].x, o, 64);
      const float oy = __shfl_xor(acc[i].y, o, 64);
      acc[i].x = acc[i].x + ox;   // a + b on one lane, b + a on its partner: the same bits on both
      acc[i].y = acc[i].y + oy;
    }
  }
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < kMB; ++i) {
      const long long m = m_a + sg * kMB + i;
      if (m < a.m_first + a.n_out) a.out[m - a.m_first] = make_float2(acc[i].x, acc[i].y);
    }
  }
}

__global__ __launch_bounds__(kThreads) void ddc_history_kernel(DdcLaunch a) {
  __shared__ float lut[256];
  fill_lut(a.fmt, lut);
  __syncthreads();
  const long long H = (long long)a.phases * a.D;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < H; k += (long long)gridDim.x * kThreads) {
    const long long n = a.n0 + a.n_in - H + k;
    a.hist_out[k] = n >= a.n0 ? ddc_mix(a, n - a.n0, lut) : a.hist[k + a.n_in];
  }
}

template <int LANES>
hipError_t fir_launch(const DdcLaunch& a, hipStream_t s) {
  constexpr int MT = (kThreads / LANES) * kMB;
  const int rows = MT + a.phases - 1;
  const size_t lds = size_t(prow(rows - 1) + 1) * LANES * sizeof(float2);
  const long long tiles = (a.n_out + MT - 1) / MT;
  hipLaunchKernelGGL(ddc_fir_kernel<LANES>, dim3(unsigned(tiles)), dim3(kThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ddc(const DdcLaunch& a, hipStream_t s) {
  if (a.n_out > 0) {
    hipError_t e;
    if (a.D >= 64) e = fir_launch<64>(a, s);
    else if (a.D > 16) e = fir_launch<32>(a, s);
    else if (a.D > 8) e = fir_launch<16>(a, s);
    else if (a.D > 4) e = fir_launch<8>(a, s);
    else if (a.D > 2) e = fir_launch<4>(a, s);
    else e = fir_launch<2>(a, s);
    if (e != hipSuccess) return e;
  }
  if (a.n_in > 0) {
    const long long H = (long long)a.phases * a.D;
    long long grid = (H + kThreads - 1) / kThreads;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(ddc_history_kernel, dim3(unsigned(grid)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace tdsa
