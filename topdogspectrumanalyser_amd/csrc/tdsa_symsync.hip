// tdsa_symsync.hip - symbol recovery for EVM: timing, resampling, carrier, derotation.
//
// symsync_kernel: one workgroup of 256 threads per segment, four stages separated by barriers.
//   1 timing    P = sum |x_j|^2, C = sum |x_j|^2 exp(-2 pi i (j nu mod 2^32) / 2^32)  (Oerder-Meyr), delta_fx from arg C
//   2 resample  y_k = cubic Lagrange at delta_fx + k step, k < K, kept in LDS (and stored to `raw`)
//   3 carrier   z = y^M, Z = DFT_G(z) in LDS (radix-2 decimation in frequency, a barrier per pass, bit-reversed out),
//               g* = lowest index of the largest |Z_g|^2, refined by the phase between the two halves of the derotated
//               z, then the phase of sum z_k exp(-2 pi i k M step_f / 2^32)
//   4 derotate  sym_k = y_k exp(-2 pi i (theta_fx + k step_f) / 2^32)
// The segment is read from HBM twice (stage 1, stage 2); everything after lives in LDS: y[K], Z[G], 4 KiB of scratch.
//
// Every sum is one fixed tree per (seg_len, K): thread t folds its elements t, t + 256, ... in order, then the 256
// partial sums fold pairwise, (t, t + 128), (t, t + 64), ...  So a segment's results depend on its samples alone, not on
// n_seg or on which segment it is.  The arithmetic is tdsa_symsync_math.hpp's.
#include <hip/hip_runtime.h>

#include "tdsa_seg_block.hpp"
#include "tdsa_symsync.hpp"
#include "tdsa_symsync_math.hpp"

// every rounding below is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kT = kSegThreads;

__device__ inline float2 cmul(float2 a, float2 b) {
  float2 r;
  sym_cmul(a.x, a.y, b.x, b.y, &r.x, &r.y);
  return r;
}

__device__ inline float2 power(float2 y, int order) {
  float2 z;
  sym_pow(y.x, y.y, order, &z.x, &z.y);
  return z;
}

__global__ __launch_bounds__(kT) void symsync_kernel(SymLaunch a) {
  extern __shared__ float2 lds[];   // y[K], then Z[G]
  __shared__ float4 red[kT];
  const int tid = threadIdx.x;
  const int K = a.K;
  const long long seg = blockIdx.x;
  const float2* x = a.in + seg * a.hop;
  float2* sym = a.sym + seg * a.out_stride;
  float2* raw = a.raw ? a.raw + seg * a.out_stride : nullptr;
  float2* y = lds;
  float2* Z = lds + K;

  // ---- 1: timing
  float pw = 0.0f, cr = 0.0f, ci = 0.0f;
  for (long long j = tid; j < a.seg_len; j += kT) {
    const float2 v = x[j];
    const float p = fmaf(v.x, v.x, v.y * v.y);
    const float2 w = rot(a.nco, uint32_t(j) * a.nu);
    pw = pw + p;
    cr = fmaf(p, w.x, cr);
    ci = fmaf(p, w.y, ci);
  }
  const float4 s1 = block_sum4(make_float4(pw, cr, ci, 0.0f), red, tid);
  const float P = s1.x, Cr = s1.y, Ci = s1.z;
  SymRecord rec = {};
  if (!(isfinite(P) && isfinite(Cr) && isfinite(Ci))) {   // the same for every thread
    const float qnan = __int_as_float(0x7fc00000);
    for (int k = tid; k < K; k += kT) {
      sym[k] = make_float2(qnan, qnan);
      if (raw) raw[k] = make_float2(qnan, qnan);
    }
    rec.flags = kSymFlagNonFinite;
    if (tid == 0) a.rec[seg] = rec;
    return;
  }
  const uint64_t delta = a.fixed ? a.delta_fx : sym_delta(Cr, Ci, a.step);
  rec.delta_fx = delta;
  rec.c_re = Cr;
  rec.c_im = Ci;
  rec.p = P;

  // ---- 2: resample.  delta >= 2^32 and K's definition keep x[i - 1 .. i + 2] inside the segment.
  for (int k = tid; k < K; k += kT) {
    const uint64_t pos = delta + uint64_t(k) * a.step;
    const long long i = sym_index(pos);
    float c[4];
    sym_coeffs(sym_mu(pos), c);
    const float2 x0 = x[i - 1], x1 = x[i], x2 = x[i + 1], x3 = x[i + 2];
    const float2 v = make_float2(sym_interp(c, x0.x, x1.x, x2.x, x3.x), sym_interp(c, x0.y, x1.y, x2.y, x3.y));
    y[k] = v;
    if (raw) raw[k] = v;
    if (a.order == 0) sym[k] = v;
  }
  if (a.order == 0) {
    if (tid == 0) a.rec[seg] = rec;
    return;
  }

  // ---- 3: carrier.  Z = DFT_G of z = y^M, zero padded
  const int M = a.order, log2G = a.log2G, G = 1 << log2G;
  __syncthreads();
  for (int e = tid; e < G; e += kT) Z[e] = e < K ? power(y[e], M) : make_float2(0.0f, 0.0f);
  for (int lh = log2G - 1; lh >= 0; --lh) {
    __syncthreads();
    const int h = 1 << lh;
    for (int b = tid; b < G / 2; b += kT) {
      const int k = b & (h - 1);
      const int e0 = ((b >> lh) << (lh + 1)) + k;
      const float2 x0 = Z[e0], x1 = Z[e0 + h];
      const float2 w = rot(a.nco, uint32_t(k) << (31 - lh));   // exp(-2 pi i k / (2 h))
      Z[e0] = make_float2(x0.x + x1.x, x0.y + x1.y);
      Z[e0 + h] = cmul(make_float2(x0.x - x1.x, x0.y - x1.y), w);
    }
  }
  __syncthreads();
  float best = -1.0f, tot = 0.0f;
  int bi = 0;
  for (int e = tid; e < G; e += kT) {
    const float2 v = Z[e];
    const float m = fmaf(v.x, v.x, v.y * v.y);
    const int g = int(__brev(unsigned(e)) >> (32 - log2G));
    tot = tot + m;
    if (m > best || (m == best && g < bi)) {
      best = m;
      bi = g;
    }
  }
  const float4 am = block_argmax_sum(best, bi, tot, red, tid);
  uint32_t step_f = 0, theta = 0;
  if (isfinite(am.z)) {
    const int gs = __float_as_int(am.y);
    rec.g = gs;
    rec.peak = am.x;
    rec.mean = am.z * (1.0f / float(G));
    // the two halves of z exp(-2 pi i (k g* mod G) / G)
    const int H = K / 2;
    float2 h1 = make_float2(0.0f, 0.0f), h2 = h1;
    for (int k = tid; k < 2 * H; k += kT) {
      const float2 w = rot(a.nco, uint32_t(k * gs) << (32 - log2G));
      const float2 v = cmul(power(y[k], M), w);
      if (k < H) h1 = make_float2(h1.x + v.x, h1.y + v.y);
      else h2 = make_float2(h2.x + v.x, h2.y + v.y);
    }
    const float4 s = block_sum4(make_float4(h1.x, h1.y, h2.x, h2.y), red, tid);
    const float dre = fmaf(s.z, s.x, s.w * s.y), dim = fmaf(s.w, s.x, -(s.z * s.y));   // S2 conj S1
    const float d = demod_atan2_over_pi(dim, dre);
    const int log2M = M == 2 ? 1 : M == 4 ? 2 : 3;
    step_f = sym_step_f(gs < G / 2 ? gs : gs - G, log2G + log2M, d, H, M);
    // the phase that is left
    const uint32_t zstep = uint32_t(M) * step_f;
    float2 ph = make_float2(0.0f, 0.0f);
    for (int k = tid; k < K; k += kT) {
      const float2 v = cmul(power(y[k], M), rot(a.nco, uint32_t(k) * zstep));
      ph = make_float2(ph.x + v.x, ph.y + v.y);
    }
    const float4 t = block_sum4(make_float4(ph.x, ph.y, 0.0f, 0.0f), red, tid);
    theta = sym_theta(demod_atan2_over_pi(t.y, t.x), a.ref, M);
  } else {
    rec.flags = kSymFlagCarrier;
  }
  rec.step_f = step_f;
  rec.theta_fx = theta;

  // ---- 4: derotate
  for (int k = tid; k < K; k += kT) sym[k] = cmul(y[k], rot(a.nco, theta + uint32_t(k) * step_f));
  if (tid == 0) a.rec[seg] = rec;
}

}  // namespace

// once per device, at create: the opt-in a runtime wants for more than 48 KiB of dynamic LDS, sized for the largest K
hipError_t symsync_prepare() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&symsync_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             kSymMaxLdsBytes - kSymStaticLdsBytes);
}

hipError_t launch_symsync(const SymLaunch& a, hipStream_t s) {
  if (a.n_seg < 1) return hipSuccess;
  const size_t lds = (size_t(a.K) + (a.order ? size_t(1) << a.log2G : 0)) * sizeof(float2);
  if (lds + kSymStaticLdsBytes > size_t(kSymMaxLdsBytes)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(symsync_kernel, dim3(unsigned(a.n_seg)), dim3(kT), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
