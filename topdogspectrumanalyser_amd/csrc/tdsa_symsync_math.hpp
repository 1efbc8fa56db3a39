// tdsa_symsync_math.hpp - the arithmetic of the symbol recovery, in plain C++ that the device
// kernel (tdsa_symsync.hip) and a host program (tests/symsync_math_host.cpp) compile alike: only +, -, x and fmaf, every
// rounding written out, so the accuracy measured on the host is the device's.
#pragma once
#include <cmath>
#include <cstdint>

#include "tdsa_demod_math.hpp"   // TDSA_HD, demod_atan2_over_pi

// no fused operation the text does not show
#pragma clang fp contract(off)

namespace tdsa {

// The interpolator's position in 32.32 fixed point: the sample index and mu, the top 24 bits of the fraction (exact).
TDSA_HD inline long long sym_index(uint64_t pos) { return (long long)(pos >> 32); }
TDSA_HD inline float sym_mu(uint64_t pos) { return float(uint32_t(pos & 0xffffffffu) >> 8) * 0x1p-24f; }

// Cubic Lagrange coefficients over the nodes -1, 0, 1, 2 at 0 <= mu < 1.  mu - 1 is exact; mu + 1 and mu - 2 round
// once.  mu = 0 gives exactly (0, 1, 0, 0).
TDSA_HD inline void sym_coeffs(float mu, float c[4]) {
  const float m1 = mu - 1.0f, m2 = mu - 2.0f, p1 = mu + 1.0f;
  c[0] = ((mu * m1) * m2) * -0.16666667f;
  c[1] = ((p1 * m1) * m2) * 0.5f;
  c[2] = ((p1 * mu) * m2) * -0.5f;
  c[3] = ((p1 * mu) * m1) * 0.16666667f;
}

// c0 x0 + c1 x1 + c2 x2 + c3 x3 of one part (re or im): one product, then three fused steps, in tap order
TDSA_HD inline float sym_interp(const float c[4], float x0, float x1, float x2, float x3) {
  float t = c[0] * x0;
  t = fmaf(c[1], x1, t);
  t = fmaf(c[2], x2, t);
  return fmaf(c[3], x3, t);
}

// (ar + j ai)(br + j bi)
TDSA_HD inline void sym_cmul(float ar, float ai, float br, float bi, float* re, float* im) {
  *re = fmaf(ar, br, -(ai * bi));
  *im = fmaf(ar, bi, ai * br);
}

// y^M, M = 2, 4 or 8, by repeated squaring: (r^2 - i^2, (r + r) i).  Exact for y = 2^e j^q.
TDSA_HD inline void sym_pow(float yr, float yi, int order, float* zr, float* zi) {
  for (int m = 1; m < order; m += m) {
    const float r = fmaf(yr, yr, -(yi * yi));
    yi = (yr + yr) * yi;
    yr = r;
  }
  *zr = yr;
  *zi = yi;
}

// exp(-2 pi j p / 2^32) the way the down-converter's NCO forms it (tdsa_ddc.hip): (hx, hy) = the table's entry for the
// top 12 bits, p >> 20, that is (cos, -sin) of 2 pi (p >> 20) / 4096; the low 20 bits (an angle below 1.6e-3) by their
// series.  With the low bits zero the table value comes back as it is.
TDSA_HD inline void sym_rot(uint32_t p, float hx, float hy, float* rr, float* ri) {
  const float t = float(p & 0xFFFFFu) * 1.46291807926715968e-9f;   // 2 pi / 2^32
  const float t2 = t * t;
  const float sl = fmaf(t * t2, 0.16666667f, -t);   // -sin t
  const float cm1 = t2 * -0.5f;                      // cos t - 1
  *rr = hx + fmaf(hx, cm1, -(hy * sl));
  *ri = hy + fmaf(hy, cm1, hx * sl);
}

// The clock phase of a spectral line C at the symbol rate, in symbols: a = arg C / pi, t = -a / 2 (+ 1 if negative),
// 0 <= t <= 1 ...
TDSA_HD inline float sym_clock_phase(float c_re, float c_im) {
  const float t = demod_atan2_over_pi(c_im, c_re) * -0.5f;
  return t < 0.0f ? t + 1.0f : t;
}
// ... and floor(t step) with t taken to 32 fractional bits: (tq * step) >> 32 without overflow, step = sh 2^32 + sl
TDSA_HD inline uint64_t sym_phase_to_samples(float t, uint64_t step) {
  const uint64_t tq = uint64_t(t * 0x1p32f);        // <= 2^32
  const uint64_t sh = step >> 32, sl = step & 0xffffffffu;
  return tq * sh + ((tq * sl) >> 32);
}

// Stage 1's end: the timing offset from the spectral line C of |x|^2, in 32.32 samples: floor(t step), + step below
// one sample: in [2^32, step + 2^32).
TDSA_HD inline uint64_t sym_delta(float c_re, float c_im, uint64_t step) {
  uint64_t d = sym_phase_to_samples(sym_clock_phase(c_re, c_im), step);
  if (d < (uint64_t(1) << 32)) d += step;
  return d;
}

// Stage 3's end.  step_f = round(f / M 2^32) mod 2^32 with f = g / G + d / (2 H) cycles per symbol of z: g the signed
// peak bin, G M a power of two (log2gm its exponent, <= 16), d = arg(S2 conj S1) / pi.
TDSA_HD inline uint32_t sym_step_f(int g_signed, int log2gm, float d, int H, int order) {
  const long long coarse = (long long)g_signed * (1ll << (32 - log2gm));
  const float fine = d / float(2 * H * order) * 0x1p32f;
  return uint32_t(uint64_t(coarse + (long long)rintf(fine)));
}
// theta_fx = round((a - ref) / (2 M) 2^32) mod 2^32, a and ref in half turns
TDSA_HD inline uint32_t sym_theta(float a, float ref, int order) {
  const float th = (a - ref) / float(2 * order) * 0x1p32f;
  return uint32_t(uint64_t((long long)rintf(th)));
}

}  // namespace tdsa
