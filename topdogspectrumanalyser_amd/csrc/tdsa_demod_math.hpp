// tdsa_demod_math.hpp - the discriminators of the analog demodulator, in plain C++ that the
// device kernels (tdsa_demod.hip) and a host program (tests/demod_math_host.cpp) compile alike: only +, -, x, fmaf and
// the correctly rounded / and sqrt, every rounding written out, so the accuracy measured on the host is the device's.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TDSA_HD __host__ __device__
#else
#define TDSA_HD
#endif

// no fused operation the text does not show
#pragma clang fp contract(off)

namespace tdsa {

// atan(t) / pi for 0 <= t <= 1, in half turns: t Q(t^2), Q of degree 8 fitted at Chebyshev nodes to atan(sqrt s) /
// (pi sqrt s) on [0, 1] (truncation 0.12 u, u = 2^-24 of a half turn; evaluated in float32 0.53 u).  Exactly 0 at t = 0.
TDSA_HD inline float demod_atan_over_pi(float t) {
  const float s = t * t;
  float q = 0x1.d8f74p-11f;
  q = fmaf(q, s, -0x1.4de086p-8f);
  q = fmaf(q, s, 0x1.bc3472p-7f);
  q = fmaf(q, s, -0x1.86e6d4p-6f);
  q = fmaf(q, s, 0x1.155d0ap-5f);
  q = fmaf(q, s, -0x1.72587p-5f);
  q = fmaf(q, s, 0x1.04a956p-4f);
  q = fmaf(q, s, -0x1.b2987ap-4f);
  q = fmaf(q, s, 0x1.45f306p-2f);
  return t * q;
}

// atan2(im, re) / pi in (-1, 1]: 0 at im = re = 0, +1 at im = +-0 and re < 0; the axes are exact (0, +-1/2, 1).
// Octant reduction: the smaller of |re|, |im| over the larger, the polynomial, then the reflections, all in half turns.
// NaN where either argument is NaN or both are infinite (what a non-finite sample makes of the product): a NaN among
// ax, ay leaves one in mx or mn, so the early return is 0 + 0 or NaN, and inf / inf is NaN.
TDSA_HD inline float demod_atan2_over_pi(float im, float re) {
  const float ax = fabsf(re), ay = fabsf(im);
  const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  if (!(mx > 0.0f)) return mx + mn;
  float r = demod_atan_over_pi(mn / mx);
  if (ay > ax) r = 0.5f - r;
  if (re < 0.0f) r = 1.0f - r;
  return im < 0.0f && r < 1.0f ? -r : r;   // a step that rounds to a whole half turn is +1, never -1
}

// FM: the phase step from y = x[n - 1] to x = x[n], arg(x conj y) / pi
TDSA_HD inline float demod_fm(float xr, float xi, float yr, float yi) {
  const float re = fmaf(xr, yr, xi * yi);
  const float im = fmaf(xi, yr, -(xr * yi));
  return demod_atan2_over_pi(im, re);
}

// AM: |x|
TDSA_HD inline float demod_am(float xr, float xi) { return sqrtf(fmaf(xr, xr, xi * xi)); }

}  // namespace tdsa
