// tdsa_fsk_math.hpp - the arithmetic of the FSK analysis that is its own, in plain C++ that the
// device kernel (tdsa_fsk.hip) and a host program (tests/fsk_math_host.cpp) compile alike; the discriminator is
// tdsa_demod_math.hpp's, the positions, the resampler and the rotation are tdsa_symsync_math.hpp's.  Only +, -, x, fmaf,
// floorf and the correctly rounded /, every rounding written out, so what is measured on the host is the device's.
#pragma once
#include <cmath>
#include <cstdint>

#include "tdsa_symsync_math.hpp"   // TDSA_HD, demod_atan2_over_pi, demod_fm, sym_*

// no fused operation the text does not show
#pragma clang fp contract(off)

namespace tdsa {

// float32(1 / B), the boxcar's scale, and float32(1 / (2 (M - 1))), the first guess of the level spacing: one correctly
// rounded division each; B = 1 gives exactly 1
TDSA_HD inline float fsk_boxcar_scale(int boxcar) { return 1.0f / float(boxcar); }
TDSA_HD inline float fsk_level_scale(int levels) { return 1.0f / float(2 * (levels - 1)); }

// Stage 2's end from t, the clock phase of the transitions in symbols, 0 <= t <= 1, taken to 32 fractional bits:
// floor(t step), then L / 2 samples on to where the transitions lie among the b_j, half a symbol on to the symbol
// centres, modulo step and into [2^32, step + 2^32).  All in integers.
TDSA_HD inline uint64_t fsk_delta_from_t(float t, uint64_t step, int lag) {
  uint64_t d = sym_phase_to_samples(t, step);
  d += (uint64_t(lag) << 31) + (step >> 1);
  d %= step;
  if (d < (uint64_t(1) << 32)) d += step;
  return d;
}
// ... from the spectral line C of e, as sym_delta takes its t
TDSA_HD inline uint64_t fsk_delta(float c_re, float c_im, uint64_t step, int lag) {
  return fsk_delta_from_t(sym_clock_phase(c_re, c_im), step, lag);
}

// Stage 4's first guess from the extremes: o = (hi + lo) / 2, g = (hi - lo) float32(1 / (2 (M - 1)))
TDSA_HD inline void fsk_first_guess(float lo, float hi, int levels, float* o, float* g) {
  *o = (hi + lo) * 0.5f;
  *g = (hi - lo) * fsk_level_scale(levels);
}

// The decision: i = clamp(floor((v - o) / (g + g) + M / 2), 0, M - 1), four float32 operations; a NaN (0 / 0 at g = 0
// among them) decides for 0, an infinity for its end.  The level is l = 2 i - (M - 1).
TDSA_HD inline int fsk_decide(float v, float o, float g, int levels) {
  const float q = floorf((v - o) / (g + g) + float(levels / 2));
  return q >= float(levels - 1) ? levels - 1 : q > 0.0f ? int(q) : 0;
}
TDSA_HD inline int fsk_level(int i, int levels) { return 2 * i - (levels - 1); }

// The least-squares line v = o + g l through K symbols from their sums: sum l and sum l^2 exact integers, sum v and
// sum l v in float64.  D = K sum l^2 - (sum l)^2 = 0 (every symbol on one level): false, o and g untouched.  Else five
// float64 operations for g, three more for o, each rounded once, and one rounding to float32 each.
TDSA_HD inline bool fsk_fit(int K, long long sum_l, long long sum_l2, double sum_v, double sum_lv, float* o, float* g) {
  const long long D = (long long)K * sum_l2 - sum_l * sum_l;
  if (D == 0) return false;
  const double num = double(K) * sum_lv - double(sum_l) * sum_v;
  const double g64 = num / double(D);
  const double o64 = (sum_v - g64 * double(sum_l)) / double(K);
  *g = float(g64);
  *o = float(o64);
  return true;
}

// Stage 5: what is left of a symbol beside its level
TDSA_HD inline float fsk_err(float v, float o, float g, int l) { return v - fmaf(g, float(l), o); }

}  // namespace tdsa
