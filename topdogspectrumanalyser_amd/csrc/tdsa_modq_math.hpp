// tdsa_modq_math.hpp - the arithmetic of the modulation quality stage in plain C++ that the
// device kernel (tdsa_modq.hip) and a host program (tests/modq_math_host.cpp) compile alike: first guess, decision,
// least-squares fit and the errors of a symbol.  Only +, -, x and the correctly rounded / and sqrt in float32 and float64,
// every rounding written out and no fused operation, so what the host program prints is what the device computes; the
// arctangent of the phase error is tdsa_demod_math.hpp's.  A complex product is four products, one difference and one
// sum; a product of two float32 values is exact in float64.
#pragma once
#include <cmath>
#include <cstdint>

#include "tdsa_demod_math.hpp"   // TDSA_HD, demod_atan2_over_pi

// no fused operation at all
#pragma clang fp contract(off)

namespace tdsa {

constexpr int kModqMaxPoints = 64;                   // T
constexpr int kModqMinSymbols = 2;                   // K ...
constexpr int kModqMaxSymbols = 4096;
constexpr unsigned kModqFlagNonFinite = 1u;          // S_y or S_yy is not finite: zero indices, NaN errors, a zero record
constexpr unsigned kModqFlagDegenerate = 2u;         // the first guess of the gain is zero: no decisions
constexpr unsigned kModqFlagOnePoint = 4u;           // a round of the fit found every symbol on one point: a, c kept

struct ModqC32 {
  float re, im;
};
struct ModqC64 {
  double re, im;
};

// x y in float64: four products, one difference, one sum
TDSA_HD inline ModqC64 modq_mul(ModqC64 x, ModqC64 y) {
  return ModqC64{x.re * y.re - x.im * y.im, x.re * y.im + x.im * y.re};
}
// conj(r) y and r y of two float32 pairs in float64: the products are exact, each part rounds once
TDSA_HD inline ModqC64 modq_conj_mul(ModqC32 r, ModqC32 y) {
  return ModqC64{double(r.re) * double(y.re) + double(r.im) * double(y.im),
                 double(r.re) * double(y.im) - double(r.im) * double(y.re)};
}
TDSA_HD inline ModqC64 modq_plain_mul(ModqC32 r, ModqC32 y) {
  return ModqC64{double(r.re) * double(y.re) - double(r.im) * double(y.im),
                 double(r.re) * double(y.im) + double(r.im) * double(y.re)};
}
// re^2 + im^2 of a float32 pair in float64: one rounding
TDSA_HD inline double modq_norm64(ModqC32 y) { return double(y.re) * double(y.re) + double(y.im) * double(y.im); }
// ... in float32: three roundings
TDSA_HD inline float modq_norm32(ModqC32 y) {
  const float a = y.re * y.re, b = y.im * y.im;
  return a + b;
}
// what the host uploads beside the table
TDSA_HD inline float modq_abs32(ModqC32 r) { return sqrtf(modq_norm32(r)); }

// Stage 0 from the tree sums: c0 = float32(S_y / K) per part, a0 = (sqrtf(float32(max(v, 0))) inv_rho, 0) with
// v = S_yy / K - |S_y / K|^2.  Returns the flags: non-finite sums, or a0 = 0.
TDSA_HD inline unsigned modq_first_guess(int K, ModqC64 s_y, double s_yy, float inv_rho, ModqC32* a, ModqC32* c) {
  a->re = a->im = c->re = c->im = 0.0f;
  // x - x is zero for a finite x alone
  if (!(s_y.re - s_y.re == 0.0 && s_y.im - s_y.im == 0.0 && s_yy - s_yy == 0.0)) return kModqFlagNonFinite;
  const double k = double(K);
  const double mr = s_y.re / k, mi = s_y.im / k;
  c->re = float(mr);
  c->im = float(mi);
  const double v = s_yy / k - (mr * mr + mi * mi);
  const float vf = float(v > 0.0 ? v : 0.0);
  a->re = sqrtf(vf) * inv_rho;
  return a->re == 0.0f ? kModqFlagDegenerate : 0u;
}

// q = conj(a) / (a_re^2 + a_im^2) in float64, each part rounded to float32 once
TDSA_HD inline ModqC32 modq_inverse(ModqC32 a) {
  const double n = modq_norm64(a);
  return ModqC32{float(double(a.re) / n), float(-double(a.im) / n)};
}

// w = (y - c) q in float32: two differences, four products, one difference, one sum
TDSA_HD inline ModqC32 modq_normalise(ModqC32 y, ModqC32 c, ModqC32 q) {
  const float tr = y.re - c.re, ti = y.im - c.im;
  const float rr = tr * q.re, ii = ti * q.im, ri = tr * q.im, ir = ti * q.re;
  return ModqC32{rr - ii, ri + ir};
}

// Stage 1: the lowest index of the smallest d_i = fl(fl((w_re - r_re)^2) + fl((w_im - r_im)^2)) over the T points,
// compared with <; a NaN distance never wins, every distance NaN gives 0.  The table is read through `at`, an index
// to ModqC32, so that the kernel can hand in its LDS copy.
template <class Table>
TDSA_HD inline int modq_decide(ModqC32 w, const Table& at, int T) {
  int best = 0;
  float bd = NAN;                    // no distance taken yet
#pragma unroll 8
  for (int i = 0; i < T; ++i) {
    const ModqC32 r = at(i);
    const float dr = w.re - r.re, di = w.im - r.im;
    const float a = dr * dr, b = di * di;
    const float d = a + b;
    // the first distance that is not a NaN is taken as it is (an infinity too), later ones only when smaller; written
    // without a branch, so that the loads of several points go out together
    const bool take = (d < bd) | ((bd != bd) & (d == d));
    bd = take ? d : bd;
    best = take ? i : best;
  }
  return best;
}

// The count-derived sums of a round, in float64 and in index order: S_r = sum n_i r_i, S_rr = sum n_i |r_i|^2; also the
// largest count.
template <class Table, class Counts>
TDSA_HD inline void modq_count_sums(const Table& at, const Counts& n_of, int T, ModqC64* s_r, double* s_rr, int* n_max) {
  ModqC64 sr{0.0, 0.0};
  double srr = 0.0;
  int most = 0;
  for (int i = 0; i < T; ++i) {
    const ModqC32 r = at(i);
    const int n = n_of(i);
    const double nd = double(n);
    sr.re = sr.re + nd * double(r.re);
    sr.im = sr.im + nd * double(r.im);
    srr = srr + nd * modq_norm64(r);
    most = n > most ? n : most;
  }
  *s_r = sr;
  *s_rr = srr;
  *n_max = most;
}

// Stage 2: the least-squares y = a r + c through K symbols from the sums.  D = K S_rr - |S_r|^2; every symbol on one
// index, or D <= 0: false, a and c untouched.  Else a = (K S_ry - conj(S_r) S_y) / D and c = (S_y - a S_r) / K in float64
// (c from the unrounded a), each part rounded to float32 once.
TDSA_HD inline bool modq_fit(int K, ModqC64 s_r, double s_rr, int n_max, ModqC64 s_y, ModqC64 s_ry, ModqC32* a, ModqC32* c) {
  const double k = double(K);
  const double D = k * s_rr - (s_r.re * s_r.re + s_r.im * s_r.im);
  if (n_max >= K || !(D > 0.0)) return false;
  const ModqC64 x = modq_mul(ModqC64{s_r.re, -s_r.im}, s_y);
  const ModqC64 num{k * s_ry.re - x.re, k * s_ry.im - x.im};
  const ModqC64 a64{num.re / D, num.im / D};
  const ModqC64 ar = modq_mul(a64, s_r);
  a->re = float(a64.re);
  a->im = float(a64.im);
  c->re = float((s_y.re - ar.re) / k);
  c->im = float((s_y.im - ar.im) / k);
  return true;
}

// Stage 4 of one symbol against its point r (r_abs beside it): the error vector, its squared length, the magnitude
// error and the phase error in half turns (0 where r = 0)
struct ModqErr {
  ModqC32 eps;
  float e2, m, p;
};
TDSA_HD inline ModqErr modq_error(ModqC32 w, ModqC32 r, float r_abs) {
  ModqErr e;
  e.eps = ModqC32{w.re - r.re, w.im - r.im};
  e.e2 = modq_norm32(e.eps);
  e.m = sqrtf(modq_norm32(w)) - r_abs;
  // w conj(r): four products, one sum, one difference
  const float rr = w.re * r.re, ii = w.im * r.im, ir = w.im * r.re, ri = w.re * r.im;
  e.p = (r.re == 0.0f && r.im == 0.0f) ? 0.0f : demod_atan2_over_pi(ir - ri, rr + ii);
  return e;
}

}  // namespace tdsa
