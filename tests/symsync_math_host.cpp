// symsync_math_host.cpp - the accuracy of the symbol recovery's arithmetic (csrc/tdsa_symsync_math.hpp), measured on
// the host against double: the header's arithmetic is +, -, x and fmaf only, so what this program measures is what the
// device computes.  Prints the worst errors in u = 2^-24:
//   coef <A>                 a Lagrange coefficient relative to itself, over every mu = m 2^-24 the sweep visits
//   pow2 / pow4 / pow8 <A>   y^M relative to |y|^M: random points, then structured ones - |re| = |im|, phases next to
//                            every multiple of pi / 8, one part tiny, mantissas next to a power of two
//   rot <A>                  the rotation, absolute, with the table entry rounded from double as the library builds it:
//                            every table entry with its low bits at both ends and spread between, then random phases
//   atan <A>                 demod_atan2_over_pi in half turns, on the circle: every octant densely, the neighbourhoods
//                            of the axes and diagonals, |re| = |im|, amplitudes 2^-20 .. 2^20
// then the pinned special cases, "special ok" or the first one that fails: mu = 0 gives exactly (0, 1, 0, 0) and x[i],
// quarter turns and powers of 2^e j^q are exact, the fixed-point pieces (index, mu, delta_fx's range) are what the
// contract says.
//
//   clang++ -O2 -std=c++17 -I topdogspectrumanalyser_amd/csrc tests/symsync_math_host.cpp -o symsync_math_host
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>

#include "tdsa_symsync_math.hpp"

namespace {

const double kPi = 3.14159265358979323846;
const double kU = 1.0 / 16777216.0;

// the library's table entry for the top 12 phase bits (tdsa_capi_symsync.cpp)
void table(uint32_t p, float* hx, float* hy) {
  const int k = int(p >> 20), q = 1024;
  const double th = 2.0 * kPi * double(k % q) / 4096.0;
  const float c = k % q ? float(std::cos(th)) : 1.0f, s = k % q ? float(std::sin(th)) : 0.0f;
  const float cs[4] = {c, -s, -c, s}, sn[4] = {s, c, -s, -c};
  *hx = cs[k / q];
  *hy = -sn[k / q];
}

}  // namespace

int main() {
  unsigned long long lcg = 12345;
  auto next = [&]() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return lcg >> 11;
  };

  // ---- coefficients: a stride through every exponent of mu, and the neighbourhoods of 0 and 1
  double worst_c = 0.0;
  for (uint32_t m = 0; m < (1u << 24); m += (m < 4096 || m > (1u << 24) - 4096) ? 1 : 509) {
    const float mu = float(m) * 0x1p-24f;
    float c[4];
    tdsa::sym_coeffs(mu, c);
    const double t = double(mu);
    const double want[4] = {-t * (t - 1) * (t - 2) / 6, (t + 1) * (t - 1) * (t - 2) / 2, -(t + 1) * t * (t - 2) / 2,
                            (t + 1) * t * (t - 1) / 6};
    for (int i = 0; i < 4; ++i) {
      if (want[i] == 0.0) {
        if (c[i] != 0.0f) {
          std::printf("special: coefficient %d at mu = %a is %a, not 0\n", i, mu, c[i]);
          return 1;
        }
        continue;
      }
      const double e = std::fabs(double(c[i]) - want[i]) / std::fabs(want[i]) / kU;
      if (e > worst_c) worst_c = e;
    }
  }
  std::printf("coef %.2f\n", worst_c);

  // ---- powers
  for (int order = 2; order <= 8; order += order) {
    double worst = 0.0;
    for (int i = 0; i < 400000; ++i) {
      const double ph = double(next()) / 9007199254740992.0 * 2.0 * kPi, mag = std::ldexp(0.5 + double(next() & 1023) / 2046.0, int(next() % 9) - 4);
      const float yr = float(mag * std::cos(ph)), yi = float(mag * std::sin(ph));
      float zr, zi;
      tdsa::sym_pow(yr, yi, order, &zr, &zi);
      const std::complex<double> want = std::pow(std::complex<double>(yr, yi), order);
      const double e = std::abs(std::complex<double>(zr, zi) - want) / std::abs(want) / kU;
      if (e > worst) worst = e;
    }
    // structured: |re| = |im|, phases next to the multiples of pi / 8 (where a part of some power passes through zero),
    // one part tiny, mantissas just below and above a power of two
    const double eps[] = {0.0, 1e-9, 1e-7, 3e-6, 1e-4, 1e-3, 1e-2};
    const double mant[] = {1.0, 1.0 - 0x1p-24, 1.0 + 0x1p-23, 1.5, 1.999999, 1.25, 1.4142135623730951, 1.7320508075688772};
    for (int oct = 0; oct < 16; ++oct)
      for (double d : eps)
        for (int sg = -1; sg <= 1; sg += 2)
          for (double m1 : mant)
            for (double m2 : mant) {
              const double ph = oct * kPi / 8.0 + sg * d;
              float yr = float(m1 * std::cos(ph)), yi = float(m1 * std::sin(ph));
              if (d == 0.0 && oct % 4 == 2) yi = (yi < 0 ? -1.0f : 1.0f) * std::fabs(yr), yr *= float(m2 / m2);   // |re| = |im| exactly
              if (d == 0.0 && oct % 4 != 2) yi *= float(m2 * 0x1p-12);                                          // another ratio of the parts
              float zr, zi;
              tdsa::sym_pow(yr, yi, order, &zr, &zi);
              const std::complex<double> want = std::pow(std::complex<double>(yr, yi), order);
              if (std::abs(want) == 0.0) continue;
              const double e = std::abs(std::complex<double>(zr, zi) - want) / std::abs(want) / kU;
              if (e > worst) worst = e;
            }
    std::printf("pow%d %.2f\n", order, worst);
  }

  // ---- rotation
  double worst_r = 0.0;
  for (int i = 0; i < 2000000 + 4096 * 256; ++i) {
    const int j = i - 2000000;     // then every table entry with its low bits spread over their range
    const uint32_t p = i < 4096 ? uint32_t(i) << 20 : i < 8192 ? (uint32_t(i) << 20) | 0xFFFFFu
                       : j >= 0 ? (uint32_t(j >> 8) << 20) | uint32_t((j & 255) * 4111 + 17) : uint32_t(next());
    float hx, hy, rr, ri;
    table(p, &hx, &hy);
    tdsa::sym_rot(p, hx, hy, &rr, &ri);
    const double th = 2.0 * kPi * double(p) / 4294967296.0;
    const double e = std::hypot(double(rr) - std::cos(th), double(ri) + std::sin(th)) / kU;
    if (e > worst_r) worst_r = e;
  }
  std::printf("rot %.2f\n", worst_r);

  // ---- the arctangent, in half turns, the difference taken on the circle
  double worst_a = 0.0;
  {
    const double near[] = {0.0, 1e-9, 1e-8, 1e-7, 3e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2};
    const int kPer = 200000;
    for (int oct = 0; oct < 8; ++oct)
      for (int i = 0; i < kPer + 20; ++i) {
        const double th = i < kPer ? (oct + (i + 0.5) / kPer) * kPi / 4.0 - kPi
                                   : oct * kPi / 4.0 - kPi + (i - kPer < 10 ? near[i - kPer] : -near[i - kPer - 10]);
        for (int mag = -20; mag <= 20; mag += 10) {
          const double a = std::ldexp(0.5 + double(next() & 1023) / 2046.0, mag);
          const float re = float(a * std::cos(th)), im = float(a * std::sin(th));
          if (re == 0.0f && im == 0.0f) continue;
          double e = std::fabs(double(tdsa::demod_atan2_over_pi(im, re)) - std::atan2(double(im), double(re)) / kPi);
          if (e > 1.0) e = 2.0 - e;
          if (e / kU > worst_a) worst_a = e / kU;
        }
      }
    for (int i = 0; i < 100000; ++i) {     // |re| = |im| exactly, every sign
      const float a = float(std::ldexp(0.5 + double(next() & 0xFFFFFF) / 33554432.0, int(next() % 41) - 20));
      const float sr[] = {1, -1, -1, 1}, si[] = {1, 1, -1, -1};
      for (int q = 0; q < 4; ++q) {
        double e = std::fabs(double(tdsa::demod_atan2_over_pi(a * si[q], a * sr[q])) - std::atan2(double(a * si[q]), double(a * sr[q])) / kPi);
        if (e > 1.0) e = 2.0 - e;
        if (e / kU > worst_a) worst_a = e / kU;
      }
    }
  }
  std::printf("atan %.2f\n", worst_a);

  // ---- special cases
  {
    float c[4];
    tdsa::sym_coeffs(0.0f, c);
    if (!(c[0] == 0.0f && c[1] == 1.0f && c[2] == 0.0f && c[3] == 0.0f)) {
      std::printf("special: mu = 0 gives (%a, %a, %a, %a)\n", c[0], c[1], c[2], c[3]);
      return 1;
    }
    const float xs[] = {3.25f, -0x1p-30f, 0x1.fffffep20f, 0.0f};
    for (float x1 : xs)
      if (tdsa::sym_interp(c, 7.0f, x1, -9.0f, 0x1p40f) != x1) {
        std::printf("special: mu = 0 does not give x[i] = %a back\n", x1);
        return 1;
      }
  }
  for (int q = 0; q < 4; ++q) {
    float hx, hy, rr, ri;
    const uint32_t p = uint32_t(q) << 30;
    table(p, &hx, &hy);
    tdsa::sym_rot(p, hx, hy, &rr, &ri);
    const float wr[] = {1, 0, -1, 0}, wi[] = {0, -1, 0, 1};
    if (rr != wr[q] || ri != wi[q]) {
      std::printf("special: %d quarter turns give (%a, %a)\n", q, rr, ri);
      return 1;
    }
    for (int e = -3; e <= 3; ++e)
      for (int order = 2; order <= 8; order += order) {
        const float a = std::ldexp(1.0f, e), jr[] = {1, 0, -1, 0}, ji[] = {0, 1, 0, -1};
        float zr, zi;
        tdsa::sym_pow(a * jr[q], a * ji[q], order, &zr, &zi);
        const int qq = (q * order) % 4;
        if (zr != std::ldexp(1.0f, e * order) * jr[qq] || zi != std::ldexp(1.0f, e * order) * ji[qq]) {
          std::printf("special: (2^%d j^%d)^%d gave (%a, %a)\n", e, q, order, zr, zi);
          return 1;
        }
      }
  }
  if (tdsa::sym_index(0x0000000500000000ull | 0xffffffffu) != 5 || tdsa::sym_mu(0x5000001ffull) != 0x1p-24f ||
      tdsa::sym_mu(0x5ffffffffull) != 1.0f - 0x1p-24f) {
    std::printf("special: index / mu of a 32.32 position\n");
    return 1;
  }
  {
    const uint64_t one = 1ull << 32, steps[] = {4 * one, uint64_t(4.37 * 4294967296.0), 64 * one};
    for (uint64_t step : steps) {
      if (tdsa::sym_delta(0.0f, 0.0f, step) != step) {
        std::printf("special: C = 0 must give delta_fx = step\n");
        return 1;
      }
      for (int i = 0; i < 100000; ++i) {
        const double ph = double(next()) / 9007199254740992.0 * 2.0 * kPi;
        const uint64_t d = tdsa::sym_delta(float(std::cos(ph)), float(std::sin(ph)), step);
        if (d < one || d >= step + one) {
          std::printf("special: delta_fx = %llu outside [2^32, step + 2^32)\n", (unsigned long long)d);
          return 1;
        }
      }
      // the wrap: an argument just below and just above zero
      if (tdsa::sym_delta(1.0f, 0x1p-40f, step) != step || tdsa::sym_delta(1.0f, -0x1p-40f, step) != step) {
        std::printf("special: arg C = +-0 must give delta_fx = step\n");
        return 1;
      }
    }
  }
  if (tdsa::sym_step_f(-4, 4, 0.0f, 3, 2) != 0xC0000000u || tdsa::sym_step_f(1, 16, 0.0f, 5, 8) != 0x10000u ||
      tdsa::sym_theta(1.0f, 1.0f, 4) != 0u || tdsa::sym_theta(0.0f, 1.0f, 4) != 0xE0000000u) {
    std::printf("special: step_f / theta_fx\n");
    return 1;
  }
  std::printf("special ok\n");
  return 0;
}
