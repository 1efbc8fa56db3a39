// fsk_math_host.cpp - the accuracy of the FSK analysis' own arithmetic (csrc/tdsa_fsk_math.hpp), measured on the host
// against double and long double: the header is +, -, x, fmaf, floorf and the correctly rounded / only, so what this
// program measures is what the device computes.  Prints the worst errors in u = 2^-24:
//   t <A>      the clock phase t behind delta_fx against -atan2 / (2 pi) in double, in u of a symbol, on the circle:
//              every octant densely and the neighbourhoods of the axes; then delta_fx itself at every L = 1 .. 64 and
//              several steps against the contract's integer expression in 128-bit integers, from the same t, to the count
//   dec <A>    the decision's argument (v - o) / (g + g) + M / 2 against long double, in u of max(|t|, |t + M / 2|, 1),
//              next to every threshold from both sides, over seven decades of g and offsets up to 64 g
//   fit <A>    o and g of the fit against long double, in u of |o| + |g|: random levels with noise, sums in the same order
// then the pinned special cases, "special ok" or the first one that fails: B = 1 scales by exactly 1, the decision at a
// threshold itself, a NaN and the infinities, g = 0, hi = lo, D = 0, exact fits of lines on a binary grid.
//
//   clang++ -O2 -std=c++17 -I topdogspectrumanalyser_amd/csrc tests/fsk_math_host.cpp -o fsk_math_host
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tdsa_fsk_math.hpp"

namespace {

const double kPi = 3.14159265358979323846;
const double kU = 1.0 / 16777216.0;

// the contract's integer expression (tests/fsk_contract.py: delta_from_t)
uint64_t delta_ref(float t, uint64_t step, int lag) {
  const unsigned __int128 tq = (unsigned __int128)(uint64_t)std::floor(double(t) * 4294967296.0);
  unsigned __int128 d = (tq * step) >> 32;
  d = (d + ((unsigned __int128)lag << 31) + (step >> 1)) % step;
  if (d < ((unsigned __int128)1 << 32)) d += step;
  return uint64_t(d);
}

}  // namespace

int main() {
  unsigned long long lcg = 4321;
  auto next = [&]() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return lcg >> 11;
  };
  const uint64_t one = 1ull << 32;
  const uint64_t steps[] = {4 * one, uint64_t(4.37 * 4294967296.0), 8 * one - 4096, 8 * one, uint64_t(33.3 * 4294967296.0), 64 * one};

  // ---- t and delta_fx
  double worst_t = 0.0;
  {
    const double near[] = {0.0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2};
    const int kPer = 100000;
    for (int oct = 0; oct < 8; ++oct)
      for (int i = 0; i < kPer + 18; ++i) {
        const double th = i < kPer ? (oct + (i + 0.5) / kPer) * kPi / 4.0 - kPi
                                   : oct * kPi / 4.0 - kPi + (i - kPer < 9 ? near[i - kPer] : -near[i - kPer - 9]);
        const double a = std::ldexp(0.5 + double(next() & 1023) / 2046.0, int(next() % 41) - 20);
        const float re = float(a * std::cos(th)), im = float(a * std::sin(th));
        if (re == 0.0f && im == 0.0f) continue;
        float t = tdsa::demod_atan2_over_pi(im, re) * -0.5f;
        if (t < 0.0f) t = t + 1.0f;
        double want = -std::atan2(double(im), double(re)) / (2.0 * kPi);
        if (want < 0.0) want += 1.0;
        double e = std::fabs(double(t) - want);
        if (e > 0.5) e = 1.0 - e;
        if (e / kU > worst_t) worst_t = e / kU;
        const uint64_t step = steps[i % 6];
        const int lag = 1 + i % 64;
        const uint64_t d = tdsa::fsk_delta(re, im, step, lag);
        if (d != delta_ref(t, step, lag) || d < one || d >= step + one) {
          std::printf("special: delta_fx of C = (%a, %a), step %llu, L %d is %llu, the contract's %llu\n", re, im,
                      (unsigned long long)step, lag, (unsigned long long)d, (unsigned long long)delta_ref(t, step, lag));
          return 1;
        }
      }
    // every L at every step, t across its range and at its ends
    for (uint64_t step : steps)
      for (int lag = 1; lag <= 64; ++lag)
        for (int i = 0; i <= 4100; ++i) {
          const float t = i <= 4096 ? float(i) / 4096.0f : i == 4097 ? 0x1p-24f : i == 4098 ? 1.0f - 0x1p-24f : float(next() & 0xFFFFFF) * 0x1p-24f;
          const uint64_t d = tdsa::fsk_delta_from_t(t, step, lag);
          if (d != delta_ref(t, step, lag) || d < one || d >= step + one) {
            std::printf("special: delta_fx of t = %a, step %llu, L %d\n", t, (unsigned long long)step, lag);
            return 1;
          }
        }
  }
  std::printf("t %.2f\n", worst_t);

  // ---- the decision next to every threshold
  double worst_d = 0.0;
  for (int M = 2; M <= 8; M += M)
    for (int ge = -18; ge <= 2; ge += 3)
      for (int rep = 0; rep < 4000; ++rep) {
        const float g = float(std::ldexp(0.5 + double(next() & 0xFFFFFF) / 33554432.0, ge));
        const float o = float((double(next() % 129) - 64.0) * double(g) * (double(next() & 1023) / 1023.0));
        for (int j = 0; j <= M; ++j) {
          const double th = double(o) + double(g) * (2.0 * j - M);
          for (int side = -3; side <= 3; ++side) {
            float v = float(th);
            for (int s = 0; s < (side < 0 ? -side : side); ++s) v = std::nextafterf(v, side < 0 ? -INFINITY : INFINITY);
            if (side == 3) v = float(th + double(g) * (double(next() & 1023) / 512.0 - 1.0));   // anywhere in the cell
            const float q = (v - o) / (g + g) + float(M / 2);
            const long double want = ((long double)v - (long double)o) / (2.0L * (long double)g) + (long double)(M / 2);
            long double scale = std::fabs((double)(want - M / 2));
            if (std::fabs((double)want) > scale) scale = std::fabs((double)want);
            if (scale < 1.0L) scale = 1.0L;
            const double e = double(std::fabs((double)((long double)q - want)) / scale) / kU;
            if (e > worst_d) worst_d = e;
            const int i = tdsa::fsk_decide(v, o, g, M);
            const float fl = floorf(q);
            const int ref = fl >= float(M - 1) ? M - 1 : fl > 0.0f ? int(fl) : 0;
            if (i != ref || i < 0 || i > M - 1) {
              std::printf("special: decision of v = %a, o = %a, g = %a, M = %d is %d\n", v, o, g, M, i);
              return 1;
            }
          }
        }
      }
  std::printf("dec %.2f\n", worst_d);

  // ---- the fit
  double worst_f = 0.0;
  for (int M = 2; M <= 8; M += M)
    for (int rep = 0; rep < 3000; ++rep) {
      const int K = rep < 100 ? 2 + rep : 2 + int(next() % 4095);
      const double g = std::ldexp(0.5 + double(next() & 1023) / 2046.0, int(next() % 12) - 10);
      const double o = (double(next() % 2001) - 1000.0) / 1000.0 * 4.0 * g;
      long long sl = 0, sl2 = 0;
      double sv = 0.0, slv = 0.0;
      long double lv = 0.0L, llv = 0.0L;
      for (int k = 0; k < K; ++k) {
        const int l = 2 * int(next() % M) - (M - 1);
        const float v = float(o + g * l + g * 0.2 * (double(next() & 1023) / 512.0 - 1.0));
        sl += l;
        sl2 += l * l;
        sv = sv + double(v);
        slv = slv + double(l) * double(v);
        lv += (long double)v;
        llv += (long double)l * (long double)v;
      }
      float of = 0.0f, gf = 0.0f;
      const long long D = (long long)K * sl2 - sl * sl;
      const bool ok = tdsa::fsk_fit(K, sl, sl2, sv, slv, &of, &gf);
      if (ok != (D != 0)) {
        std::printf("special: fit with D = %lld says %d\n", D, int(ok));
        return 1;
      }
      if (!ok) continue;
      const long double gw = ((long double)K * llv - (long double)sl * lv) / (long double)D;
      const long double ow = (lv - gw * (long double)sl) / (long double)K;
      const double scale = std::fabs((double)ow) + std::fabs((double)gw);
      const double e = std::fmax(std::fabs(double((long double)gf - gw)), std::fabs(double((long double)of - ow))) / scale / kU;
      if (e > worst_f) worst_f = e;
    }
  std::printf("fit %.2f\n", worst_f);

  // ---- special cases
  if (tdsa::fsk_boxcar_scale(1) != 1.0f || tdsa::fsk_boxcar_scale(64) != 0x1p-6f || tdsa::fsk_level_scale(2) != 0.5f ||
      tdsa::fsk_level_scale(8) != float(1.0 / 14.0)) {
    std::printf("special: the scales\n");
    return 1;
  }
  for (int M = 2; M <= 8; M += M) {
    // on a binary grid: the threshold itself belongs to the cell above, a quarter cell below it to the one below, the ends clamp
    const float o = 0.375f, g = 0.0625f;
    for (int j = -2; j <= M + 2; ++j) {
      const float th = o + g * float(2 * j - M);
      const int up = j < 0 ? 0 : j > M - 1 ? M - 1 : j, down = j - 1 < 0 ? 0 : j - 1 > M - 1 ? M - 1 : j - 1;
      if (tdsa::fsk_decide(th, o, g, M) != up || tdsa::fsk_decide(th - 0.5f * g, o, g, M) != down) {
        std::printf("special: the decision at threshold %d of %d\n", j, M);
        return 1;
      }
    }
    if (tdsa::fsk_decide(NAN, o, g, M) != 0 || tdsa::fsk_decide(INFINITY, o, g, M) != M - 1 ||
        tdsa::fsk_decide(-INFINITY, o, g, M) != 0 || tdsa::fsk_decide(o, o, 0.0f, M) != 0 ||
        tdsa::fsk_decide(o + 1.0f, o, 0.0f, M) != M - 1 || tdsa::fsk_decide(o - 1.0f, o, 0.0f, M) != 0) {
      std::printf("special: the decision of a NaN, an infinity or at g = 0\n");
      return 1;
    }
    float o0, g0;
    tdsa::fsk_first_guess(-0.25f, 0.75f, M, &o0, &g0);
    if (o0 != 0.25f || g0 != 1.0f * tdsa::fsk_level_scale(M)) {
      std::printf("special: the first guess\n");
      return 1;
    }
    tdsa::fsk_first_guess(0.3f, 0.3f, M, &o0, &g0);
    if (o0 != 0.3f || g0 != 0.0f || tdsa::fsk_decide(0.3f, o0, g0, M) != 0) {
      std::printf("special: hi = lo\n");
      return 1;
    }
    // an exact line: v = o + l 2^-5 on every level, the sums exact in float64
    long long sl = 0, sl2 = 0;
    double sv = 0.0, slv = 0.0;
    const int K = 3 * M + 1;
    for (int k = 0; k < K; ++k) {
      const int l = tdsa::fsk_level(k % M, M);
      const float v = 0.375f + float(l) * 0x1p-5f;
      sl += l, sl2 += l * l, sv += double(v), slv += double(l) * double(v);
      if (tdsa::fsk_err(v, 0.375f, 0x1p-5f, l) != 0.0f) {
        std::printf("special: the error of a symbol on its level\n");
        return 1;
      }
    }
    float of = -1.0f, gf = -1.0f;
    if (!tdsa::fsk_fit(K, sl, sl2, sv, slv, &of, &gf) || of != 0.375f || gf != 0x1p-5f) {
      std::printf("special: the exact fit, M = %d: (%a, %a)\n", M, of, gf);
      return 1;
    }
    of = 7.0f, gf = 9.0f;
    if (tdsa::fsk_fit(5, 5 * (M - 1), 5 * (M - 1) * (M - 1), 1.0, 1.0, &of, &gf) || of != 7.0f || gf != 9.0f) {
      std::printf("special: D = 0 must leave o and g\n");
      return 1;
    }
  }
  // C = 0: t = 0, delta_fx = (L / 2 + sps / 2) mod sps, brought up
  if (tdsa::fsk_delta(0.0f, 0.0f, 4 * one, 2) != 3 * one || tdsa::fsk_delta(0.0f, 0.0f, 8 * one, 4) != 6 * one ||
      tdsa::fsk_delta(0.0f, 0.0f, 4 * one, 4) != 4 * one || tdsa::fsk_delta(0.0f, 0.0f, 4 * one, 1) != 2 * one + one / 2) {
    std::printf("special: delta_fx of C = 0\n");
    return 1;
  }
  std::printf("special ok\n");
  return 0;
}
