// demod_math_host.cpp - the accuracy of the demodulator's discriminators (csrc/tdsa_demod_math.hpp), measured on the
// host against double: the header's arithmetic is +, -, x, fmaf and the correctly rounded / and sqrt only, so what this
// program measures is what the device computes.  Prints the worst |error| in u = 2^-24: "fm <A>" in half turns, the
// difference taken on the circle (a step next to +-pi may come out on the other side of the cut), "am <A>" in units
// of |x|; then the pinned special cases, "special ok" or the first one that fails; then the non-finite rule over every
// (x[n], x[n-1]) with parts from {NaN, +-inf, +-0, a few finite values}, "nonfinite ok <combinations>" or the first
// combination that breaks it: FM is NaN exactly when a part is not finite, AM is |x| as IEEE has it (inf, else NaN).
//
//   clang++ -O2 -std=c++17 -I topdogspectrumanalyser_amd/csrc tests/demod_math_host.cpp -o demod_math_host
#include <cmath>
#include <cstdio>

#include "tdsa_demod_math.hpp"

namespace {

const double kPi = 3.14159265358979323846;
const double kU = 1.0 / 16777216.0;

double fm_error(float xr, float xi, float yr, float yi) {
  const float got = tdsa::demod_fm(xr, xi, yr, yi);
  const double re = double(xr) * yr + double(xi) * yi, im = double(xi) * yr - double(xr) * yi;
  double want = std::atan2(im, re) / kPi;
  if (re == 0.0 && im == 0.0) want = 0.0;
  double e = std::fabs(double(got) - want);
  if (e > 1.0) e = 2.0 - e;
  return e / kU;
}

double am_error(float xr, float xi) {
  const double want = std::sqrt(double(xr) * xr + double(xi) * xi);
  return want > 0.0 ? std::fabs(double(tdsa::demod_am(xr, xi)) - want) / want / kU : 0.0;
}

}  // namespace

int main() {
  double worst_fm = 0.0, worst_am = 0.0;
  const int kPerOctant = 100000;
  const double near[] = {0.0, 1e-9, 1e-8, 1e-7, 3e-7, 1e-6, 1e-5, 1e-4, 1e-3};
  unsigned long long lcg = 12345;
  for (int oct = 0; oct < 8; ++oct) {
    for (int i = 0; i < kPerOctant + 2 * 9; ++i) {
      double th;                           // the phase step, in radians
      if (i < kPerOctant) th = (oct + (i + 0.5) / kPerOctant) * kPi / 4.0 - kPi;
      else {                               // next to the octant's lower edge: an axis, a diagonal or -pi
        const int j = i - kPerOctant;
        th = oct * kPi / 4.0 - kPi + (j < 9 ? near[j] : -near[j - 9]);
      }
      for (int mag = 0; mag <= 20; mag += 4) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        const double ph = double(lcg >> 11) / 9007199254740992.0 * 2.0 * kPi;      // where on the circle the pair sits
        const double ay = std::ldexp(1.0, -mag), ax = std::ldexp(1.0, -(20 - mag)) * (0.5 + 0.5 * double((lcg >> 3) & 1023) / 1023.0);
        const float yr = float(ay * std::cos(ph)), yi = float(ay * std::sin(ph));
        const float xr = float(ax * std::cos(ph + th)), xi = float(ax * std::sin(ph + th));
        const double e = fm_error(xr, xi, yr, yi);
        if (e > worst_fm) worst_fm = e;
        const double ea = am_error(xr, xi);
        if (ea > worst_am) worst_am = ea;
      }
    }
  }
  std::printf("fm %.2f\nam %.2f\n", worst_fm, worst_am);

  // quarter turns with exactly representable products: 0, +-1/2, 1, whatever the amplitudes
  const float amp[] = {0.125f, 1.0f, 8.0f, 3.0f};
  for (float a : amp)
    for (float b : amp) {
      const float jr[] = {1, 0, -1, 0}, ji[] = {0, 1, 0, -1};
      const float want[] = {0.0f, 0.5f, 1.0f, -0.5f};
      for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) {
          const float got = tdsa::demod_fm(a * jr[(p + q) % 4], a * ji[(p + q) % 4], b * jr[p], b * ji[p]);
          if (got != want[q]) {
            std::printf("special: quarter turn %d from %d at amplitudes %g, %g gave %.9g\n", q, p, a, b, got);
            return 1;
          }
        }
    }
  if (tdsa::demod_fm(0.5f, -0.25f, 0.0f, 0.0f) != 0.0f || tdsa::demod_fm(0.0f, 0.0f, 1.0f, 1.0f) != 0.0f) {
    std::printf("special: a zero product must give 0\n");
    return 1;
  }
  if (tdsa::demod_atan2_over_pi(-0.0f, -2.0f) != 1.0f || tdsa::demod_atan2_over_pi(0.0f, -2.0f) != 1.0f) {
    std::printf("special: Im = +-0, Re < 0 must give +1\n");
    return 1;
  }
  if (tdsa::demod_am(3.0f, 4.0f) != 5.0f || tdsa::demod_am(-5.0f, 12.0f) != 13.0f || tdsa::demod_am(0.0f, -7.0f) != 7.0f) {
    std::printf("special: exact envelopes\n");
    return 1;
  }
  std::printf("special ok\n");

  const float v[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1.0f, -0.5f, 0x1p-100f, -0x1p60f};
  const int nv = int(sizeof(v) / sizeof(v[0]));
  int bad_inputs = 0;
  for (int i = 0; i < nv * nv * nv * nv; ++i) {
    const float xr = v[i % nv], xi = v[i / nv % nv], yr = v[i / (nv * nv) % nv], yi = v[i / (nv * nv * nv)];
    const bool finite = std::isfinite(xr) && std::isfinite(xi) && std::isfinite(yr) && std::isfinite(yi);
    const float d = tdsa::demod_fm(xr, xi, yr, yi);
    if (finite ? !(d > -1.0f && d <= 1.0f) : !std::isnan(d)) {
      std::printf("nonfinite: fm(%g, %g | %g, %g) gave %.9g\n", xr, xi, yr, yi, d);
      return 1;
    }
    const float e = tdsa::demod_am(xr, xi);
    const bool inf = std::isinf(xr) || std::isinf(xi), nan = std::isnan(xr) || std::isnan(xi);
    if (inf && nan ? std::isfinite(e) : inf ? !(std::isinf(e) && e > 0.0f) : nan ? !std::isnan(e) : !std::isfinite(e)) {
      std::printf("nonfinite: am(%g, %g) gave %.9g\n", xr, xi, e);
      return 1;
    }
    bad_inputs += !finite;
  }
  std::printf("nonfinite ok %d\n", bad_inputs);
  return 0;
}
