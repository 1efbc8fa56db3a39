// modq_math_host.cpp - the modulation quality stage on the host: the functions of
// csrc/tdsa_modq_math.hpp, which the device kernel compiles too, driven through the stages in the kernel's order with the
// contract's summation tree written out for 256 threads in four waves.  The header is +, -, x and the correctly rounded
// / and sqrt only, so the records, indices and error vectors this program writes are the device's.
//
//   clang++ -O2 -std=c++17 -ffp-contract=off -I topdogspectrumanalyser_amd/csrc tests/modq_math_host.cpp -o modq_math_host
//   ./modq_math_host cases.bin results.bin
//
// cases.bin, back to back: int32 K, int32 T, T (re, im) float32 pairs, K (re, im) float32 pairs.
// results.bin, back to back: the 128-byte record, K uint8 indices, K (re, im) float32 error vectors.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tdsa_modq_math.hpp"

#pragma clang fp contract(off)

namespace {

using namespace tdsa;

// include/tdsa_hip.h: tdsa_modq_record
struct Record {
  float a_re, a_im, c_re, c_im;
  double s_y[2], s_yy, s_ry[2], s_cy[2];
  double err_sumsq, ref_sumsq, mag_sumsq, phase_sumsq;
  float err_peak;
  uint32_t err_peak_k, changed, flags;
  uint32_t reserved[2];
};
static_assert(sizeof(Record) == 128, "record layout");

constexpr int kThreads = 256;

// thread t folds elements t, t + 256, ... in order from 0.0; the 64 partial sums of a wave fold by the xor butterfly,
// own value first; the four wave sums as (W0 + W1) + (W2 + W3)
double tree_sum(const std::vector<double>& v) {
  double p[kThreads];
  for (int t = 0; t < kThreads; ++t) p[t] = 0.0;
  for (size_t k = 0; k < v.size(); ++k) p[k % kThreads] = p[k % kThreads] + v[k];
  for (int o = 32; o >= 1; o >>= 1) {
    double q[kThreads];
    for (int t = 0; t < kThreads; ++t) q[t] = p[t] + p[(t & ~63) | ((t & 63) ^ o)];
    std::memcpy(p, q, sizeof(p));
  }
  return (p[0] + p[64]) + (p[128] + p[192]);
}

bool analyse(int K, int T, const std::vector<ModqC32>& tab, const std::vector<ModqC32>& y, std::FILE* out) {
  std::vector<float> r_abs(T);
  double power = 0.0;
  for (int i = 0; i < T; ++i) {
    r_abs[i] = modq_abs32(tab[i]);
    power += modq_norm64(tab[i]);
  }
  const float inv_rho = float(1.0 / std::sqrt(power / double(T)));
  const auto at = [&](int i) { return tab[i]; };
  std::vector<double> v0(K), v1(K), v2(K), v3(K);
  for (int k = 0; k < K; ++k) v0[k] = double(y[k].re), v1[k] = double(y[k].im), v2[k] = modq_norm64(y[k]);
  const ModqC64 s_y{tree_sum(v0), tree_sum(v1)};
  const double s_yy = tree_sum(v2);
  ModqC32 a, c;
  unsigned flags = modq_first_guess(K, s_y, s_yy, inv_rho, &a, &c);
  Record rec = {};
  std::vector<uint8_t> idx(K, 0);
  std::vector<ModqC32> eps(K, ModqC32{NAN, NAN});
  if (!(flags & kModqFlagNonFinite)) {
    const bool decided = !(flags & kModqFlagDegenerate);
    ModqC64 s_ry{0.0, 0.0}, s_cy{0.0, 0.0};
    double s_rr = 0.0;
    unsigned changed = 0;
    for (int r = 0; decided && r < 2; ++r) {
      const ModqC32 q = modq_inverse(a);
      std::vector<int> counts(T, 0);
      for (int k = 0; k < K; ++k) {
        const int i = modq_decide(modq_normalise(y[k], c, q), at, T);
        if (r == 1 && idx[k] != uint8_t(i)) ++changed;
        idx[k] = uint8_t(i);
        ++counts[i];
        const ModqC64 ry = modq_conj_mul(tab[i], y[k]), cy = modq_plain_mul(tab[i], y[k]);
        v0[k] = ry.re, v1[k] = ry.im, v2[k] = cy.re, v3[k] = cy.im;
      }
      s_ry = ModqC64{tree_sum(v0), tree_sum(v1)};
      s_cy = ModqC64{tree_sum(v2), tree_sum(v3)};
      ModqC64 s_r;
      int n_max;
      modq_count_sums(at, [&](int i) { return counts[i]; }, T, &s_r, &s_rr, &n_max);
      if (!modq_fit(K, s_r, s_rr, n_max, s_y, s_ry, &a, &c)) flags |= kModqFlagOnePoint;
    }
    const ModqC32 q = modq_inverse(a);
    float best = 0.0f;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
      ModqErr er;
      if (decided) {
        er = modq_error(modq_normalise(y[k], c, q), tab[idx[k]], r_abs[idx[k]]);
      } else {
        er.eps = ModqC32{y[k].re - c.re, y[k].im - c.im};
        er.e2 = modq_norm32(er.eps);
        er.m = er.p = 0.0f;
      }
      eps[k] = er.eps;
      v0[k] = double(er.e2), v1[k] = double(er.m) * double(er.m), v2[k] = double(er.p) * double(er.p);
      if (er.e2 > best) best = er.e2, bk = k;
    }
    rec.a_re = a.re, rec.a_im = a.im, rec.c_re = c.re, rec.c_im = c.im;
    rec.s_y[0] = s_y.re, rec.s_y[1] = s_y.im, rec.s_yy = s_yy;
    rec.s_ry[0] = s_ry.re, rec.s_ry[1] = s_ry.im, rec.s_cy[0] = s_cy.re, rec.s_cy[1] = s_cy.im;
    rec.err_sumsq = tree_sum(v0), rec.ref_sumsq = s_rr, rec.mag_sumsq = tree_sum(v1), rec.phase_sumsq = tree_sum(v2);
    rec.err_peak = best, rec.err_peak_k = uint32_t(bk), rec.changed = changed;
  }
  rec.flags = flags;
  return std::fwrite(&rec, sizeof(rec), 1, out) == 1 && std::fwrite(idx.data(), 1, K, out) == size_t(K) &&
         std::fwrite(eps.data(), sizeof(ModqC32), K, out) == size_t(K);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  int n = 0;
  int32_t head[2];
  while (std::fread(head, sizeof(head), 1, in) == 1) {
    const int K = head[0], T = head[1];
    if (K < kModqMinSymbols || K > kModqMaxSymbols || T < 1 || T > kModqMaxPoints) {
      std::fprintf(stderr, "case %d: K = %d, T = %d\n", n, K, T);
      return 1;
    }
    std::vector<ModqC32> tab(T), y(K);
    if (std::fread(tab.data(), sizeof(ModqC32), T, in) != size_t(T) || std::fread(y.data(), sizeof(ModqC32), K, in) != size_t(K) ||
        !analyse(K, T, tab, y, out)) {
      std::fprintf(stderr, "case %d: short file\n", n);
      return 1;
    }
    ++n;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 1;
  std::printf("cases %d\n", n);
  return 0;
}
