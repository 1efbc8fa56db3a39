// tdsa_modq.hip - modulation quality: decisions, gain / phase / offset fit, error vector.
//
// modq_kernel: one workgroup of 256 threads per segment of K symbols, [n_seg][in_stride] complex64 as the symbol
// recovery leaves them.  Thread t owns symbols t, t + 256, ... (16 at most); it copies them into LDS on the one pass over
// HBM and reads only its own back in the passes that follow, so no barrier stands between a pass and its symbols.
//   0 first guess  S_y, S_yy; c0 the mean, a0 from the variance and the table's rms
//   1 decide       w = (y - c) q, the nearest of the T points by brute force, the lowest index on a tie
//   2 fit          counts per point in an LDS histogram (integers, order-free), S_ry and S_cy, the least-squares a and c
//   3 two rounds   of 1 and 2; `changed` counts the symbols whose index moved
//   4 errors       against the second round's decisions with the final a and c
// The table, r_abs and the counts sit in LDS; the steps that the contract gives to one thread (first guess, q, fit) are
// computed by every thread from the same LDS words - the same bits, and no barrier to hand them round.
//
// Every float64 sum is one fixed tree per K: a thread folds its symbols in order, the 64 partial sums of a wave fold by
// wave_sum's xor butterfly (offsets 32 .. 1, own value first), the four wave sums as (W0 + W1) + (W2 + W3) - two
// barriers a sum.  So a segment's bits depend on its symbols alone.  The arithmetic is tdsa_modq_math.hpp's.
#include <hip/hip_runtime.h>

#include "tdsa_modq.hpp"
#include "tdsa_modq_math.hpp"
#include "tdsa_wave.hpp"

// every rounding below is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kT = kModqThreads;

// v[i], i < N: the block's sums in every thread
template <int N>
__device__ inline void block_sums(double (&v)[N], double (*red)[kModqSums], int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[tid >> 6][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  __syncthreads();   // the next reduction writes red behind this barrier
}

__device__ inline ModqC32 c32(float2 v) { return ModqC32{v.x, v.y}; }

__global__ __launch_bounds__(kT) void modq_kernel(ModqLaunch a) {
  extern __shared__ float2 ysh[];    // y[K], then the K indices of the round in hand
  __shared__ double red[kModqWaves][kModqSums];
  __shared__ float2 tab[kModqMaxPoints];
  __shared__ float rabs[kModqMaxPoints];
  __shared__ unsigned hist[2][kModqMaxPoints];
  __shared__ float pkv[kModqWaves];
  __shared__ int pki[kModqWaves];
  const int tid = threadIdx.x;
  const int K = a.K;
  const long long s = blockIdx.x;
  uint8_t* ish = reinterpret_cast<uint8_t*>(ysh + K);
  const float2* seg = a.in + s * a.in_stride;
  uint8_t* idx = a.idx + s * a.out_stride;
  float2* err = a.err ? a.err + s * a.out_stride : nullptr;
  const int T = a.table->T;
  const float inv_rho = a.table->inv_rho;
  const auto at = [&](int i) { return c32(tab[i]); };

  if (tid < kModqMaxPoints) {
    tab[tid] = tid < T ? a.table->r[tid] : make_float2(0.0f, 0.0f);
    rabs[tid] = tid < T ? a.table->r_abs[tid] : 0.0f;
    hist[0][tid] = 0u;
    hist[1][tid] = 0u;
  }

  // ---- 0: the one pass over HBM, and the first guess
  double v0[3] = {0.0, 0.0, 0.0};
  for (int k = tid; k < K; k += kT) {
    const float2 y = seg[k];
    ysh[k] = y;
    v0[0] = v0[0] + double(y.x);
    v0[1] = v0[1] + double(y.y);
    v0[2] = v0[2] + modq_norm64(c32(y));
  }
  block_sums(v0, red, tid);          // its first barrier also stands behind the table and the zeroed counts
  const ModqC64 s_y{v0[0], v0[1]};
  const double s_yy = v0[2];
  ModqC32 ga, gc;
  unsigned flags = modq_first_guess(K, s_y, s_yy, inv_rho, &ga, &gc);
  if (flags & kModqFlagNonFinite) {  // the same for every thread
    const float qnan = __int_as_float(0x7fc00000);
    for (int k = tid; k < K; k += kT) {
      idx[k] = 0;
      if (err) err[k] = make_float2(qnan, qnan);
    }
    if (tid == 0) {
      ModqRecord r = {};
      r.flags = kModqFlagNonFinite;
      a.rec[s] = r;
    }
    return;
  }
  const bool decided = !(flags & kModqFlagDegenerate);

  // ---- 1 - 3: two rounds of decide and fit
  ModqC64 s_ry{0.0, 0.0}, s_cy{0.0, 0.0};
  double s_rr = 0.0;
  int changed = 0;
  for (int r = 0; decided && r < 2; ++r) {
    const ModqC32 q = modq_inverse(ga);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < K; k += kT) {
      const ModqC32 y = c32(ysh[k]);
      const int i = modq_decide(modq_normalise(y, gc, q), at, T);
      if (r == 1) changed += ish[k] != uint8_t(i) ? 1 : 0;
      ish[k] = uint8_t(i);
      atomicAdd(&hist[r][i], 1u);
      const ModqC32 p = at(i);
      const ModqC64 ry = modq_conj_mul(p, y), cy = modq_plain_mul(p, y);
      v[0] = v[0] + ry.re;
      v[1] = v[1] + ry.im;
      v[2] = v[2] + cy.re;
      v[3] = v[3] + cy.im;
    }
    block_sums(v, red, tid);         // behind its barriers the round's counts are whole
    s_ry = ModqC64{v[0], v[1]};
    s_cy = ModqC64{v[2], v[3]};
    ModqC64 s_r;
    int n_max;
    modq_count_sums(at, [&](int i) { return int(hist[r][i]); }, T, &s_r, &s_rr, &n_max);
    if (!modq_fit(K, s_r, s_rr, n_max, s_y, s_ry, &ga, &gc)) flags |= kModqFlagOnePoint;
  }

  // ---- 4: errors, against the second round's decisions
  const ModqC32 q = modq_inverse(ga);
  double e[4] = {0.0, 0.0, 0.0, double(changed)};
  PeakPair best{0.0f, 0};
  for (int k = tid; k < K; k += kT) {
    const ModqC32 y = c32(ysh[k]);
    int i = 0;
    ModqErr er;
    if (decided) {
      i = ish[k];
      er = modq_error(modq_normalise(y, gc, q), at(i), rabs[i]);
    } else {
      er.eps = ModqC32{y.re - gc.re, y.im - gc.im};
      er.e2 = modq_norm32(er.eps);
      er.m = er.p = 0.0f;
    }
    idx[k] = uint8_t(i);
    if (err) err[k] = make_float2(er.eps.re, er.eps.im);
    e[0] = e[0] + double(er.e2);
    e[1] = e[1] + double(er.m) * double(er.m);
    e[2] = e[2] + double(er.p) * double(er.p);
    if (er.e2 > best.v) best = PeakPair{er.e2, k};   // k ascends: the lowest k of the largest; a NaN never wins
  }
  // the larger e2, the lower k where two are equal
  const auto better = [](PeakPair x, PeakPair y) { return x.v > y.v || (x.v == y.v && x.i < y.i); };
  best = wave_best(best, better);
  if ((tid & 63) == 0) {
    pkv[tid >> 6] = best.v;
    pki[tid >> 6] = best.i;
  }
  block_sums(e, red, tid);
  if (tid == 0) {
    best = PeakPair{pkv[0], pki[0]};
    for (int w = 1; w < kModqWaves; ++w)
      if (better(PeakPair{pkv[w], pki[w]}, best)) best = PeakPair{pkv[w], pki[w]};
    ModqRecord rec = {};
    rec.a_re = ga.re;
    rec.a_im = ga.im;
    rec.c_re = gc.re;
    rec.c_im = gc.im;
    rec.s_y[0] = s_y.re;
    rec.s_y[1] = s_y.im;
    rec.s_yy = s_yy;
    rec.s_ry[0] = s_ry.re;
    rec.s_ry[1] = s_ry.im;
    rec.s_cy[0] = s_cy.re;
    rec.s_cy[1] = s_cy.im;
    rec.err_sumsq = e[0];
    rec.ref_sumsq = s_rr;
    rec.mag_sumsq = e[1];
    rec.phase_sumsq = e[2];
    rec.err_peak = best.v;
    rec.err_peak_k = uint32_t(best.i);
    rec.changed = uint32_t(e[3]);
    rec.flags = flags;
    a.rec[s] = rec;
  }
}

}  // namespace

hipError_t launch_modq(const ModqLaunch& a, hipStream_t s) {
  if (a.n_seg < 1) return hipSuccess;
  if (a.K < kModqMinSymbols || a.K > kModqMaxSymbols) return hipErrorInvalidValue;
  const size_t lds = size_t(a.K) * 9;
  hipLaunchKernelGGL(modq_kernel, dim3(unsigned(a.n_seg)), dim3(kT), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
