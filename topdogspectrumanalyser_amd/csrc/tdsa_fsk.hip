// tdsa_fsk.hip - FSK analysis: symbol clock, deviation per level, symbols, FSK error.
//
// fsk_kernel<KIND>: one workgroup of 256 threads per segment, the stages separated by barriers, KIND the input (complex64
// through the discriminator, or float32 that is a frequency already).
// The stages are numbered as in the contract (include/tdsa_hip.h): 0 discriminate, 1 boxcar, 2 timing, ...
//   0 - 2 timing  the segment in tiles of 1024 differences: the tile's d_j into LDS (a sample passes through the
//                 arctangent once per tile), its boxcar sums b_j beside them, then e_j = (b_j+L - b_j)^2, P = sum e_j,
//                 C = sum e_j exp(-2 pi i (j nu mod 2^32) / 2^32), delta_fx from arg C
//   3 resample    v_k = cubic Lagrange over b at delta_fx + k step, k < K, kept in LDS (and stored): a symbol recomputes
//                 the B + 3 values of d under its four taps, which one running pass turns into the four sums
//   4 levels      lo, hi, the first guess, then two rounds of decide and least-squares fit
//   5 errors      err_k, their float64 sum of squares, the largest with its lowest k
// The tile's LDS is read at stride one by consecutive threads: d_t[m + i] at step i of thread m's sum, no bank meets twice.
//
// Every sum is one fixed tree per (seg_len, B, L, K): thread t folds its elements t, t + 256, ... in order, then the 256
// partial sums fold pairwise, (t, t + 128), (t, t + 64), ...  So a segment's results depend on its samples alone, not on
// n_seg or on which segment it is.  The arithmetic is tdsa_fsk_math.hpp's and what that includes.
#include <hip/hip_runtime.h>

#include "tdsa_fsk.hpp"
#include "tdsa_fsk_math.hpp"
#include "tdsa_seg_block.hpp"

// every rounding below is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kT = kSegThreads;

// a segment that is not finite: NaN levels, zero indices, a zero record with the flag; a thread rewrites only the
// out[k] it wrote itself
__device__ inline void fsk_not_finite(FskRecord* rec, float* out, uint8_t* idx, int K, int tid) {
  const float qnan = __int_as_float(0x7fc00000);
  for (int k = tid; k < K; k += kT) {
    out[k] = qnan;
    if (idx) idx[k] = 0;
  }
  if (tid == 0) {
    FskRecord r = {};
    r.flags = kFskFlagNonFinite;
    *rec = r;
  }
}

template <int KIND>
__global__ __launch_bounds__(kT) void fsk_kernel(FskLaunch a) {
  extern __shared__ float v[];       // v[K]
  __shared__ float4 red[kT];
  __shared__ double2 redd[kT];
  __shared__ float td[kFskTileD];
  __shared__ float tb[kFskTileB];
  const int tid = threadIdx.x;
  const int K = a.K, M = a.levels, B = a.boxcar, L = a.lag;
  const long long s = blockIdx.x;
  const void* seg = KIND == kFskIq ? static_cast<const void*>(static_cast<const float2*>(a.in) + s * a.hop)
                                   : static_cast<const void*>(static_cast<const float*>(a.in) + s * a.hop);
  float* out = a.out + s * a.out_stride;
  uint8_t* idx = a.idx ? a.idx + s * a.out_stride : nullptr;
  const int n_d = int(a.seg_len) - (KIND == kFskIq ? 1 : 0);
  const int n_b = n_d - B + 1, n_e = n_b - L;
  const float inv_b = fsk_boxcar_scale(B);

  // ---- 0 - 2: timing.  Tile [j0, j0 + ne) of e needs b[j0 .. j0 + ne + L) and d[j0 .. j0 + ne + L + B - 1): the last of
  // them is d[n_e + L + B - 2] = d[n_d - 1].
  float pw = 0.0f, cr = 0.0f, ci = 0.0f;
  for (int j0 = 0; j0 < n_e; j0 += kFskTile) {
    const int ne = n_e - j0 < kFskTile ? n_e - j0 : kFskTile;
    const int nb = ne + L, nd = nb + B - 1;
    for (int m = tid; m < nd; m += kT) td[m] = seg_disc<KIND == kFskIq>(seg, j0 + m);
    __syncthreads();
    seg_boxcar_tile(td, tb, nb, B, inv_b, tid);
    __syncthreads();   // the next tile writes td behind this barrier, tb behind its own first
    for (int m = tid; m < ne; m += kT) {
      const float df = tb[m + L] - tb[m];
      const float e = df * df;
      const float2 w = rot(a.nco, uint32_t(j0 + m) * a.nu);
      pw = pw + e;
      cr = fmaf(e, w.x, cr);
      ci = fmaf(e, w.y, ci);
    }
  }
  const float4 s1 = block_sum3(pw, cr, ci, red, tid);
  const float P = s1.x, Cr = s1.y, Ci = s1.z;
  FskRecord rec = {};
  if (!(isfinite(P) && isfinite(Cr) && isfinite(Ci))) {   // the same for every thread
    fsk_not_finite(a.rec + s, out, idx, K, tid);
    return;
  }
  const uint64_t delta = a.fixed ? a.delta_fx : fsk_delta(Cr, Ci, a.step, L);
  rec.delta_fx = delta;
  rec.c_re = Cr;
  rec.c_im = Ci;
  rec.p = P;

  // ---- 3: resample.  delta >= 2^32 and K's definition keep b[i - 1 .. i + 2] inside n_b, that is d[i - 1 .. i + B + 1]
  // inside n_d.  One pass over those B + 3 values feeds the four sums, each from its own first term on.
  float lo = INFINITY, hi = -INFINITY, bad = 0.0f;
  for (int k = tid; k < K; k += kT) {
    const uint64_t pos = delta + uint64_t(k) * a.step;
    const int i = int(sym_index(pos));
    float c[4];
    sym_coeffs(sym_mu(pos), c);
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
    float2 prev = make_float2(0.0f, 0.0f);
    if constexpr (KIND == kFskIq) prev = static_cast<const float2*>(seg)[i - 1];
    for (int m = 0; m < B + 3; ++m) {
      float dm;
      if constexpr (KIND == kFskIq) {
        const float2 nx = static_cast<const float2*>(seg)[i + m];
        dm = demod_fm(nx.x, nx.y, prev.x, prev.y);
        prev = nx;
      } else {
        dm = static_cast<const float*>(seg)[i - 1 + m];
      }
      b0 = m == 0 ? dm : m < B ? b0 + dm : b0;
      b1 = m == 1 ? dm : m > 1 && m < B + 1 ? b1 + dm : b1;
      b2 = m == 2 ? dm : m > 2 && m < B + 2 ? b2 + dm : b2;
      b3 = m == 3 ? dm : m > 3 ? b3 + dm : b3;
    }
    const float vk = sym_interp(c, b0 * inv_b, b1 * inv_b, b2 * inv_b, b3 * inv_b);
    v[k] = vk;
    out[k] = vk;
    lo = vk < lo ? vk : lo;
    hi = vk > hi ? vk : hi;
    if (!isfinite(vk)) bad = 1.0f;
  }

  // ---- 4: levels.  A thread reads back only the v_k it wrote (k = tid, tid + 256, ...) in every loop below.
  const float4 mm = block_minmax(lo, hi, bad, red, tid);
  if (mm.z > 0.0f) {   // a v_k that is not finite, which P and C did not show: the same for every thread
    fsk_not_finite(a.rec + s, out, idx, K, tid);
    return;
  }
  rec.lo = mm.x;
  rec.hi = mm.y;
  float o, g, od = 0.0f, gd = 0.0f;   // the line, and the one the round in hand decides by
  fsk_first_guess(mm.x, mm.y, M, &o, &g);
  for (int r = 0; r < 2; ++r) {
    od = o;
    gd = g;
    int sl = 0, sl2 = 0;
    double sv = 0.0, slv = 0.0;
    for (int k = tid; k < K; k += kT) {
      const float vk = v[k];
      const int l = fsk_level(fsk_decide(vk, od, gd, M), M);
      sl += l;
      sl2 += l * l;
      sv = sv + double(vk);
      slv = slv + double(l) * double(vk);
    }
    const int4 si = block_sum2i(sl, sl2, reinterpret_cast<int4*>(red), tid);
    const double2 sd = block_sum2(sv, slv, redd, tid);
    if (!fsk_fit(K, si.x, si.y, sd.x, sd.y, &o, &g)) rec.flags |= kFskFlagOneLevel;
    rec.sum_l = si.x;
  }
  rec.offset = o;
  rec.dev = g;

  // ---- 5: errors, against the second round's decisions
  double se = 0.0;
  float best = 0.0f;
  int bk = 0;
  for (int k = tid; k < K; k += kT) {
    const float vk = v[k];
    const int i = fsk_decide(vk, od, gd, M);
    if (idx) idx[k] = uint8_t(i);
    const float er = fsk_err(vk, o, g, fsk_level(i, M));
    se = se + double(er) * double(er);
    const float ae = fabsf(er);
    if (ae > best) {
      best = ae;
      bk = k;
    }
  }
  const double2 ss = block_sum2(se, 0.0, redd, tid);
  const float4 am = block_argmax(best, bk, red, tid);
  rec.err_sumsq = ss.x;
  rec.err_peak = am.x;
  rec.err_peak_k = __float_as_int(am.y);
  if (tid == 0) a.rec[s] = rec;
}

}  // namespace

hipError_t launch_fsk(const FskLaunch& a, hipStream_t s) {
  if (a.n_seg < 1) return hipSuccess;
  const size_t lds = size_t(a.K) * sizeof(float);
  if (a.K < 1 || lds + kFskStaticLdsBytes > size_t(kFskMaxLdsBytes)) return hipErrorInvalidValue;
  if (a.kind == kFskIq) hipLaunchKernelGGL(fsk_kernel<kFskIq>, dim3(unsigned(a.n_seg)), dim3(kT), lds, s, a);
  else hipLaunchKernelGGL(fsk_kernel<kFskFreq>, dim3(unsigned(a.n_seg)), dim3(kT), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
