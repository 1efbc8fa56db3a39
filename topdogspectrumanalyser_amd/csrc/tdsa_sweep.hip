// tdsa_sweep.hip - the sweep assembler's two kernels.
//
//   sweep_detector_kernel  rows [steps][frames][nfft] float32 dB -> T [steps][K]: the kept range [k0, k1) of every step's
//                          rows folded over the frames (last / max / min / mean of linear power).  One lane owns four
//                          adjacent bins of the row: a 16-byte load per frame where the quad lies whole inside the kept
//                          range, scalar loads at its ragged head and tail.
//   sweep_stitch_kernel    T of the steps present -> float64 trace on the host's frequency grid: np.interp over the
//                          concatenated kept bins, or the maximum of the bins in each grid cell.  One lane per grid
//                          point; the steps' first frequencies sit in LDS for the binary search.
//
// The frequency of kept bin k of a step is centre + (koff + k) * bin_hz: one float64 multiply, one float64 add.  Every
// comparison the stitch makes is on that expression, and its interpolation is np.interp's, rounding for rounding, so
// nothing in this file may contract into a fused multiply-add.  The arithmetic is written with plain operators for
// that reason: the pragma governs the operations spelled out here, not those inside the runtime headers' __dmul_rn /
// __dadd_rn, which the compiler is free to fuse with each other once they are inlined.
#pragma clang fp contract(off)
#include "tdsa_sweep.hpp"

#include "../../include/tdsa_hip.h"

namespace tdsa {
namespace {

constexpr int kDetBlock = 256;
constexpr int kDetBatch = 8;        // frames whose loads are in flight together
constexpr int kStitchBlock = 256;
constexpr int kStitchMaxBlocks = 2048;

constexpr float kDbToLog2 = 0.33219280948873623f;   // log2(10) / 10
constexpr float kLog2ToDb = 3.0102999566398120f;    // 10 / log2(10)

// ---- detector --------------------------------------------------------------------------------------------------------
template <int DET>
struct Fold;
template <>
struct Fold<TDSA_SWEEP_DET_MAX> {   // np.max: the first NaN stays
  float acc;
  __device__ void first(float v) { acc = v; }
  __device__ void next(float v) { acc = (acc != acc) ? acc : ((v > acc || v != v) ? v : acc); }
  __device__ float result(int) const { return acc; }
};
template <>
struct Fold<TDSA_SWEEP_DET_MIN> {
  float acc;
  __device__ void first(float v) { acc = v; }
  __device__ void next(float v) { acc = (acc != acc) ? acc : ((v < acc || v != v) ? v : acc); }
  __device__ float result(int) const { return acc; }
};
template <>
struct Fold<TDSA_SWEEP_DET_AVG> {   // 10 log10(max(mean(10^(d/10)), 1e-30)), the sum in float64 in frame order
  double acc;
  __device__ void first(float v) { acc = double(exp2f(v * kDbToLog2)); }
  __device__ void next(float v) { acc += double(exp2f(v * kDbToLog2)); }
  __device__ float result(int frames) const {
    const double mean = acc / double(frames);
    const double m = mean < 1e-30 ? 1e-30 : mean;   // a NaN stays
    return log2f(float(m)) * kLog2ToDb;
  }
};

template <int DET>
__global__ __launch_bounds__(kDetBlock) void sweep_detector_kernel(const float* __restrict__ rows, long long step_stride,
                                                                   int frames, int nfft, int k0, int k1, int vec,
                                                                   float* __restrict__ T) {
  const int K = k1 - k0;
  const float* base = rows + (long long)blockIdx.y * step_stride;
  float* out = T + (long long)blockIdx.y * K;
  const int b0 = ((k0 >> 2) + int(blockIdx.x) * kDetBlock + int(threadIdx.x)) * 4;   // this lane's quad of the row
  if (b0 >= k1) return;
  if constexpr (DET == TDSA_SWEEP_DET_SAMPLE) {
    base += (long long)(frames - 1) * nfft;
    frames = 1;
  }
  if (vec && b0 >= k0 && b0 + 4 <= k1) {
    const float* src = base + b0;
    float4 r;
    if constexpr (DET == TDSA_SWEEP_DET_SAMPLE) {
      r = *reinterpret_cast<const float4*>(src);
    } else {
      Fold<DET> a, b, c, d;
      float4 v = *reinterpret_cast<const float4*>(src);
      a.first(v.x); b.first(v.y); c.first(v.z); d.first(v.w);
      int f = 1;
      for (; f + kDetBatch <= frames; f += kDetBatch) {
        float4 w[kDetBatch];
#pragma unroll
        for (int i = 0; i < kDetBatch; ++i) w[i] = *reinterpret_cast<const float4*>(src + (long long)(f + i) * nfft);
#pragma unroll
        for (int i = 0; i < kDetBatch; ++i) {
          a.next(w[i].x); b.next(w[i].y); c.next(w[i].z); d.next(w[i].w);
        }
      }
      for (; f < frames; ++f) {
        v = *reinterpret_cast<const float4*>(src + (long long)f * nfft);
        a.next(v.x); b.next(v.y); c.next(v.z); d.next(v.w);
      }
      r = make_float4(a.result(frames), b.result(frames), c.result(frames), d.result(frames));
    }
    float* dst = out + (b0 - k0);
    dst[0] = r.x; dst[1] = r.y; dst[2] = r.z; dst[3] = r.w;
    return;
  }
  // ragged head / tail of the kept range, and rows a 16-byte load cannot take: bin by bin
  for (int e = 0; e < 4; ++e) {
    const int b = b0 + e;
    if (b < k0 || b >= k1) continue;
    const float* src = base + b;
    float r;
    if constexpr (DET == TDSA_SWEEP_DET_SAMPLE) {
      r = *src;
    } else {
      Fold<DET> a;
      a.first(*src);
      for (int f = 1; f < frames; ++f) a.next(src[(long long)f * nfft]);
      r = a.result(frames);
    }
    out[b - k0] = r;
  }
}

// ---- stitch ----------------------------------------------------------------------------------------------------------
// xp, the concatenation of the present steps' kept-bin frequencies, is addressed as (p, k): step p of the present ones,
// kept bin k.  Its linear index is p K + k.
struct Xp {
  const double2* tab;   // LDS: (x of kept bin 0, centre) per present step
  int P, K, koff;
  double bin, inv_bin;

  __device__ double at(int p, int k) const { return tab[p].y + double(koff + k) * bin; }

  // largest (p, k) with xp <= x; x >= xp[0] (and not NaN) is the caller's business
  __device__ void find_le(double x, int* p_out, int* k_out) const {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tab[mid].x <= x) lo = mid; else hi = mid;
    }
    const double t = (x - tab[lo].x) * inv_bin;      // a guess; only the exact expression decides
    int k = t >= double(K - 1) ? K - 1 : int(t);
    while (k < K - 1 && at(lo, k + 1) <= x) ++k;
    while (k > 0 && at(lo, k) > x) --k;
    *p_out = lo;
    *k_out = k;
  }

  // linear index of the first xp >= v (P K when there is none)
  __device__ long long lower_bound(double v) const {
    if (v <= tab[0].x) return 0;
    int p, k;
    find_le(v, &p, &k);
    const long long j = (long long)p * K + k;
    return at(p, k) == v ? j : j + 1;
  }
};

__device__ double sweep_interp(const Xp& xp, const float* __restrict__ T, const int* __restrict__ step_of, double x) {
  const int P = xp.P, K = xp.K;
  if (x < xp.tab[0].x) return double(T[(long long)step_of[0] * K]);
  int p, k;
  xp.find_le(x, &p, &k);
  const float* row = T + (long long)step_of[p] * K;
  const double x0 = xp.at(p, k), f0 = double(row[k]);
  if ((p == P - 1 && k == K - 1) || x0 == x) return f0;   // beyond the last bin as well
  double x1, f1;
  if (k < K - 1) {
    x1 = xp.at(p, k + 1);
    f1 = double(row[k + 1]);
  } else {
    x1 = xp.tab[p + 1].x;
    f1 = double(T[(long long)step_of[p + 1] * K]);
  }
  const double slope = (f1 - f0) / (x1 - x0);
  double r = slope * (x - x0) + f0;
  if (r != r) {
    r = slope * (x - x1) + f1;
    if (r != r && f0 == f1) r = f0;
  }
  return r;
}

__global__ __launch_bounds__(kStitchBlock) void sweep_stitch_kernel(SweepStitchLaunch a) {
  extern __shared__ double2 s_tab[];
  for (int i = threadIdx.x; i < a.n_present; i += kStitchBlock) s_tab[i] = a.tab[i];
  __syncthreads();
  Xp xp{s_tab, a.n_present, a.K, a.koff, a.bin_hz, 1.0 / a.bin_hz};
  for (int i = blockIdx.x * kStitchBlock + threadIdx.x; i < a.n_grid; i += gridDim.x * kStitchBlock) {
    const double x = a.grid[i];
    double r;
    bool done = false;
    if (a.n_present == 0) {
      r = __builtin_nan("");
      done = true;
    } else if (a.mode == TDSA_SWEEP_PEAK) {
      const double half = 0.5 * a.h;
      const long long j0 = xp.lower_bound(x - half);
      const long long j1 = xp.lower_bound(x + half);
      if (j1 > j0) {   // the cell holds bins: their maximum, a NaN stays
        int p = int(j0 / a.K), k = int(j0 - (long long)p * a.K);
        const float* row = a.T + (long long)a.step_of[p] * a.K;
        float m = row[k];
        for (long long j = j0 + 1; j < j1; ++j) {
          if (++k == a.K) {
            k = 0;
            row = a.T + (long long)a.step_of[++p] * a.K;
          }
          const float v = row[k];
          m = (m != m) ? m : ((v > m || v != v) ? v : m);
        }
        r = double(m);
        done = true;
      }
    }
    if (!done) r = sweep_interp(xp, a.T, a.step_of, x);
    a.out[i] = r;
  }
}

}  // namespace

hipError_t launch_sweep_detector(const SweepDetLaunch& a, hipStream_t s) {
  if (a.n_steps <= 0) return hipSuccess;
  const int quads = (a.k1 + 3) / 4 - a.k0 / 4;
  const dim3 grid((quads + kDetBlock - 1) / kDetBlock, a.n_steps);
  const int vec = (reinterpret_cast<uintptr_t>(a.rows) % 16 == 0 && a.nfft % 4 == 0 && a.step_stride % 4 == 0) ? 1 : 0;
#define TDSA_SWEEP_DET(D)                                                                                          \
  hipLaunchKernelGGL(sweep_detector_kernel<D>, grid, dim3(kDetBlock), 0, s, a.rows, a.step_stride, a.frames, a.nfft, \
                     a.k0, a.k1, vec, a.T)
  switch (a.detector) {
    case TDSA_SWEEP_DET_SAMPLE: TDSA_SWEEP_DET(TDSA_SWEEP_DET_SAMPLE); break;
    case TDSA_SWEEP_DET_MAX: TDSA_SWEEP_DET(TDSA_SWEEP_DET_MAX); break;
    case TDSA_SWEEP_DET_MIN: TDSA_SWEEP_DET(TDSA_SWEEP_DET_MIN); break;
    case TDSA_SWEEP_DET_AVG: TDSA_SWEEP_DET(TDSA_SWEEP_DET_AVG); break;
    default: return hipErrorInvalidValue;
  }
#undef TDSA_SWEEP_DET
  return hipGetLastError();
}

hipError_t launch_sweep_stitch(const SweepStitchLaunch& a, hipStream_t s) {
  if (a.n_grid <= 0) return hipSuccess;
  int blocks = (a.n_grid + kStitchBlock - 1) / kStitchBlock;
  if (blocks > kStitchMaxBlocks) blocks = kStitchMaxBlocks;
  hipLaunchKernelGGL(sweep_stitch_kernel, dim3(blocks), dim3(kStitchBlock), size_t(a.n_present) * sizeof(double2), s, a);
  return hipGetLastError();
}

}  // namespace tdsa
