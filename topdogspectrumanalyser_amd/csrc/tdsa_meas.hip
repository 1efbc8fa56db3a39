// tdsa_meas.hip - channel measurements on dB rows that sit in device memory (the contract is
// tests/meas_contract.py).  One workgroup of 256 threads takes a row at a time, staged once into LDS with one float of
// padding per 64 bins (bin i at float i + i / 64):
//   channels  one wave per channel, in rounds: peak, NaN count and power.  Lane l adds bins lo + l, lo + l + 64, ... in
//             order and the 64 partial sums meet in tdsa::wave_sum<64> - the detector's tree, so a channel set to a
//             detector record's [start, stop] has that record's power bits.
//   obw       thread t owns bins 64 t .. 64 t + 63 of the range and adds them in order; an exclusive scan over the 256
//             sums gives it E_t, the power below its bins.  The cumulative power at its j-th bin is E_t + (the sum of its
//             first j bins), so the first thread whose last bin reaches a target holds the crossing, and only it walks.
//             The padding puts the 64 walkers of a wave on 64 distinct LDS banks.
//   peak, mask  one strided pass over the row: the range's peak, and per bin the limit test and the margin
//   x-dB      one strided pass over the range: first and last bin within xdb of the peak
// Every fold across lanes is tdsa_wave.hpp's; across the four waves the results meet in LDS in wave order.  No
// floating-point atomics: a row's records are a function of its bins and the configuration alone.
#include "tdsa_meas.hpp"

#include "tdsa_rows_align.hpp"
#include "tdsa_wave.hpp"

namespace tdsa {
namespace {

constexpr int kT = kMeasThreads;
constexpr int kW = kT / 64;
constexpr int kBig = 0x7fffffff;

__device__ __forceinline__ int pad(int i) { return i + (i >> 6); }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// (value, bin) of a maximum so far; bin == kBig: none yet.  The larger value wins, the lower bin among equals; a NaN
// never enters.
__device__ __forceinline__ bool better(const PeakPair& q, const PeakPair& p) {
  return q.i != kBig && (p.i == kBig || q.v > p.v || (q.v == p.v && q.i < p.i));
}
__device__ __forceinline__ void take(PeakPair& p, float v, int i) {   // a lane's bins come in ascending order
  if (v == v && (p.i == kBig || v > p.v)) p = PeakPair{v, i};
}
__device__ __forceinline__ double linear(float v) { return (double)exp10f(v / 10.0f); }   // rows_stats_kernel's expression

struct Cross {   // one edge of the occupied bandwidth
  int k;
  double x;
};

// The thread that holds the crossing of `target` walks its bins b0 .. b1: S[k] = E + (the sum of its bins up to k), the
// first k with S[k] >= target.  (A thread chosen because no thread's last bin reached the target - the targets and the
// scan round differently - ends at its last bin that holds power.)
__device__ __forceinline__ Cross walk(const float* row, int b0, int b1, double E, double target) {
  double inner = 0.0, below = E, pk = 0.0;
  int k = -1;
  for (int i = b0; i <= b1; ++i) {
    const float v = row[pad(i)];
    if (v != v) continue;
    const double p = linear(v);
    const double next = inner + p;
    if (E + next >= target) {
      k = i;
      below = E + inner;
      pk = p;
      break;
    }
    if (p > 0.0) {
      k = i;
      below = E + inner;
      pk = p;
    }
    inner = next;
  }
  Cross c;
  c.k = k;
  const double left = double(k) - 0.5, right = double(k) + 0.5;
  double x = pk > 0.0 ? left + (target - below) / pk : left;
  x = x < left ? left : x;
  x = x > right ? right : x;
  c.x = k < 0 ? (double)quiet_nan() : x;
  return c;
}

// the first set bit of four ballot words in wave order, as a thread number; -1: none
__device__ __forceinline__ int first_thread(const unsigned long long* wd) {
  for (int k = 0; k < kW; ++k)
    if (wd[k]) return 64 * k + __ffsll((long long)wd[k]) - 1;
  return -1;
}
__device__ __forceinline__ int last_thread(const unsigned long long* wd) {
  for (int k = kW - 1; k >= 0; --k)
    if (wd[k]) return 64 * k + 63 - __clzll((long long)wd[k]);
  return -1;
}

template <bool VEC>
__global__ void __launch_bounds__(kT) meas_kernel(MeasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) float row[];     // [n + n / 64], padded
  __shared__ double s_tot[kW];                        // the scan's wave totals
  __shared__ unsigned long long s_word[3][kW];        // threads whose last bin reaches t_lo / t_hi; threads with power
  __shared__ PeakPair s_pair[2][kW];                  // the range's peak, the worst margin
  __shared__ int s_int[6][kW];                        // n_nan, n_fail, first_fail, last_fail, xdb_lo, xdb_hi
  __shared__ Cross s_cross[2];
  __shared__ float s_ref;                             // channel 0's peak_db
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = a.n, lo = a.obw_lo, hi = a.obw_hi;
  const auto add = [](auto x, auto y) { return x + y; };
  const auto imin = [](int x, int y) { return y < x ? y : x; };
  const auto imax = [](int x, int y) { return y > x ? y : x; };

  for (size_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
    const float* src = a.rows + r * size_t(n);
    if (VEC) {
      typedef float f4 __attribute__((ext_vector_type(4)));
      const f4* src4 = reinterpret_cast<const f4*>(src);
      for (int j = tid; j < n / 4; j += kT) {
        const f4 v = __builtin_nontemporal_load(src4 + j);        // read once
        float* dst = row + pad(4 * j);                // four bins of one 64-bin group: contiguous in the padded row
        dst[0] = v.x;
        dst[1] = v.y;
        dst[2] = v.z;
        dst[3] = v.w;
      }
    } else {
      for (int i = tid; i < n; i += kT) row[pad(i)] = src[i];
    }
    __syncthreads();

    // ---- channels: one wave each, in rounds
    MeasChannel* ch_out = a.ch_rec + r * size_t(a.C);
    for (int c = w; c < a.C; c += kW) {
      const int c_lo = a.ch_lo[c], c_hi = a.ch_hi[c];
      PeakPair pk{0.0f, kBig};
      double pw = 0.0;
      int nn = 0;
      for (int i = c_lo + lane; i <= c_hi; i += 64) {
        const float v = row[pad(i)];
        take(pk, v, i);
        if (v == v) pw += linear(v);
        else ++nn;
      }
      pk = wave_best(pk, [](const PeakPair& q, const PeakPair& p) { return better(q, p); });
      pw = wave_sum<64>(pw);
      nn = wave_sum<64>(nn);
      if (lane == 0) {
        MeasChannel g;
        g.power = pw;
        g.peak_db = pk.i == kBig ? quiet_nan() : pk.v;
        g.peak_bin = pk.i == kBig ? -1 : pk.i;
        g.n_nan = nn;
        g.reserved = 0;
        ch_out[c] = g;
        if (c == 0) s_ref = g.peak_db;
      }
    }

    // ---- occupied bandwidth: the threads' sums, their scan, the total
    const int b0 = 64 * tid > lo ? 64 * tid : lo;
    const int b1 = 64 * tid + 63 < hi ? 64 * tid + 63 : hi;
    double own = 0.0;
    int nn = 0;
    for (int i = b0; i <= b1; ++i) {
      const float v = row[pad(i)];
      if (v == v) own += linear(v);
      else ++nn;
    }
    const double inc = wave_scan_inclusive(own, add);
    const double exc = wave_lane_below(inc, 0.0);
    nn = wave_sum<64>(nn);
    if (lane == 63) s_tot[w] = inc;
    if (lane == 0) s_int[0][w] = nn;
    __syncthreads();                                  // (also publishes s_ref)
    double pre = 0.0, T = 0.0;
    int n_nan = 0;
#pragma unroll
    for (int k = 0; k < kW; ++k) {
      const double t = s_tot[k];
      if (k < w) pre += t;
      T += t;
      n_nan += s_int[0][k];
    }
    const double E = pre + exc, I = E + own;          // the power below this thread's bins, and up to its last
    int flags = !(T > 0.0) ? kMeasFlagEmpty : T == (double)INFINITY ? kMeasFlagInf : 0;
    const double t_lo = T * (1.0 - a.f) / 2.0, t_hi = T * (1.0 + a.f) / 2.0;
    {
      const bool has = b0 <= b1;
      const unsigned long long m_lo = __ballot(has && I >= t_lo), m_hi = __ballot(has && I >= t_hi);
      const unsigned long long m_pw = __ballot(has && own > 0.0);
      if (lane == 0) {
        s_word[0][w] = m_lo;
        s_word[1][w] = m_hi;
        s_word[2][w] = m_pw;
      }
    }
    __syncthreads();
    if (flags == 0) {
      int at_lo = first_thread(s_word[0]), at_hi = first_thread(s_word[1]);
      if (at_lo < 0) at_lo = last_thread(s_word[2]);
      if (at_hi < 0) at_hi = last_thread(s_word[2]);
      if (tid == at_lo) s_cross[0] = walk(row, b0, b1, E, t_lo);
      if (tid == at_hi) s_cross[1] = walk(row, b0, b1, E, t_hi);
    }

    // ---- the range's peak, and the limit line over the whole row
    const float ref = a.relative ? s_ref : 0.0f;
    PeakPair pk{0.0f, kBig}, worst{0.0f, kBig};
    int n_fail = 0, first_fail = kBig, last_fail = -1;
    for (int i = tid; i < n; i += kT) {
      const float v = row[pad(i)];
      if (i >= lo && i <= hi) take(pk, v, i);
      if (a.limit) {
        const float l = a.limit[i];
        const float lim = a.relative ? l + ref : l;
        if (v > lim) {
          ++n_fail;
          first_fail = first_fail < i ? first_fail : i;
          last_fail = i;
        }
        take(worst, v - lim, i);
      }
    }
    const auto pair_better = [](const PeakPair& q, const PeakPair& p) { return better(q, p); };
    pk = wave_best(pk, pair_better);
    worst = wave_best(worst, pair_better);
    n_fail = wave_sum<64>(n_fail);
    first_fail = wave_reduce(first_fail, imin);
    last_fail = wave_reduce(last_fail, imax);
    if (lane == 0) {
      s_pair[0][w] = pk;
      s_pair[1][w] = worst;
      s_int[1][w] = n_fail;
      s_int[2][w] = first_fail;
      s_int[3][w] = last_fail;
    }
    __syncthreads();
    pk = s_pair[0][0];
    worst = s_pair[1][0];
    n_fail = s_int[1][0];
    first_fail = s_int[2][0];
    last_fail = s_int[3][0];
#pragma unroll
    for (int k = 1; k < kW; ++k) {
      if (better(s_pair[0][k], pk)) pk = s_pair[0][k];
      if (better(s_pair[1][k], worst)) worst = s_pair[1][k];
      n_fail += s_int[1][k];
      first_fail = imin(first_fail, s_int[2][k]);
      last_fail = imax(last_fail, s_int[3][k]);
    }

    // ---- x-dB: the first and the last bin of the range within xdb of its peak
    int x_lo = kBig, x_hi = -1;
    if (pk.i != kBig) {
      const float edge = pk.v - a.xdb;
      for (int i = lo + tid; i <= hi; i += kT) {
        if (row[pad(i)] >= edge) {
          x_lo = x_lo < i ? x_lo : i;
          x_hi = i;
        }
      }
    }
    x_lo = wave_reduce(x_lo, imin);
    x_hi = wave_reduce(x_hi, imax);
    if (lane == 0) {
      s_int[4][w] = x_lo;
      s_int[5][w] = x_hi;
    }
    __syncthreads();                                  // (also publishes s_cross)
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < kW; ++k) {
        x_lo = imin(x_lo, s_int[4][k]);
        x_hi = imax(x_hi, s_int[5][k]);
      }
      MeasRow q;
      q.obw_total = T;
      if (flags == 0) {
        q.x_lo = s_cross[0].x;
        q.x_hi = s_cross[1].x;
        q.k_lo = s_cross[0].k;
        q.k_hi = s_cross[1].k;
      } else {
        q.x_lo = q.x_hi = (double)quiet_nan();
        q.k_lo = q.k_hi = -1;
      }
      q.xdb_lo = x_lo == kBig ? -1 : x_lo;
      q.xdb_hi = x_hi;
      q.peak_bin = pk.i == kBig ? -1 : pk.i;
      q.peak_db = pk.i == kBig ? quiet_nan() : pk.v;
      q.n_nan = n_nan;
      q.n_fail = n_fail;
      q.worst_bin = worst.i == kBig ? -1 : worst.i;
      q.worst_margin = worst.i == kBig ? quiet_nan() : worst.v;
      q.first_fail = first_fail == kBig ? -1 : first_fail;
      q.last_fail = last_fail;
      if (n_fail > 0) flags |= kMeasFlagMaskFail;
      q.flags = flags;
      q.reserved = 0;
      a.row_rec[r] = q;
    }
    __syncthreads();                                  // the row and the scratch are rewritten by the next row
  }
}

}  // namespace

hipError_t meas_prepare() {
  const int bytes = kMeasMaxLdsBytes - kMeasStaticLdsBytes;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&meas_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&meas_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}

hipError_t launch_meas(const MeasLaunch& a, hipStream_t s) {
  if (a.n_rows < 1) return hipSuccess;
  if (a.n < 1 || a.n > kMeasMaxBins || a.C < 1 || a.C > kMeasMaxChannels || a.obw_lo < 0 || a.obw_hi >= a.n ||
      a.obw_lo > a.obw_hi || !(a.f > 0.0 && a.f < 1.0) || !(a.xdb >= 0.0f) || !a.rows || !a.row_rec || !a.ch_rec)
    return hipErrorInvalidValue;
  for (int c = 0; c < a.C; ++c)
    if (a.ch_lo[c] < 0 || a.ch_hi[c] >= a.n || a.ch_lo[c] > a.ch_hi[c]) return hipErrorInvalidValue;
  const size_t lds = (size_t(a.n + (a.n - 1) / kMeasOwn) * sizeof(float) + 15) & ~size_t(15);
  const unsigned grid = unsigned(a.n_rows < size_t(kMeasMaxGrid) ? a.n_rows : size_t(kMeasMaxGrid));
  if (rows_take_vec16(a.rows, a.n))
    hipLaunchKernelGGL(meas_kernel<true>, dim3(grid), dim3(kT), lds, s, a);
  else
    hipLaunchKernelGGL(meas_kernel<false>, dim3(grid), dim3(kT), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
