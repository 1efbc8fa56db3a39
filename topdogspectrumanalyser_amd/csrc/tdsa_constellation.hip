// tdsa_constellation.hip - Constellation2D.update_iq_data (displays/constellation_2d.py:104-160 of the reference) on the
// device, bit for bit.  Per segment of IQ samples:
//
//   power pass   per 8192-sample block: numpy's pairwise sum of fl(|x|^2), |x| = L * sqrtf(fmaf(S/L, S/L, 1)) as numpy's
//                complex64 absolute computes it
//   symbol pass  fold of the block sums from 0 (numpy's add.reduce), mean = float32(double(sum) / N), rms = sqrtf(mean),
//                AGC when rms > float32(1e-10): re * (1/rms), im * (1/rms) by numpy's complex division; then per sample
//                the minimum squared distance to the reference table (per-block pairwise sums, float or double as the
//                table), the histogram2d bin against float64 linspace edges, and the scatter tail
//   EVM fold     fold of the distance block sums, mean, sqrt
//
// Pairwise sums: a full block is 64 leaves of 128 (eight accumulators each, seeded with a[0..7]) under a perfect
// binary tree; 256 threads form the 512 accumulator chains, wave 0 combines the leaves and the tree with shuffles.  A
// partial block (the last one of a segment) takes numpy's recursion literally: lane 0 lists the leaves, one thread per
// leaf sums it, lane 0 walks the tree again to combine them.
//
// Exactness: every sum, product and difference below is one IEEE operation (contraction is off for the whole file;
// the one fused multiply-add is numpy's own, inside |x|); division and sqrt are HIP's correctly rounded ones.  On a
// grid table (the point set is X x Y) the minimum over the grid is fl(min_x fl((i-x)^2) + min_y fl((q-y)^2)) because
// rounding is monotone, so the per-axis minima give exactly the brute-force value; other tables (8psk) run brute force.
// NaN propagates as in np.min.  The histogram counts are integer LDS adds merged with integer atomics: order-free.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tdsa_constellation.hpp"
#include "tdsa_unpack.hpp"

#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kThreads = 256;
// checked for every n <= 8192 by tests/test_constellation_host.py: at most 65 leaves (every leaf of a split holds at
// least 64 elements), the deepest leaf 7 splits below the root
constexpr int kMaxLeaves = 128;
constexpr int kStack = 16;

struct Walk {                     // LDS of the partial-block path
  int lstart[kMaxLeaves], lsize[kMaxLeaves];
  int st_n[kStack], st_start[kStack], st_state[kStack];
  int n_leaves;
};

// numpy 2.x complex64 absolute (loops_unary_complex): an infinite part wins, then NaN, then L * sqrt(fma(r, r, 1))
__device__ inline float np_cabs(float re, float im) {
  const float ar = fabsf(re), ai = fabsf(im);
  if (isinf(ar) || isinf(ai)) return INFINITY;
  if (isnan(ar) || isnan(ai)) return NAN;
  const float big = fmaxf(ar, ai), small = fminf(ar, ai);
  const float r = big > 0.0f ? small / big : 0.0f;
  return big * sqrtf(__builtin_fmaf(r, r, 1.0f));
}

// numpy's pairwise_sum over one leaf (n <= 128) of values f(start .. start + n - 1)
template <typename T, class F>
__device__ T leaf_sum(int start, int n, F f) {
  if (n < 8) {
    T res = T(-0.0);
    for (int i = 0; i < n; ++i) res = res + f(start + i);
    return res;
  }
  T r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = f(start + k);
  int i = 8;
  const int lim = n - n % 8;
  for (; i < lim; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = r[k] + f(start + i + k);
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + f(start + i);
  return res;
}

// numpy's recursion over n elements, one thread: EVAL = false lists the leaves in order, EVAL = true combines their sums
template <typename T, bool EVAL>
__device__ T walk_tree(int n, Walk& w, const T* leafsum, T* st_val) {
  int sp = 0, li = 0;
  w.st_n[0] = n;
  w.st_start[0] = 0;
  w.st_state[0] = 0;
  T ret = T(0);
  for (;;) {
    const int m = w.st_n[sp];
    const int state = w.st_state[sp];
    int m2 = m / 2;
    m2 -= m2 % 8;
    if (state == 0 && m > 128) {           // descend into the left half
      w.st_state[sp] = 1;
      w.st_n[sp + 1] = m2;
      w.st_start[sp + 1] = w.st_start[sp];
      w.st_state[sp + 1] = 0;
      ++sp;
      continue;
    }
    if (state == 0) {                      // a leaf
      if (EVAL) {
        ret = leafsum[li];
      } else {
        w.lstart[li] = w.st_start[sp];
        w.lsize[li] = m;
      }
      ++li;
    } else if (state == 1) {               // left half done: keep it, descend into the right half
      if (EVAL) st_val[sp] = ret;
      w.st_state[sp] = 2;
      w.st_n[sp + 1] = m - m2;
      w.st_start[sp + 1] = w.st_start[sp] + m2;
      w.st_state[sp + 1] = 0;
      ++sp;
      continue;
    } else {                               // both halves done
      if (EVAL) ret = st_val[sp] + ret;
    }
    if (sp == 0) break;
    --sp;
  }
  if (!EVAL) w.n_leaves = li;
  return ret;
}

// pairwise sum of a block of nb values f(0 .. nb - 1), the whole workgroup; thread 0 returns it.  Every thread calls.
template <typename T, class F>
__device__ T block_sum_partial(int nb, F f, Walk& w, T* leafsum, T* st_val) {
  const int tid = threadIdx.x;
  if (tid == 0) walk_tree<T, false>(nb, w, leafsum, st_val);
  __syncthreads();
  if (tid < w.n_leaves) leafsum[tid] = leaf_sum<T>(w.lstart[tid], w.lsize[tid], f);
  __syncthreads();
  T total = T(0);
  if (tid == 0) total = walk_tree<T, true>(nb, w, leafsum, st_val);
  return total;
}

// a full block: chains[512] hold the eight accumulators of the 64 leaves; wave 0 forms the leaves and the tree
template <typename T>
__device__ T block_sum_full(const T* chains) {
  const int tid = threadIdx.x;
  T x = T(0);
  if (tid < 64) {
    const T* r = chains + 8 * tid;
    x = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int st = 1; st < 64; st <<= 1) {
      const T y = __shfl_down(x, st, 64);
      if ((tid & (2 * st - 1)) == 0) x = x + y;
    }
  }
  return x;
}

__global__ __launch_bounds__(kThreads) void cst_power_kernel(CstLaunch a, int nblk) {
  __shared__ float lut[256];
  __shared__ float chains[2 * kThreads];
  __shared__ float leafsum[kMaxLeaves];
  __shared__ float st_val[kStack];
  __shared__ Walk w;
  const int tid = threadIdx.x;
  const int seg = blockIdx.x / nblk, b = blockIdx.x % nblk;
  fill_lut(a.fmt, lut);
  __syncthreads();
  const long long base = seg * a.hop + (long long)b * kCstBlock;
  const long long rest = a.seg_len - (long long)b * kCstBlock;
  const int nb = rest < kCstBlock ? int(rest) : kCstBlock;
  auto val = [&](int j) -> float {
    const float2 x = unpack_iq(a.fmt, a.in, base + j, lut);
    const float re = x.x, im = x.y;
    const float m = np_cabs(re, im);
    return m * m;
  };
  float total;
  if (nb == kCstBlock) {
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int c = tid + kThreads * h, L = c >> 3, k = c & 7;
      float s = 0.0f;
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {
        const float v = val(128 * L + k + 8 * j);
        s = j == 0 ? v : s + v;
      }
      chains[c] = s;
    }
    __syncthreads();
    total = block_sum_full<float>(chains);
  } else {
    total = block_sum_partial<float>(nb, val, w, leafsum, st_val);
  }
  if (tid == 0) a.bs_pow[seg * nblk + b] = total;
  if (a.counts) {                  // the segment's histogram starts from zero: every block clears its share
    const long long nbin2 = (long long)a.bins * a.bins;
    unsigned* out = a.counts + seg * nbin2;
    for (long long k = b * nbin2 / nblk + tid; k < (b + 1) * nbin2 / nblk; k += kThreads) out[k] = 0u;
  }
}

// aggregate equal bins of the wave (a clean capture puts most samples in a few bins), then one LDS add per lane left.
// Every lane of the wave calls.  Two 16-bit counts per word: a block adds at most 8192 to a bin.
__device__ inline void hist_add(unsigned* hist, int key) {
  bool pending = key >= 0;
  for (;;) {
    const unsigned long long m = __ballot(pending);
    if (m == 0ull) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const int lk = __shfl(key, lead);
    const bool same = pending && key == lk;
    const int cnt = __popcll(__ballot(same));
    if (int(__lane_id()) == lead) atomicAdd(&hist[lk >> 1], unsigned(cnt) << ((lk & 1) * 16));
    if (same) pending = false;
    if (cnt < 4) break;          // a spread wave: the rest go one by one
  }
  if (pending) atomicAdd(&hist[key >> 1], 1u << ((key & 1) * 16));
}

// np.searchsorted(edges, v, 'right') - 1 with the last edge in the last bin; -1 outside [-r, r] and for NaN
__device__ inline int bin_of(float v, const double* edges, int bins, float lo, float inv_w) {
  const double d = double(v);
  if (!(d >= edges[0] && d <= edges[bins])) return -1;
  int k = int((v - lo) * inv_w);
  k = k < 0 ? 0 : (k > bins - 1 ? bins - 1 : k);
  while (k > 0 && d < edges[k]) --k;
  while (k < bins - 1 && d >= edges[k + 1]) ++k;
  return k;
}

// MODE 0: no table (no EVM), 1: grid table (per-axis minima), 2: brute force over the points
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void cst_symbol_kernel(CstLaunch a, int nblk) {
  __shared__ unsigned hist[kCstMaxBins * kCstMaxBins / 2];
  __shared__ double edges[kCstMaxBins + 1];
  __shared__ float lut[256];
  __shared__ T chains[2 * kThreads];
  __shared__ T leafsum[kMaxLeaves];
  __shared__ T st_val[kStack];
  __shared__ Walk w;
  __shared__ float sh_scl;
  __shared__ int sh_norm;
  const int tid = threadIdx.x;
  const int seg = blockIdx.x / nblk, b = blockIdx.x % nblk;
  const int bins = a.bins, nbin2 = a.bins * a.bins, hwords = (nbin2 + 1) / 2;
  const bool do_hist = a.counts != nullptr;
  fill_lut(a.fmt, lut);
  if (do_hist) {
    for (int k = tid; k <= bins; k += kThreads) {
      const double lo = -a.range;
      edges[k] = k == bins ? a.range : double(k) * a.step + lo;   // np.linspace: k * step + start, last = stop
    }
    for (int k = tid; k < hwords; k += kThreads) hist[k] = 0u;
  }
  if (tid == 0) {
    float acc = 0.0f;
    for (int k = 0; k < nblk; ++k) acc = acc + a.bs_pow[seg * nblk + k];
    const float mean = float(double(acc) / double(a.seg_len));
    const float rms = sqrtf(mean);
    sh_norm = rms > 1e-10f;
    sh_scl = 1.0f / rms;
    if (b == 0) a.rms[seg] = rms;
  }
  __syncthreads();
  const bool norm = sh_norm != 0;
  const float scl = sh_scl;
  const float lo_f = float(-a.range), inv_w = float(double(bins) / (2.0 * a.range));
  const long long base = seg * a.hop + (long long)b * kCstBlock;
  const long long rest = a.seg_len - (long long)b * kCstBlock;
  const int nb = rest < kCstBlock ? int(rest) : kCstBlock;
  const long long tail0 = a.seg_len - a.n_tail;   // segment index of the first tail point
  const bool do_tail = a.tail != nullptr && seg == 0 && (long long)b * kCstBlock + nb > tail0;

  auto sample = [&](int j, float& i, float& q) {
    const float2 x = unpack_iq(a.fmt, a.in, base + j, lut);
    const float re = x.x, im = x.y;
    if (norm) {                      // numpy complex division by (rms + 0j): (re + im * 0) * (1 / rms)
      i = (re + im * 0.0f) * scl;
      q = (im - re * 0.0f) * scl;
    } else {
      i = re;
      q = im;
    }
  };
  auto side = [&](int j, float i, float q, bool valid) {   // histogram and scatter tail; every lane of the wave calls
    if (do_tail && valid) {
      const long long g = (long long)b * kCstBlock + j - tail0;
      if (g >= 0) {
        a.tail[g] = i;
        a.tail[a.n_tail + g] = q;
      }
    }
    if (do_hist) {
      int key = -1;
      if (valid) {
        const int bi = bin_of(i, edges, bins, lo_f, inv_w);
        const int bq = bin_of(q, edges, bins, lo_f, inv_w);
        if (bi >= 0 && bq >= 0) key = bq * bins + bi;     // image layout: [q_bin][i_bin]
      }
      hist_add(hist, key);
    }
  };
  auto dist = [&](float i, float q) -> T {
    const T* tab = static_cast<const T*>(a.tab.dev);
    const T ti = T(i), tq = T(q);
    T best;
    if (MODE == 1) {
      T bx = T(INFINITY), by = T(INFINITY);
      for (int k = 0; k < a.tab.nx; ++k) {
        const T d = ti - tab[k];
        bx = fmin(bx, d * d);
      }
      for (int k = 0; k < a.tab.ny; ++k) {
        const T d = tq - tab[kCstMaxPoints + k];
        by = fmin(by, d * d);
      }
      best = bx + by;
    } else {
      best = T(INFINITY);
      for (int k = 0; k < a.tab.n_points; ++k) {
        const T dx = ti - tab[k], dy = tq - tab[kCstMaxPoints + k];
        best = fmin(best, dx * dx + dy * dy);
      }
    }
    return (isnan(i) || isnan(q)) ? T(NAN) : best;       // np.min propagates NaN
  };

  if (MODE == 0 || nb != kCstBlock) {
    if (do_hist || do_tail) {
      for (int j0 = 0; j0 < nb; j0 += kThreads) {
        const int j = j0 + tid;
        const bool valid = j < nb;
        float i = 0.0f, q = 0.0f;
        if (valid) sample(j, i, q);
        side(j, i, q, valid);
      }
    }
    if (MODE != 0) {
      auto val = [&](int j) -> T {
        float i, q;
        sample(j, i, q);
        return dist(i, q);
      };
      const T total = block_sum_partial<T>(nb, val, w, leafsum, st_val);
      if (tid == 0) static_cast<T*>(a.bs_evm)[seg * nblk + b] = total;
    }
  } else {
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int c = tid + kThreads * h, L = c >> 3, k = c & 7;
      T s = T(0);
#pragma unroll 2
      for (int jj = 0; jj < 16; ++jj) {
        const int j = 128 * L + k + 8 * jj;
        float i, q;
        sample(j, i, q);
        side(j, i, q, true);
        const T v = dist(i, q);
        s = jj == 0 ? v : s + v;
      }
      chains[c] = s;
    }
    __syncthreads();
    const T total = block_sum_full<T>(chains);
    if (tid == 0) static_cast<T*>(a.bs_evm)[seg * nblk + b] = total;
  }
  if (do_hist) {
    __syncthreads();
    unsigned* out = a.counts + (long long)seg * nbin2;
    for (int k = tid; k < hwords; k += kThreads) {
      const unsigned v = hist[k];
      if (v & 0xffffu) atomicAdd(&out[2 * k], v & 0xffffu);
      if ((v >> 16) && 2 * k + 1 < nbin2) atomicAdd(&out[2 * k + 1], v >> 16);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cst_evm_kernel(CstLaunch a, int nblk) {
  const int seg = blockIdx.x * kThreads + threadIdx.x;
  if (seg >= a.n_seg) return;
  if (a.tab.n_points == 0) {
    a.evm[seg] = NAN;
    return;
  }
  const T* bs = static_cast<const T*>(a.bs_evm) + (long long)seg * nblk;
  T acc = T(0);
  for (int k = 0; k < nblk; ++k) acc = acc + bs[k];
  if (sizeof(T) == 4) {
    const float mean = float(double(acc) / double(a.seg_len));
    a.evm[seg] = double(sqrtf(mean));
  } else {
    const double mean = double(acc) / double(a.seg_len);
    a.evm[seg] = sqrt(mean);
  }
}

template <typename T>
hipError_t launch_symbol(const CstLaunch& a, int nblk, hipStream_t s) {
  const dim3 grid(unsigned(nblk) * unsigned(a.n_seg));
  if (a.tab.n_points == 0)
    hipLaunchKernelGGL((cst_symbol_kernel<float, 0>), grid, dim3(kThreads), 0, s, a, nblk);
  else if (a.tab.separable)
    hipLaunchKernelGGL((cst_symbol_kernel<T, 1>), grid, dim3(kThreads), 0, s, a, nblk);
  else
    hipLaunchKernelGGL((cst_symbol_kernel<T, 2>), grid, dim3(kThreads), 0, s, a, nblk);
  hipLaunchKernelGGL((cst_evm_kernel<T>), dim3((a.n_seg + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a, nblk);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_constellation(const CstLaunch& a, hipStream_t s) {
  if (a.n_seg <= 0 || a.seg_len <= 0) return hipSuccess;
  const int nblk = int((a.seg_len + kCstBlock - 1) / kCstBlock);
  hipLaunchKernelGGL(cst_power_kernel, dim3(unsigned(nblk) * unsigned(a.n_seg)), dim3(kThreads), 0, s, a, nblk);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return a.tab.is_f64 ? launch_symbol<double>(a, nblk, s) : launch_symbol<float>(a, nblk, s);
}

}  // namespace tdsa
