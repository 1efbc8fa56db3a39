// tdsa_detect.hip - signal detection on dB rows that sit in device memory (the contract is
// tests/detect_contract.py).  One workgroup of 256 threads takes a row at a time, staged once into LDS:
//   floor    the rank-th smallest value of row[lo .. hi]: a radix selection over order-preserving keys, four 8-bit
//            digits from the top, one LDS histogram per digit
//   mask     row[i] > floor + margin as 64-bit ballot words, one word per thread from then on; the set bits also go
//            to the occupancy counts (integer atomics)
//   runs     scans over the words give every thread the last set bin before its word and the first after it, so it
//            marks the starts and stops inside its word; a third scan finds the stop of a run that leaves the word, a
//            fourth numbers the runs that are wide enough.  Only the first S are written down (LDS, then records).
//   measure  one wave per recorded run: peak, x-dB edges, power and first moment.  Lane l adds bins start + l,
//            start + l + 64, ... in order and the 64 partial sums meet in one butterfly, so the sums are a function of
//            (start, stop) and the bins alone.
// No floating-point atomics; nothing is indexed by a run number beyond S.
#include "tdsa_detect.hpp"

#include "tdsa_rows_align.hpp"

namespace tdsa {
namespace {

constexpr int kT = kDetThreads;
constexpr int kBig = 0x7fffffff;

// float32 -> a key that sorts as np.sort does: negatives below non-negatives, every NaN last (+0 and -0 differ)
__device__ __forceinline__ unsigned det_key(float v) {
  const unsigned b = __float_as_uint(v);
  if (v != v) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float det_unkey(unsigned k) {
  if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct OpAdd {
  static __device__ __forceinline__ int id() { return 0; }
  static __device__ __forceinline__ int f(int a, int b) { return a + b; }
};
struct OpMax {
  static __device__ __forceinline__ int id() { return -1; }
  static __device__ __forceinline__ int f(int a, int b) { return a > b ? a : b; }
};
struct OpMin {
  static __device__ __forceinline__ int id() { return kBig; }
  static __device__ __forceinline__ int f(int a, int b) { return a < b ? a : b; }
};

// exclusive scan over the workgroup's 256 threads, from thread 0 up (FWD) or from thread 255 down; *total: all of them
template <class Op, bool FWD>
__device__ __forceinline__ int block_scan_excl(int v, int* s_tmp, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = FWD ? __shfl_up(inc, d) : __shfl_down(inc, d);
    if (FWD ? lane >= d : lane + d < 64) inc = Op::f(inc, o);
  }
  __syncthreads();                                   // the scratch's previous readers are done
  if (lane == (FWD ? 63 : 0)) s_tmp[w] = inc;
  __syncthreads();
  int ex = FWD ? __shfl_up(inc, 1) : __shfl_down(inc, 1);
  if (lane == (FWD ? 0 : 63)) ex = Op::id();
  int pre = Op::id(), tot = Op::id();
#pragma unroll
  for (int k = 0; k < kT / 64; ++k) {
    const int t = s_tmp[k];
    tot = Op::f(tot, t);
    if (FWD ? k < w : k > w) pre = Op::f(pre, t);
  }
  if (total) *total = tot;
  return Op::f(pre, ex);
}

template <bool VEC>
__global__ void __launch_bounds__(kT) detect_kernel(DetLaunch a) {
  extern __shared__ __attribute__((aligned(16))) float row[];     // [n]
  __shared__ unsigned long long s_mask[kDetWords], s_stop[kDetWords];
  __shared__ unsigned s_hist[256];
  __shared__ int2 s_run[kDetMaxSignals];
  __shared__ int s_tmp[kT / 64];
  __shared__ unsigned s_sel[2];                      // the selection's key prefix and the rank within it
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = a.n, lo = a.lo, hi = a.hi, n_eff = hi - lo + 1, S = a.S;

  for (size_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
    const float* src = a.rows + r * size_t(n);
    if (VEC) {
      typedef float f4 __attribute__((ext_vector_type(4)));
      const f4* src4 = reinterpret_cast<const f4*>(src);
      for (int j = tid; j < n / 4; j += kT) reinterpret_cast<f4*>(row)[j] = __builtin_nontemporal_load(src4 + j);   // read once
    } else {
      for (int i = tid; i < n; i += kT) row[i] = src[i];
    }
    if (tid == 0) {
      s_sel[0] = 0u;
      s_sel[1] = unsigned(a.rank);
    }

    // ---- floor: the key of rank `rank` among row[lo .. hi], a digit per pass
    for (int pass = 0; pass < 4; ++pass) {
      s_hist[tid] = 0u;
      __syncthreads();
      const unsigned prefix = s_sel[0], rank = s_sel[1];
      const int shift = 24 - 8 * pass;
      for (int base = 0; base < n_eff; base += kT) {
        const int i = base + tid;
        bool act = false;
        unsigned digit = 0u;
        if (i < n_eff) {
          const unsigned key = det_key(row[lo + i]);
          act = pass == 0 || (key >> (shift + 8)) == prefix;
          digit = (key >> shift) & 255u;
        }
        // dB rows share their top digits: up to two of a wave's digits are counted by one lane each, the rest singly
        for (int round = 0; round < 2; ++round) {
          const unsigned long long am = __ballot(act);
          if (!am) break;
          const int leader = __ffsll((long long)am) - 1;
          const unsigned d0 = unsigned(__shfl(int(digit), leader));
          const bool same = act && digit == d0;
          const unsigned long long sm = __ballot(same);
          if (lane == leader) atomicAdd(&s_hist[d0], unsigned(__popcll(sm)));
          act = act && !same;
        }
        if (act) atomicAdd(&s_hist[digit], 1u);
      }
      __syncthreads();
      const unsigned c = s_hist[tid];
      const unsigned ex = unsigned(block_scan_excl<OpAdd, true>(int(c), s_tmp, nullptr));
      if (rank >= ex && rank < ex + c) {             // exactly one thread: the prefix's keys are more than `rank`
        s_sel[0] = (prefix << 8) | unsigned(tid);
        s_sel[1] = rank - ex;
      }
      __syncthreads();
    }
    const float floor_v = det_unkey(s_sel[0]);
    const float thr = floor_v + a.margin;            // a NaN floor makes a NaN threshold, which nothing exceeds
    const int flags = floor_v != floor_v ? kDetFlagNanFloor : 0;

    // ---- mask words, n_over, occupancy
    int over = 0;
    for (int wd = w; wd < kDetWords; wd += kT / 64) {   // all 256 words: those beyond the row are zero
      const int i = 64 * wd + lane;
      bool p = false;
      if (i >= lo && i <= hi) p = row[i] > thr;
      const unsigned long long b = __ballot(p);
      if (lane == 0) {
        s_mask[wd] = b;
        over += __popcll(b);
      }
      if (p) atomicAdd(&a.occ[i], 1u);
    }
    int n_over = 0;
    (void)block_scan_excl<OpAdd, true>(over, s_tmp, &n_over);     // (its barriers also publish s_mask)

    // ---- runs: thread t owns bins 64 t .. 64 t + 63
    const unsigned long long m = s_mask[tid];
    const int last = m ? 64 * tid + 63 - __clzll((long long)m) : -1;
    const int first = m ? 64 * tid + __ffsll((long long)m) - 1 : kBig;
    const int prev_last = block_scan_excl<OpMax, true>(last, s_tmp, nullptr);
    const int next_first = block_scan_excl<OpMin, false>(first, s_tmp, nullptr);
    const int G = a.max_gap + 1;                     // two set bins further apart than this are in different runs
    unsigned long long st = 0ull, sp = 0ull;
    {
      int prev = prev_last;
      unsigned long long bits = m;
      while (bits) {
        const int j = __ffsll((long long)bits) - 1;
        const int b = 64 * tid + j;
        bits &= bits - 1;
        const int nxt = bits ? 64 * tid + __ffsll((long long)bits) - 1 : next_first;
        if (prev < 0 || b - prev > G) st |= 1ull << j;
        if (nxt == kBig || nxt - b > G) sp |= 1ull << j;
        prev = b;
      }
    }
    s_stop[tid] = sp;
    const int next_stop_word = block_scan_excl<OpMin, false>(sp ? tid : kBig, s_tmp, nullptr);   // (publishes s_stop)
    // the stop of the run that starts at bit j of this word: the first stop at or after it
    auto stop_of = [&](int j) {
      const unsigned long long own = sp & (~0ull << j);
      if (own) return 64 * tid + __ffsll((long long)own) - 1;
      const int nw = next_stop_word & (kDetWords - 1);            // (every start has a stop: the mask only bounds the index)
      return 64 * nw + __ffsll((long long)s_stop[nw]) - 1;
    };
    unsigned long long keep = 0ull;
    for (unsigned long long bits = st; bits; bits &= bits - 1) {
      const int j = __ffsll((long long)bits) - 1;
      if (stop_of(j) - (64 * tid + j) + 1 >= a.min_width) keep |= 1ull << j;
    }
    int n_found = 0;
    int idx = block_scan_excl<OpAdd, true>(__popcll(keep), s_tmp, &n_found);
    for (unsigned long long bits = keep; bits && idx < S; bits &= bits - 1, ++idx) {
      const int j = __ffsll((long long)bits) - 1;
      s_run[idx] = make_int2(64 * tid + j, stop_of(j));
    }
    __syncthreads();

    // ---- records
    const int n_rec = n_found < S ? n_found : S;
    DetSignal* out = a.sig_rec + r * size_t(S);
    for (int k = w; k < n_rec; k += kT / 64) {
      const int2 run = s_run[k];
      float bv = -INFINITY;                          // the run's first bin is above the threshold, so above -inf
      int bi = kBig;
      double pw = 0.0, mo = 0.0;
      for (int i = run.x + lane; i <= run.y; i += 64) {
        const float v = row[i];
        if (v > bv) {
          bv = v;
          bi = i;
        }
        if (v == v) {
          const double p = (double)exp10f(v / 10.0f);   // rows_stats_kernel's expression
          pw += p;
          mo += double(i - run.x) * p;
        }
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
        pw += __shfl_xor(pw, d);
        mo += __shfl_xor(mo, d);
      }
      const float edge = bv - a.xdb;
      int x_lo = kBig, x_hi = -1;
      for (int i = run.x + lane; i <= run.y; i += 64) {
        if (row[i] >= edge) {
          x_lo = x_lo < i ? x_lo : i;
          x_hi = i;
        }
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        x_lo = OpMin::f(x_lo, __shfl_xor(x_lo, d));
        x_hi = OpMax::f(x_hi, __shfl_xor(x_hi, d));
      }
      if (lane == 0) {
        DetSignal g;
        g.start = run.x;
        g.stop = run.y;
        g.peak_bin = bi;
        g.x_lo = x_lo;
        g.x_hi = x_hi;
        g.peak_db = bv;
        g.power = pw;
        g.moment = mo;
        out[k] = g;
      }
    }
    for (int k = n_rec + tid; k < S; k += kT) {
      DetSignal g;
      g.start = g.stop = g.peak_bin = g.x_lo = g.x_hi = -1;
      g.peak_db = __uint_as_float(0x7fc00000u);
      g.power = g.moment = 0.0;
      out[k] = g;
    }
    if (tid == 0) {
      DetRow q;
      q.floor = floor_v;
      q.thr = thr;
      q.n_found = n_found;
      q.n_over = n_over;
      q.flags = flags;
      q.reserved[0] = q.reserved[1] = q.reserved[2] = 0;
      a.row_rec[r] = q;
    }
    __syncthreads();                                 // the row and the runs are rewritten by the next row
  }
}

}  // namespace

hipError_t detect_prepare() {
  const int bytes = kDetMaxLdsBytes - kDetStaticLdsBytes;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&detect_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&detect_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}

hipError_t launch_detect(const DetLaunch& a, hipStream_t s) {
  if (a.n_rows < 1) return hipSuccess;
  if (a.n < 1 || a.n > kDetMaxBins || a.lo < 0 || a.hi >= a.n || a.lo > a.hi || a.rank < 0 || a.rank > a.hi - a.lo ||
      a.S < 1 || a.S > kDetMaxSignals || a.max_gap < 0 || a.max_gap > kDetMaxBins)
    return hipErrorInvalidValue;
  const size_t lds = (size_t(a.n) * sizeof(float) + 15) & ~size_t(15);
  const unsigned grid = unsigned(a.n_rows < size_t(kDetMaxGrid) ? a.n_rows : size_t(kDetMaxGrid));
  if (rows_take_vec16(a.rows, a.n))
    hipLaunchKernelGGL(detect_kernel<true>, dim3(grid), dim3(kT), lds, s, a);
  else
    hipLaunchKernelGGL(detect_kernel<false>, dim3(grid), dim3(kT), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
