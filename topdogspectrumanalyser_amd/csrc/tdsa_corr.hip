// tdsa_corr.hip - correlation search of IQ streams: where a known sequence starts (the contract is
// the comment block of tdsa_corr_* in include/tdsa_hip.h and tests/corr_contract.py).
//
//   window n   c1 = sum_{k < H} x[n+k] conj(r[k]), c2 = the same over k >= H, e = sum |x[n+k]|^2, m = |c1 + c2|^2 / (E_r e)
//   order      every sum is one chain of fmaf from 0 in the order of k.  A component of c1 or c2 takes two per k:
//              re: x_re r_re, then x_im r_im;  im: x_im r_re, then -(x_re r_im).  e is two chains, of x_re^2 and of
//              x_im^2, added once at the end.  Every window sees this same sequence of operations on the same values,
//              wherever it lies in a tile, a launch or a call: the bits of m, e, c1, c2 are a function of the samples.
//   ring       m, e, c1, c2 of window n of stream c live at entry n & ring_mask of the stream's ring: the scratch of the
//              match passes, the carry between calls and the metric trace are this one region.
//
// Five plain launches on one stream per launch cut; no workgroup ever waits for another:
//   corr_kernel        one workgroup per tile of T = 256 R windows.  It stages T + L - 1 unpacked samples in LDS as float2 -
//                      those before the launch's first from the handle's history - and each thread slides R consecutive
//                      windows over them: per k one LDS read of a new sample, r[k], and 6 R fused multiply-adds.  LDS
//                      entry i lies at i + i / R, so that the threads' reads, R samples apart, fall on different banks.
//                      Two instantiations ship, the faster at either end: up to kCorrShortRef samples of reference R = 4,
//                      r[k] through uniform scalar loads and the multiply-adds as v_pk_fma_f32 - there the pass is
//                      staging and ring writes, and fewer instructions win; above, R = 8, the reference staged in LDS
//                      too - a multiply-add with a scalar operand issues at half the rate - and v_fma_f32.  The other
//                      variants are what tools/corrbench.py times against them.  All give the same bits.
//   corr_bmax_kernel   the largest m, as bits, of every block of 256 windows (on multiples of 256) that a decision of
//                      this launch can reach: the second level of the two-level maximum.
//   corr_count_kernel  one thread per window to decide.  A window at or above the threshold walks to the left and to the
//                      right: windows one by one to the end of its block, whole blocks by their maxima, windows one by
//                      one inside the last block; it stops at the first window that beats it.  At most 2 (255 + W / 256
//                      + 255) reads, and a handful for all but the peaks.  It leaves a bit per window and a count per block.
//   corr_scan_kernel   one workgroup per stream: the blocks' counts become the slots of their first matches; it also
//                      writes the stream's summary and the L - 1 samples of history for the next launch, into the slot
//                      that this launch's correlate pass did not read.
//   corr_emit_kernel   writes the records of the matches whose ordinal is below the capacity.
// m is never negative and a NaN (inf / inf, 0 / 0) is stored as 0x7fc00000, so the bits of m order as its values do with a
// NaN above +inf: the comparisons of the match rule are integer comparisons of the bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_corr.hpp"
#include "tdsa_unpack.hpp"
#include "tdsa_wave.hpp"

namespace tdsa {
namespace {

static_assert(kCorrThreads == 256 && kCorrBlock == 256, "the kernels are written for 256 threads and blocks of 256 windows");
static_assert((long long)kCorrMaxLaunchTiles * kCorrTile < (1ll << 31), "a launch's sample indices fit an int");

typedef float v2f __attribute__((ext_vector_type(2)));

template <int R, bool RLDS>
struct CorrLds {
  static constexpr int kStaged = kCorrThreads * R + kCorrMaxRef + R;     // T + L - 1 samples, and the R a thread loads ahead
  float2 x[kStaged + kStaged / R + 1];
  float2 c1[R > 8 ? kCorrThreads * R : 1];                                // the widest variant parks c1 here over the second half
  float2 ref[RLDS ? kCorrMaxRef : 1];                                     // the reference, for the variants that read it from LDS
  float lut[256];
  int n_bad;
};
static_assert(sizeof(CorrLds<kCorrWindowsPerThread, true>) <= kCorrLdsBudget, "the header states the LDS budget");
static_assert(sizeof(CorrLds<16, false>) <= kCorrLdsBudgetWide, "the header states the LDS budget of the widest variant");

template <int R>
__device__ __forceinline__ int phys(int i) {
  return i + i / R;
}

// the R windows of a thread over r[k0 .. k1 - 1]: acc[j] += x[n0 + j + k] conj(r[k]), ea / eb += the squares.  xs[] holds
// x[n0 + k + j] in slot (j + k - k0) % R: a step reads one new sample into the slot it has just finished with.
template <int R, bool PK>
__device__ __forceinline__ void slide(const float2* __restrict__ lx, const float2* __restrict__ ref, int n0, int k0, int k1,
                                      v2f (&acc)[R], v2f (&en)[R]) {
  float2 xs[R];
#pragma unroll
  for (int j = 0; j < R; ++j) xs[j] = lx[phys<R>(n0 + k0 + j)];
  for (int kb = k0; kb < k1; kb += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int k = kb + u;
      if (k < k1) {                                  // the same for every thread
        const float2 r = ref[k];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const float2 x = xs[(j + u) % R];
          if constexpr (PK) {
            acc[j] = __builtin_elementwise_fma(v2f{x.x, x.y}, v2f{r.x, r.x}, acc[j]);
            acc[j] = __builtin_elementwise_fma(v2f{x.y, x.x}, v2f{r.y, -r.y}, acc[j]);
            en[j] = __builtin_elementwise_fma(v2f{x.x, x.y}, v2f{x.x, x.y}, en[j]);
          } else {
            acc[j].x = fmaf(x.x, r.x, acc[j].x);
            acc[j].x = fmaf(x.y, r.y, acc[j].x);
            acc[j].y = fmaf(x.y, r.x, acc[j].y);
            acc[j].y = fmaf(x.x, -r.y, acc[j].y);
            en[j].x = fmaf(x.x, x.x, en[j].x);
            en[j].y = fmaf(x.y, x.y, en[j].y);
          }
        }
        xs[u] = lx[phys<R>(n0 + k + R)];             // x[n0 + (k + 1) + (R - 1)]: the newest sample of the next step
      }
    }
  }
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <int R, bool PK, bool RLDS>
__global__ __launch_bounds__(kCorrThreads) void corr_kernel(CorrLaunch a) {
  __shared__ CorrLds<R, RLDS> l;
  constexpr int T = kCorrThreads * R;
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  fill_lut(a.fmt, l.lut);
  if (tid == 0) l.n_bad = 0;
  __syncthreads();
  const size_t unit = a.fmt == 2 ? 8 : 2;
  const char* sb = static_cast<const char*>(a.in) + size_t(c) * a.in_stride * unit;
  const float2* hist = a.hist + (size_t(a.parity) * size_t(a.C) + size_t(c)) * kCorrMaxRef;
  const long long g = a.w0 + (long long)blockIdx.x * T;   // the tile's first window = the index of its first sample
  const int off = int(g - a.s0);                          // ... in the launch: -(L - 1) at the least
  const int L = a.L, H = L / 2;
  const int staged = T + L - 1 + R;
  if constexpr (RLDS) {
    for (int i = tid; i < L; i += kCorrThreads) l.ref[i] = a.ref[i];
  }
  const float2* ref = RLDS ? l.ref : a.ref;
  for (int i = tid; i < staged; i += kCorrThreads) {
    const int rel = off + i;
    float2 v = make_float2(0.0f, 0.0f);
    if (rel >= 0) {
      if (rel < a.n) v = unpack_iq(a.fmt, sb, rel, l.lut);
    } else if (rel + L - 1 >= 0) {
      v = hist[rel + L - 1];
    }
    l.x[phys<R>(i)] = v;
  }
  __syncthreads();

  const int n0 = tid * R;
  const long long left = a.w1 - g;                        // windows of the tile, T at the most
  const int nwin = left < T ? int(left) : T;
  int bad = 0;
  if (n0 < nwin) {
    v2f c1[R], c2[R], en[R];
#pragma unroll
    for (int j = 0; j < R; ++j) c1[j] = v2f{0.0f, 0.0f}, c2[j] = v2f{0.0f, 0.0f}, en[j] = v2f{0.0f, 0.0f};
    slide<R, PK>(l.x, ref, n0, 0, H, c1, en);
    if constexpr (R > 8) {
#pragma unroll
      for (int j = 0; j < R; ++j) l.c1[j * kCorrThreads + tid] = make_float2(c1[j].x, c1[j].y);
    }
    slide<R, PK>(l.x, ref, n0, H, L, c2, en);
    if constexpr (R > 8) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float2 v = l.c1[j * kCorrThreads + tid];
        c1[j] = v2f{v.x, v.y};
      }
    }
    const size_t ring = size_t(a.ring_mask) + 1;
    float* rm = a.ring_m + size_t(c) * ring;
    float* re = a.ring_e + size_t(c) * ring;
    float4* rc = a.ring_c + size_t(c) * ring;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (n0 + j < nwin) {
        const float e = en[j].x + en[j].y;
        const float cre = c1[j].x + c2[j].x, cim = c1[j].y + c2[j].y;
        const bool ok = finite_f(c1[j].x) && finite_f(c1[j].y) && finite_f(c2[j].x) && finite_f(c2[j].y) && finite_f(e) && e != 0.0f;
        float m = 0.0f;
        if (ok) {
          const float p = cre * cre + cim * cim;
          const float d = a.e_ref * e;
          m = p / d;
          if (m != m) m = __uint_as_float(0x7fc00000u);
        } else {
          ++bad;
        }
        const size_t at = size_t((unsigned long long)(g + n0 + j) & a.ring_mask);
        rm[at] = m;
        re[at] = e;
        rc[at] = make_float4(c1[j].x, c1[j].y, c2[j].x, c2[j].y);
      }
    }
  }
  if (bad) atomicAdd(&l.n_bad, bad);
  __syncthreads();
  if (tid == 0 && l.n_bad) atomicAdd(&a.sum[c].n_bad, (unsigned long long)l.n_bad);
}

// ---- the match passes ----------------------------------------------------------------------------------------------
// the bits of m[j]; 0, below every m that can match, for a window that does not exist
__device__ __forceinline__ unsigned key_at(const float* rm, unsigned mask, long long j, long long last) {
  return (j < 0 || j > last) ? 0u : __float_as_uint(rm[(unsigned long long)j & mask]);
}

// the first block a decision of the launch can reach
__device__ __forceinline__ long long first_block(const CorrLaunch& a) {
  const long long lo = a.d0 - a.W;
  return (lo > 0 ? lo : 0) >> 8;
}

struct MatchLds {
  int part[4];
};
static_assert(sizeof(MatchLds) <= kCorrMatchLdsBudget, "the header states the LDS budget");

__global__ __launch_bounds__(kCorrThreads) void corr_bmax_kernel(CorrLaunch a) {
  __shared__ MatchLds l;
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  const float* rm = a.ring_m + size_t(c) * (size_t(a.ring_mask) + 1);
  for (int b = 0; b < kCorrBlocksPerWorkgroup; ++b) {
    const unsigned blk = blockIdx.x * kCorrBlocksPerWorkgroup + b;
    if (blk >= a.n_reach) break;                          // the same for every thread
    const long long j = ((first_block(a) + blk) << 8) + tid;
    const int best = wave_max(int(key_at(rm, a.ring_mask, j, a.w1 - 1)));   // no sign bit: the bits order as ints
    if ((tid & 63) == 0) l.part[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      int v = l.part[0];
      for (int w = 1; w < 4; ++w) v = l.part[w] > v ? l.part[w] : v;
      a.bmax[size_t(c) * size_t(a.blocks) + blk] = unsigned(v);
    }
    __syncthreads();                                      // before the next block's maxima overwrite these
  }
}

__global__ __launch_bounds__(kCorrThreads) void corr_count_kernel(CorrLaunch a) {
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  const unsigned mask = a.ring_mask;
  const float* rm = a.ring_m + size_t(c) * (size_t(mask) + 1);
  const long long kb0 = first_block(a);
  const unsigned* bmax = a.bmax + size_t(c) * size_t(a.blocks);
  const long long last = a.w1 - 1;
  for (int b = 0; b < kCorrBlocksPerWorkgroup; ++b) {
    const unsigned blk = blockIdx.x * kCorrBlocksPerWorkgroup + b;
    if (blk >= a.n_decide) break;                           // the same for every thread
    const long long kb = (a.d0 >> 8) + blk;
    const long long n = (kb << 8) + tid;
    bool match = false;
    if (n >= a.d0 && n < a.d1) {
      const unsigned k = key_at(rm, mask, n, last);
      match = __uint_as_float(k) >= a.threshold;            // false for a NaN
      if (match) {
        const long long lo = n - a.W > 0 ? n - a.W : 0;
        long long j = n - 1;
        while (match && j >= lo && ((j + 1) & 255) != 0) match = key_at(rm, mask, j, last) < k, --j;
        while (match && j - 255 >= lo) match = bmax[(j >> 8) - kb0] < k, j -= 256;
        while (match && j >= lo) match = key_at(rm, mask, j, last) < k, --j;
        const long long hi = n + a.W < last ? n + a.W : last;
        j = n + 1;
        while (match && j <= hi && (j & 255) != 0) match = key_at(rm, mask, j, last) <= k, ++j;
        while (match && j + 255 <= hi) match = bmax[(j >> 8) - kb0] <= k, j += 256;
        while (match && j <= hi) match = key_at(rm, mask, j, last) <= k, ++j;
      }
    }
    const size_t at = size_t(c) * size_t(a.blocks) + size_t(kb - kb0);
    const unsigned long long bits = __ballot(match);
    if ((tid & 63) == 0) a.tile_bits[at * 4 + (tid >> 6)] = bits;
    const int total = __syncthreads_count(match);
    if (tid == 0) a.tile_cnt[at] = total;
  }
}

struct ScanLds {
  float lut[256];
  int part[4];
};
static_assert(sizeof(ScanLds) <= kCorrScanLdsBudget, "the header states the LDS budget");

__global__ __launch_bounds__(kCorrThreads) void corr_scan_kernel(CorrLaunch a) {
  __shared__ ScanLds l;
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  fill_lut(a.fmt, l.lut);
  CorrSummary* sum = a.sum + c;
  unsigned long long n_matches = sum->n_matches;       // the same in every thread
  __syncthreads();                                     // also: the table is filled
  const int tiles = a.d1 > a.d0 ? int(((a.d1 - 1) >> 8) - (a.d0 >> 8)) + 1 : 0;
  int* cnt = a.tile_cnt + size_t(c) * size_t(a.blocks) + size_t((a.d0 >> 8) - first_block(a));
  for (int t0 = 0; t0 < tiles; t0 += kCorrThreads) {
    const int t = t0 + tid;
    const int v = t < tiles ? cnt[t] : 0;
    const int inc = wave_scan_inclusive(v, [](int own, int lower) { return own + lower; });
    if ((tid & 63) == 63) l.part[tid >> 6] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int s = l.part[w];
      if (w < (tid >> 6)) before += s;
      all += s;
    }
    __syncthreads();
    const unsigned long long slot = n_matches + (unsigned long long)(before + inc - v);
    if (t < tiles) cnt[t] = slot < (unsigned long long)a.capacity ? int(slot) : a.capacity;
    n_matches += (unsigned long long)all;
  }
  if (tid == 0) {
    sum->n_total = (unsigned long long)(a.s0 + a.n);
    sum->n_windows = (unsigned long long)a.w1;
    sum->n_decided = (unsigned long long)a.d1;
    sum->n_matches = n_matches;
    sum->n_lost = n_matches > (unsigned long long)a.capacity ? n_matches - (unsigned long long)a.capacity : 0ull;
    sum->flushed = a.flush;
  }
  // the last L - 1 samples of the stream so far: of this launch, and before them of the history it began with
  if (a.n > 0) {
    const size_t unit = a.fmt == 2 ? 8 : 2;
    const char* sb = static_cast<const char*>(a.in) + size_t(c) * a.in_stride * unit;
    const float2* old = a.hist + (size_t(a.parity) * size_t(a.C) + size_t(c)) * kCorrMaxRef;
    float2* now = a.hist + (size_t(a.parity ^ 1) * size_t(a.C) + size_t(c)) * kCorrMaxRef;
    const int keep = a.L - 1;
    for (int j = tid; j < keep; j += kCorrThreads) {
      const int rel = a.n - keep + j;
      now[j] = rel >= 0 ? unpack_iq(a.fmt, sb, rel, l.lut) : old[rel + keep];
    }
  }
}

__global__ __launch_bounds__(kCorrThreads) void corr_emit_kernel(CorrLaunch a) {
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  const long long kb0 = first_block(a);
  const long long kb = (a.d0 >> 8) + blockIdx.x;
  const size_t at = size_t(c) * size_t(a.blocks) + size_t(kb - kb0);
  const int slot = a.tile_cnt[at];
  if (slot >= a.capacity) return;                        // the same word for every thread
  const int wave = tid >> 6, lane = tid & 63;
  int rank = 0;
  unsigned long long mine = 0ull;
  for (int w = 0; w < 4; ++w) {
    const unsigned long long bits = a.tile_bits[at * 4 + w];
    if (w < wave) rank += __popcll(bits);
    if (w == wave) mine = bits;
  }
  if (!((mine >> lane) & 1ull)) return;
  rank += __popcll(mine & ((1ull << lane) - 1ull));
  const long long ord = (long long)slot + rank;
  if (ord >= a.capacity) return;
  const long long n = (kb << 8) + tid;
  const size_t ring = size_t(a.ring_mask) + 1;
  const size_t e = size_t(c) * ring + size_t((unsigned long long)n & a.ring_mask);
  const float4 cc = a.ring_c[e];
  CorrRecord r;
  r.index = n;
  r.metric = a.ring_m[e];
  r.energy = a.ring_e[e];
  r.c1_re = cc.x, r.c1_im = cc.y, r.c2_re = cc.z, r.c2_im = cc.w;
  a.records[size_t(c) * size_t(a.capacity) + size_t(ord)] = r;
}

template <int R, bool PK, bool RLDS>
void launch_correlate(const CorrLaunch& a, hipStream_t s) {
  const long long tile = kCorrThreads * R;
  const unsigned gx = unsigned((a.w1 - a.w0 + tile - 1) / tile);
  hipLaunchKernelGGL((corr_kernel<R, PK, RLDS>), dim3(gx, unsigned(a.C)), dim3(kCorrThreads), 0, s, a);
}

}  // namespace

hipError_t launch_corr(const CorrLaunch& args, hipStream_t s) {
  if (args.C <= 0) return hipSuccess;
  CorrLaunch a = args;
  if ((a.passes & 1) && a.w1 > a.w0) {
    // as shipped: the faster of the measured variants at either end (profiles/corrbench.txt).  A short reference is
    // staging and ring writes, where the fewer instructions of 4 windows with packed multiply-adds win; a long one is
    // multiply-add issue, where vector operands from LDS and 8 windows do.  The bits are the same from both.
    const int variant = a.variant ? a.variant : a.L <= kCorrShortRef ? 4 : 6;
    switch (variant) {
      case 1: launch_correlate<4, false, false>(a, s); break;
      case 2: launch_correlate<8, false, false>(a, s); break;
      case 3: launch_correlate<16, false, false>(a, s); break;
      case 4: launch_correlate<4, true, false>(a, s); break;
      case 5: launch_correlate<8, true, false>(a, s); break;
      case 7: launch_correlate<8, true, true>(a, s); break;
      default: launch_correlate<kCorrWindowsPerThread, false, true>(a, s); break;   // 6
    }
  }
  const unsigned decide = a.d1 > a.d0 ? unsigned(((a.d1 - 1) >> 8) - (a.d0 >> 8)) + 1u : 0u;
  if ((a.passes & 2) && decide) {
    const long long lo = a.d0 - a.W > 0 ? a.d0 - a.W : 0;
    const long long hi = a.d1 - 1 + a.W < a.w1 - 1 ? a.d1 - 1 + a.W : a.w1 - 1;
    a.n_reach = unsigned((hi >> 8) - (lo >> 8)) + 1u;
    a.n_decide = decide;
    const unsigned per = kCorrBlocksPerWorkgroup;
    hipLaunchKernelGGL(corr_bmax_kernel, dim3((a.n_reach + per - 1) / per, unsigned(a.C)), dim3(kCorrThreads), 0, s, a);
    hipLaunchKernelGGL(corr_count_kernel, dim3((decide + per - 1) / per, unsigned(a.C)), dim3(kCorrThreads), 0, s, a);
  }
  if (a.passes & 4) hipLaunchKernelGGL(corr_scan_kernel, dim3(unsigned(a.C)), dim3(kCorrThreads), 0, s, a);
  if ((a.passes & 8) && decide) hipLaunchKernelGGL(corr_emit_kernel, dim3(decide, unsigned(a.C)), dim3(kCorrThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
