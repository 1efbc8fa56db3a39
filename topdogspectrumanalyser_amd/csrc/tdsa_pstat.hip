// tdsa_pstat.hip - statistics of the instantaneous power of IQ streams: the histogram behind CCDF / APD, the exact total
// power, the peak (the contract is the comment block of tdsa_pstat_* in include/tdsa_hip.h and
// tests/pstat_contract.py).  One pass over the samples, nothing written but the handle's state.
//
//   power   p = fl(fl(re re) + fl(im im)): two products and a sum, each rounded once.  The Makefile compiles this file
//           with -ffp-contract=off; no flush-to-zero option anywhere, a denormal p is a number like any other.
//   state   integers only: a count per class, 2048 counts keyed by the leading bits of p, per biased exponent the sum of
//           the 24-bit mantissas, the largest and the smallest bits.  Integer adds, max and min commute, so the state is
//           the same bits for any split into calls, any grid and any order of the atomics.
//
// A workgroup takes tiles of kPstatTile samples of ONE stream (grid.y) and strides over that stream's tiles.  It counts
// into LDS and merges into the handle's state once, at its end, with one atomic per LDS word that is not zero.  A
// constant envelope puts every sample of a wave in one bin and one octave:
//   histogram   one LDS add per sample, whatever the keys.  Aggregating equal keys of a wave by ballot first
//               (tdsa_constellation.hip's hist_add) and wave-private histograms were measured and are not used: the
//               pass is bound by the instructions it issues, not by LDS conflicts
//   mantissas   every thread keeps a running (exponent, 64-bit sum) pair in registers and adds it to LDS only when the
//               exponent changes: a constant envelope adds once per thread of a workgroup's whole life
//   classes     per-thread counts in registers, added to LDS at the end
// Load paths: a stream whose first sample lies on 16 bytes is read as 16-byte vectors (8 byte-pair samples, 2 complex64)
// with the tail by elements; any other stream by elements.  The choice is the stream's (in + c * in_stride), so with an
// odd stride the streams of one launch alternate.  Both give the same bits: the unpack arithmetic is tdsa_unpack.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_pstat.hpp"
#include "tdsa_unpack.hpp"

namespace tdsa {
namespace {

struct Lds {
  unsigned long long msum[kPstatExponents];
  unsigned hist[kPstatBins];
  float lut[256];
  unsigned cnt[6];               // n_nan, n_gated, n_inf, n_zero, n_under, n_over
  unsigned max_bits, min_bits;
};
static_assert(sizeof(Lds) == kPstatLdsBytes, "the header states the LDS of a workgroup");
static_assert(kPstatLdsBytes <= 40 * 1024, "four workgroups per CU at the least");
static_assert(kPstatMaxLaunchSamples % kPstatTile == 0 && kPstatMaxLaunchSamples < (1ll << 32), "32-bit LDS counts");
static_assert(kPstatTile % (8 * kPstatThreads) == 0, "a full tile is whole rounds of 16-byte vectors in both widths");

struct Acc {                     // a thread's registers
  unsigned cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  unsigned max_bits = 0u, min_bits = 0xffffffffu;
  unsigned cur_e = 0u;           // the running pair of the mantissa sums
  unsigned long long cur_sum = 0ull;
};

// one sample into its class (valid = false: a lane past the end)
__device__ __forceinline__ void classify(float re, float im, bool valid, int bin_base, float gate, Lds& l, Acc& t) {
  const float rr = re * re, ii = im * im;
  const float p = rr + ii;
  const unsigned u = __float_as_uint(p);
  int key = -1;
  if (valid) {
    if (p != p) {
      ++t.cnt[0];
    } else if (p < gate) {
      ++t.cnt[1];
    } else if (u == 0x7f800000u) {
      ++t.cnt[2];
    } else {
      t.max_bits = u > t.max_bits ? u : t.max_bits;
      if (u == 0u) {
        ++t.cnt[3];
      } else {
        t.min_bits = u < t.min_bits ? u : t.min_bits;
        const int b = int(u >> 18) - bin_base;
        if (b < 0) ++t.cnt[4];
        else if (b >= kPstatBins) ++t.cnt[5];
        else key = b;
        const unsigned e = u >> 23, f = u & 0x7fffffu;
        if (e != t.cur_e) {
          if (t.cur_sum) atomicAdd(&l.msum[t.cur_e], t.cur_sum);
          t.cur_e = e;
          t.cur_sum = 0ull;
        }
        t.cur_sum += e ? (f | 0x800000u) : f;
      }
    }
  }
  if (key >= 0) atomicAdd(&l.hist[key], 1u);
}

// the next sample of the 16 bytes w, which it consumes: 8 byte pairs (fmt 0, 1) or 2 complex64 (fmt 2), with
// tdsa_unpack.hpp's arithmetic.  The words shift down instead of being indexed, so they stay in registers.
__device__ __forceinline__ float2 vec_next(int fmt, uint4& w, const float* lut) {
  if (fmt == 2) {
    const float2 x = make_float2(__uint_as_float(w.x), __uint_as_float(w.y));
    w.x = w.z;
    w.y = w.w;
    return x;
  }
  const unsigned b0 = w.x & 0xffu, b1 = (w.x >> 8) & 0xffu;
  w.x = (w.x >> 16) | (w.y << 16);
  w.y = (w.y >> 16) | (w.z << 16);
  w.z = (w.z >> 16) | (w.w << 16);
  w.w >>= 16;
  if (fmt == 1) return make_float2(lut[b0], lut[b1]);
  return make_float2(float(int(int8_t(b0))) * 0.0078125f, float(int(int8_t(b1))) * 0.0078125f);
}

__global__ __launch_bounds__(kPstatThreads) void pstat_kernel(PstatLaunch a) {
  __shared__ Lds l;
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  for (int k = tid; k < kPstatBins; k += kPstatThreads) l.hist[k] = 0u;
  l.msum[tid] = 0ull;
  if (tid < 6) l.cnt[tid] = 0u;
  if (tid == 0) {
    l.max_bits = 0u;
    l.min_bits = 0xffffffffu;
  }
  fill_lut(a.fmt, l.lut);
  __syncthreads();

  const size_t unit = a.fmt == 2 ? 8 : 2;              // bytes per sample
  const int S = a.fmt == 2 ? 2 : 8;                    // samples per 16 bytes
  const char* base = static_cast<const char*>(a.in) + size_t(c) * a.in_stride * unit;
  const bool vec = (reinterpret_cast<uintptr_t>(base) & 15u) == 0u;
  const long long n = (long long)a.n;
  const long long tiles = (n + kPstatTile - 1) / kPstatTile;
  Acc t;

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long s0 = tile * kPstatTile;             // a tile starts on 16 bytes when its stream does
    const long long rest = n - s0;
    const int nt = rest < kPstatTile ? int(rest) : kPstatTile;
    const char* tb = base + size_t(s0) * unit;
    const int nvec = vec ? nt / S : 0;
    const uint4* vp = reinterpret_cast<const uint4*>(tb);
    uint4 cur = make_uint4(0u, 0u, 0u, 0u);
    if (tid < nvec) cur = vp[tid];
#pragma unroll 1
    for (int j0 = 0; j0 < nvec; j0 += kPstatThreads) {
      const int jn = j0 + kPstatThreads + tid;
      uint4 nxt = make_uint4(0u, 0u, 0u, 0u);           // the next round's load flies while this one is counted
      if (jn < nvec) nxt = vp[jn];
      const bool ok = j0 + tid < nvec;
#pragma unroll 1
      for (int s = 0; s < S; ++s) {
        const float2 x = vec_next(a.fmt, cur, l.lut);
        classify(x.x, x.y, ok, a.bin_base, a.gate, l, t);
      }
      cur = nxt;
    }
#pragma unroll 1
    for (int e0 = nvec * S; e0 < nt; e0 += kPstatThreads) {
      const int e = e0 + tid;
      const bool ok = e < nt;
      const float2 x = ok ? unpack_iq(a.fmt, tb, e, l.lut) : make_float2(0.0f, 0.0f);
      classify(x.x, x.y, ok, a.bin_base, a.gate, l, t);
    }
  }

  if (t.cur_sum) atomicAdd(&l.msum[t.cur_e], t.cur_sum);
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (t.cnt[k]) atomicAdd(&l.cnt[k], t.cnt[k]);
  if (t.max_bits) atomicMax(&l.max_bits, t.max_bits);
  if (t.min_bits != 0xffffffffu) atomicMin(&l.min_bits, t.min_bits);
  __syncthreads();

  // the merge: one atomic per word of the workgroup's that is not zero
  PstatRecord* rec = a.rec + c;
  unsigned long long* ghist = a.hist + size_t(c) * kPstatBins;
  for (int k = tid; k < kPstatBins; k += kPstatThreads) {
    const unsigned v = l.hist[k];
    if (v) atomicAdd(&ghist[k], (unsigned long long)v);
  }
  {
    const unsigned long long v = l.msum[tid];
    if (v) atomicAdd(&a.msum[size_t(c) * kPstatExponents + tid], v);
  }
  if (tid < 6 && l.cnt[tid]) atomicAdd(&rec->n_nan + tid, (unsigned long long)l.cnt[tid]);
  if (tid == 6 && l.max_bits) atomicMax(&rec->max_bits, l.max_bits);
  if (tid == 7 && l.min_bits != 0xffffffffu) atomicMin(&rec->min_bits, l.min_bits);
  if (tid == 8 && blockIdx.x == 0) atomicAdd(&rec->n_total, (unsigned long long)a.n);
}

}  // namespace

hipError_t launch_pstat(const PstatLaunch& a, hipStream_t s) {
  if (a.n == 0 || a.C <= 0) return hipSuccess;
  const size_t unit = a.fmt == 2 ? 8 : 2;
  const unsigned most = unsigned(kPstatMaxGrid / a.C > 0 ? kPstatMaxGrid / a.C : 1);
  for (size_t off = 0; off < a.n; off += size_t(kPstatMaxLaunchSamples)) {
    PstatLaunch b = a;
    b.in = static_cast<const char*>(a.in) + off * unit;
    b.n = a.n - off < size_t(kPstatMaxLaunchSamples) ? a.n - off : size_t(kPstatMaxLaunchSamples);
    const size_t tiles = (b.n + kPstatTile - 1) / kPstatTile;
    const unsigned gx = tiles < most ? unsigned(tiles) : most;
    hipLaunchKernelGGL(pstat_kernel, dim3(gx, unsigned(a.C)), dim3(kPstatThreads), 0, s, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace tdsa
