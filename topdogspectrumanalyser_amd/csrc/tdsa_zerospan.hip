// tdsa_zerospan.hip - zero span on the device: amplitude against time at the tuned frequency.
//
// zspan_push_kernel<format, detector>: unpack, detect, store into the ring.  Pure streaming, no LDS.  A launch takes
// one physically contiguous piece of the ring: a head of up to 3 samples brings the write position to a 16-byte
// boundary, the body moves 16 bytes per load (8 int8 / uint8 samples, 2 complex64, 4 real float32) and 16 bytes per
// store, a tail of fewer than one group finishes.  Head and tail are single samples on the first lanes of the grid.
//
// zspan_trigger_kernel: every lane tests its pairs (ring indices modulo the capacity) and keeps the largest hit; the
// maximum goes across the wave by shuffles, across the workgroup through LDS, and one integer atomicMax per workgroup
// into a word zeroed ahead of the launch.  An integer maximum is order-free: the result is reproducible.
//
// zspan_view_kernel<column detector, team>: reads the start the trigger search left (or the free-run start), writes
// the chunk or its P columns, and the chunk statistics.  Every sample of the chunk lies in exactly one cell, so the
// lane that reads sample k for its cell also counts it (and the pair k, k + 1) for the statistics: one pass over the
// window.  A TEAM of lanes owns a cell: a wave (64) for cells below kZsBlockCell samples, a workgroup (256) from there
// on, so that a 1 s window in 2048 columns runs on kZsMaxBlocks workgroups of 256 lanes and a 10 ms window on 512 of four waves.  Very few very long
// cells (P below the CU count at windows of seconds) leave the machine under-filled; nothing there is wrong, only slow.
// Integer counts: one atomicAdd per workgroup.  min, max and the float64 sum: one partial per workgroup, folded by the
// host in block order after the one read-back.  No workgroup waits for, or reads from, another.
#include <hip/hip_runtime.h>

#include "../../include/tdsa_hip.h"
#include "tdsa_wave.hpp"
#include "tdsa_zerospan.hpp"

// every rounding of the detectors is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kThreads = 256;
constexpr float kLog2ToDb = 3.0102999566398120f;    // 10 / log2(10)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// 16 input bytes at the alignment of one sample of each format
struct __attribute__((packed, aligned(2))) Load16A2 { u32x4 v; };
struct __attribute__((packed, aligned(4))) Load16A4 { u32x4 v; };
struct __attribute__((packed, aligned(8))) Load16A8 { u32x4 v; };

template <int FMT>
__device__ inline float unpack_byte(unsigned b) {
  if (FMT == TDSA_IN_I8) return float(int(b ^ 0x80u) - 128) * 0.0078125f;   // (float(b ^ 0x80) - 128) / 128: exact
  return (float(b) - 127.5f) * (1.0f / 127.5f);
}

template <int DET>
__device__ inline float detect(float re, float im, float log_floor, float offset_db) {
  if (DET == TDSA_ZS_DET_REAL) return re;
  const float p = re * re + im * im;
  // correctly rounded while hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt holds; __fsqrt_rn is the 1 ulp root
  if (DET == TDSA_ZS_DET_MAG) return __builtin_sqrtf(p);
  return log2f(p + log_floor) * kLog2ToDb + offset_db;
}

// samples per lane of the body: two 16-byte stores for the byte formats, one otherwise
template <int FMT>
struct Group {
  static constexpr int n = (FMT == TDSA_IN_I8 || FMT == TDSA_IN_U8) ? 8 : 4;
};

template <int FMT, int DET>
__device__ inline float push_one(const ZsPush& a, long long k) {
  float re, im = 0.f;
  if (FMT == TDSA_IN_I8 || FMT == TDSA_IN_U8) {
    const uchar2 v = static_cast<const uchar2*>(a.in)[k];
    re = unpack_byte<FMT>(v.x);
    im = unpack_byte<FMT>(v.y);
  } else if (FMT == TDSA_IN_C64) {
    const float2 v = static_cast<const float2*>(a.in)[k];
    re = v.x;
    im = v.y;
  } else {
    re = static_cast<const float*>(a.in)[k];
  }
  return detect<DET>(re, im, a.log_floor, a.offset_db);
}

template <int FMT, int DET>
__global__ __launch_bounds__(kThreads) void zspan_push_kernel(ZsPush a) {
  constexpr int G = Group<FMT>::n;
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long stride = (long long)gridDim.x * kThreads;
  long long head = (4 - ((reinterpret_cast<uintptr_t>(a.out) >> 2) & 3)) & 3;   // floats to the next 16-byte boundary
  if (head > a.n) head = a.n;
  const long long groups = (a.n - head) / G;
  const long long tail = head + groups * G;
  for (long long g = gid; g < groups; g += stride) {
    const long long k = head + g * G;
    float e[G];
    if (FMT == TDSA_IN_I8 || FMT == TDSA_IN_U8) {
      const u32x4 w = reinterpret_cast<const Load16A2*>(static_cast<const unsigned char*>(a.in) + 2 * k)->v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned pair = w[j / 2] >> (16 * (j % 2));
        e[j] = detect<DET>(unpack_byte<FMT>(pair & 0xFFu), unpack_byte<FMT>((pair >> 8) & 0xFFu), a.log_floor, a.offset_db);
      }
    } else if (FMT == TDSA_IN_C64) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4 w = reinterpret_cast<const Load16A8*>(static_cast<const float2*>(a.in) + k + 2 * h)->v;
        e[2 * h] = detect<DET>(__uint_as_float(w[0]), __uint_as_float(w[1]), a.log_floor, a.offset_db);
        e[2 * h + 1] = detect<DET>(__uint_as_float(w[2]), __uint_as_float(w[3]), a.log_floor, a.offset_db);
      }
    } else {
      const u32x4 w = reinterpret_cast<const Load16A4*>(static_cast<const float*>(a.in) + k)->v;
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = detect<DET>(__uint_as_float(w[j]), 0.f, a.log_floor, a.offset_db);
    }
#pragma unroll
    for (int q = 0; q < G / 4; ++q)
      *reinterpret_cast<f32x4*>(a.out + k + 4 * q) = f32x4{e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]};
  }
  const long long singles = head + (a.n - tail);   // fewer than 3 + G
  if (gid < singles) {
    const long long k = gid < head ? gid : tail + (gid - head);
    a.out[k] = push_one<FMT, DET>(a, k);
  }
}

__global__ __launch_bounds__(kThreads) void zspan_trigger_kernel(ZsTrigger a) {
  __shared__ int part[kThreads / 64];
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long stride = (long long)gridDim.x * kThreads;
  const long long p0 = a.first % a.cap;
  int best = 0;
  for (long long j = gid; j < a.n_pairs; j += stride) {
    long long p = p0 + j;
    if (p >= a.cap) p -= a.cap;
    const long long q = p + 1 == a.cap ? 0 : p + 1;
    const float u = a.ring[p], v = a.ring[q];
    const bool hit = a.fall ? (u >= a.level && v < a.level) : (u < a.level && v >= a.level);   // a NaN never matches
    if (hit) best = int(a.ss + j + 1);   // j ascends: the lane's last hit is its largest
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) best = part[w] > best ? part[w] : best;
    if (best > 0) atomicMax(&a.ctrl->trig, best);
  }
}

// np.min / np.max over float32: a NaN stays (kept as a flag, since fminf / fmaxf drop it)
struct MinMax {
  float mn, mx;
  int nan;
  __device__ static inline MinMax none() { return MinMax{INFINITY, -INFINITY, 0}; }
  __device__ inline void add(float v) {
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    nan |= int(v != v);
  }
  __device__ inline void wave_fold() {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      nan |= __shfl_xor(nan, o, 64);
    }
  }
  __device__ inline void fold(const MinMax& o) {
    mn = fminf(mn, o.mn);
    mx = fmaxf(mx, o.mx);
    nan |= o.nan;
  }
  __device__ inline float lo() const { return nan ? NAN : mn; }
  __device__ inline float hi() const { return nan ? NAN : mx; }
};

// the chunk statistics a lane gathers over the samples it reads
struct Stats {
  MinMax mm;
  double sum;
  long long n_ge;
  int n_rise, n_fall;
};

struct Chunk {
  const float* ring;
  long long cap, p0;   // p0: physical index of the chunk's first sample
  int length;
  float level;
  __device__ inline float at(long long k) const {
    long long p = p0 + k;
    if (p >= cap) p -= cap;
    return ring[p];
  }
  // sample k, counted for the statistics together with the pair (k, k + 1)
  __device__ inline float take(long long k, Stats& s) const {
    const float v = at(k);
    s.mm.add(v);
    s.sum = s.sum + double(v);
    const bool ge = v >= level;
    s.n_ge += ge;
    if (k + 1 < length) {
      const float nx = at(k + 1);
      s.n_rise += int(v < level && nx >= level);
      s.n_fall += int(ge && nx < level);
    }
    return v;
  }
};

constexpr int kColChunk = -1;   // the view kernel's mode for n_points = 0

template <int COL, int TEAM>
__global__ __launch_bounds__(kThreads) void zspan_view_kernel(ZsView a) {
  constexpr int kWaves = kThreads / 64;
  __shared__ MinMax s_mm[kWaves];
  __shared__ double s_sum[kWaves];
  __shared__ long long s_ge[kWaves];
  __shared__ int s_cross[kWaves][2];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int hit = a.use_trig ? a.ctrl->trig : 0;   // the trigger search ran before this launch, in stream order
  const long long start = hit > 0 ? a.base + hit : a.free_start;
  if (blockIdx.x == 0 && tid == 0) {
    a.ctrl->start = start;
    a.ctrl->triggered = hit > 0;
  }
  Chunk ch{a.ring, a.cap, start % a.cap, a.length, a.level};
  Stats st{MinMax::none(), 0.0, 0, 0, 0};
  if (COL == kColChunk) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long k = (long long)blockIdx.x * kThreads + tid; k < a.length; k += stride) a.out[k] = ch.take(k, st);
  } else {
    const int P = a.columns;
    const int lane = tid % TEAM;
    const int teams = gridDim.x * (kThreads / TEAM);
    for (int c = blockIdx.x * (kThreads / TEAM) + tid / TEAM; c < P; c += teams) {   // uniform over a team
      const long long lo = (long long)c * a.length / P, hi = (long long)(c + 1) * a.length / P;
      MinMax mm = MinMax::none();
      double sum = 0.0;
      for (long long k = lo + lane; k < hi; k += TEAM) {
        const float v = ch.take(k, st);
        if (COL == TDSA_ZS_COL_MINMAX) mm.add(v);
        if (COL == TDSA_ZS_COL_MEAN) sum = sum + double(v);
        if (COL == TDSA_ZS_COL_SAMPLE && k == lo) a.out[c] = v;
      }
      if (COL == TDSA_ZS_COL_MINMAX) {
        mm.wave_fold();
        if (TEAM > 64) {
          __syncthreads();   // the previous cell's partials have been read
          if ((tid & 63) == 0) s_mm[wave] = mm;
          __syncthreads();
          mm = s_mm[0];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) mm.fold(s_mm[w]);
        }
        if (lane == 0) {
          a.out[c] = mm.lo();
          a.out[P + c] = mm.hi();
        }
      }
      if (COL == TDSA_ZS_COL_MEAN) {
        sum = wave_sum(sum);
        if (TEAM > 64) {
          __syncthreads();
          if ((tid & 63) == 0) s_sum[wave] = sum;
          __syncthreads();
          sum = s_sum[0];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) sum = sum + s_sum[w];
        }
        if (lane == 0) a.out[c] = float(sum / double(hi - lo));   // float64 sum, rounded once
      }
    }
  }
  // the workgroup's share of the statistics
  st.mm.wave_fold();
  st.sum = wave_sum(st.sum);
  st.n_ge = wave_sum(st.n_ge);
  st.n_rise = wave_sum(st.n_rise);
  st.n_fall = wave_sum(st.n_fall);
  __syncthreads();
  if ((tid & 63) == 0) {
    s_mm[wave] = st.mm;
    s_sum[wave] = st.sum;
    s_ge[wave] = st.n_ge;
    s_cross[wave][0] = st.n_rise;
    s_cross[wave][1] = st.n_fall;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      st.mm.fold(s_mm[w]);
      st.sum = st.sum + s_sum[w];
      st.n_ge += s_ge[w];
      st.n_rise += s_cross[w][0];
      st.n_fall += s_cross[w][1];
    }
    a.part[blockIdx.x] = ZsPart{st.mm.lo(), st.mm.hi(), st.sum};
    if (st.n_ge) atomicAdd(&a.ctrl->n_ge, (unsigned long long)st.n_ge);
    if (st.n_rise) atomicAdd(&a.ctrl->n_rise, st.n_rise);
    if (st.n_fall) atomicAdd(&a.ctrl->n_fall, st.n_fall);
  }
}

template <int FMT>
hipError_t push_launch(const ZsPush& a, hipStream_t s) {
  const long long lanes = a.n / Group<FMT>::n + 16;   // the body's groups, and room for head and tail
  long long grid = (lanes + kThreads - 1) / kThreads;
  if (grid > 2048) grid = 2048;
  const dim3 g{unsigned(grid)}, b{kThreads};
  if (a.detector == TDSA_ZS_DET_REAL) hipLaunchKernelGGL((zspan_push_kernel<FMT, TDSA_ZS_DET_REAL>), g, b, 0, s, a);
  else if (a.detector == TDSA_ZS_DET_MAG) hipLaunchKernelGGL((zspan_push_kernel<FMT, TDSA_ZS_DET_MAG>), g, b, 0, s, a);
  else hipLaunchKernelGGL((zspan_push_kernel<FMT, TDSA_ZS_DET_DB>), g, b, 0, s, a);
  return hipGetLastError();
}

inline bool block_cells(const ZsView& a) { return a.columns > 0 && a.length / a.columns >= kZsBlockCell; }

template <int COL>
hipError_t view_launch(const ZsView& a, hipStream_t s) {
  const dim3 g{unsigned(a.blocks)}, b{kThreads};
  if (block_cells(a)) hipLaunchKernelGGL((zspan_view_kernel<COL, kThreads>), g, b, 0, s, a);
  else hipLaunchKernelGGL((zspan_view_kernel<COL, 64>), g, b, 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_zspan_push(const ZsPush& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.fmt == TDSA_IN_I8) return push_launch<TDSA_IN_I8>(a, s);
  if (a.fmt == TDSA_IN_U8) return push_launch<TDSA_IN_U8>(a, s);
  if (a.fmt == TDSA_IN_C64) return push_launch<TDSA_IN_C64>(a, s);
  return push_launch<TDSA_IN_F32R>(a, s);
}

hipError_t launch_zspan_trigger(const ZsTrigger& a, hipStream_t s) {
  if (a.n_pairs <= 0) return hipSuccess;
  long long grid = (a.n_pairs + 4 * kThreads - 1) / (4 * kThreads);   // about four pairs per lane
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(zspan_trigger_kernel, dim3(unsigned(grid)), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

int zs_view_blocks(const ZsView& a) {
  long long need;
  if (a.columns == 0) need = ((long long)a.length + 4 * kThreads - 1) / (4 * kThreads);
  else if (block_cells(a)) need = a.columns;
  else need = (a.columns + kThreads / 64 - 1) / (kThreads / 64);
  return int(need < 1 ? 1 : need > kZsMaxBlocks ? kZsMaxBlocks : need);
}

hipError_t launch_zspan_view(const ZsView& a, hipStream_t s) {
  if (a.columns == 0) {
    hipLaunchKernelGGL((zspan_view_kernel<kColChunk, 64>), dim3(unsigned(a.blocks)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  }
  if (a.col_detector == TDSA_ZS_COL_MINMAX) return view_launch<TDSA_ZS_COL_MINMAX>(a, s);
  if (a.col_detector == TDSA_ZS_COL_SAMPLE) return view_launch<TDSA_ZS_COL_SAMPLE>(a, s);
  return view_launch<TDSA_ZS_COL_MEAN>(a, s);
}

}  // namespace tdsa
