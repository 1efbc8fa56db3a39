// tdsa_history.hip - the 3-D history views on the device.
//
//   hist_push_kernel      dB rows -> the trace ring (as heights z = clip((dB - bottom) / range * 8, 0, 8), or as they
//                         are), and in the same pass each row's maximum with the index of its first occurrence and the
//                         running hold row
//   hist_reduce_kernel    the screen reduction: per row and column cell the maximum and the bin of its first occurrence,
//                         a group of 4 / 16 / 64 lanes per cell
//   hist_ribbon_kernel    rows -> the ribbon meshes: interleaved vertices and per-vertex RGBA (float64 HSV sextants)
//   hist_lines_kernel     rows -> the line stack: z in view order and a colour index or its RGBA
//   hist_surface_kernel   rows -> the surface: normalised z (float64 arithmetic) and its colours
//
// This translation unit is built with -ffp-contract=off: every product, quotient and difference below is rounded on its
// own, as numpy rounds it; a fused multiply-add anywhere in the height or the HSV arithmetic changes the last bit.
//
// The view passes are store-bound (the ribbon writes 56 bytes for every 4 it reads).  With a bin count that is a
// multiple of 4 every lane loads 16 bytes of a row and writes whole 16-byte pieces of the interleaved records.  The
// stores are plain global stores: the gfx950 hazard between a store of more than 8 bytes and a VALU write of its data
// registers (tdsa_big.hip) is one the compiler's recognizer always pads for FLAT-class stores; the case it misses is the
// buffer store with an SGPR offset, which this file does not use (tests/test_history_kernel_resources.py looks).
#include "tdsa_history.hpp"
#include "tdsa_wave.hpp"

namespace tdsa {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ const float* hist_row(const HistSrc& s, int r) {
  int slot = r;
  if (!s.linear) {
    slot = (s.head - 1 - s.first - r) % s.depth;   // > -2 depth
    if (slot < 0) slot += s.depth;
  }
  return s.base + size_t(slot) * size_t(s.n);
}

// np.clip(x, lo, hi) of float32: a NaN stays, and so does a -0 at lo = +0 (numpy's maximum keeps its first operand)
__device__ __forceinline__ float hist_clip(float x, float lo, float hi) {
  x = x >= lo ? x : (x != x ? x : lo);
  return x <= hi ? x : (x != x ? x : hi);
}

__device__ __forceinline__ float hist_height(float db, float bottom, float range, float zscale) {
  return hist_clip(((db - bottom) / range) * zscale, 0.f, zscale);
}

// larger value first, then the smaller index: one integer maximum does np.argmax's tie rule (0 = nothing)
__device__ __forceinline__ unsigned long long hist_key(float v, int index) {
  unsigned b = __float_as_uint(v == 0.f ? 0.f : v);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (static_cast<unsigned long long>(b) << 32) | static_cast<unsigned long long>(~unsigned(index));
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---- push -----------------------------------------------------------------------------------------------------------
// grid (column pieces, row chunks).  A lane owns V consecutive bins over the rows of its chunk.  Everything that crosses
// workgroups is a maximum (slot keys, hold bits), so the result does not depend on their order.
template <int V>
__global__ __launch_bounds__(kBlock) void hist_push_kernel(HistPush a) {
  const long long col = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) * V;
  const bool live = col < a.n;   // V = 4: n is a multiple of 4
  const int r0 = blockIdx.y * a.rows_per_wg;
  const int r1 = r0 + a.rows_per_wg < a.n_rows ? r0 + a.rows_per_wg : a.n_rows;
  float hold[V];
#pragma unroll
  for (int j = 0; j < V; ++j) hold[j] = 0.f;
  for (int k = r0; k < r1; ++k) {
    const int slot = (a.head + k) % a.depth;
    unsigned long long key = 0;
    if (live) {
      Vec<V> x;
      x.load(a.in + size_t(k) * size_t(a.n) + size_t(col));
      if (a.heights) {
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] = hist_height(x.v[j], a.bottom, a.range, a.zscale);
      }
      float bv = x.v[0];
      int bi = 0;
#pragma unroll
      for (int j = 1; j < V; ++j)
        if (x.v[j] > bv) bv = x.v[j], bi = j;
#pragma unroll
      for (int j = 0; j < V; ++j) hold[j] = x.v[j] > hold[j] ? x.v[j] : hold[j];
      if (k >= a.skip) {
        x.store(a.ring + size_t(slot) * size_t(a.n) + size_t(col));
        key = hist_key(bv, int(col) + bi);
      }
    }
    if (k >= a.skip) {   // the same for the whole workgroup
      key = wave_reduce(key, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
      if ((threadIdx.x & 63) == 0 && key != 0) atomicMax(a.keys + slot, key);
    }
  }
  if (!live || !a.heights) return;
  if (a.update_hold) {
    if (a.hold_in) {
      Vec<V> m;
      m.load(a.hold_in + size_t(col));
#pragma unroll
      for (int j = 0; j < V; ++j) hold[j] = hist_height(m.v[j], a.bottom, a.range, a.zscale);
    }
#pragma unroll
    for (int j = 0; j < V; ++j)   // z >= 0: the order of the bits is the order of the values; + 0 makes a -0 a +0
      atomicMax(reinterpret_cast<unsigned*>(a.hold + size_t(col) + j), __float_as_uint(hold[j] + 0.f));
  }
  if (a.min_in && blockIdx.y == 0) {
    Vec<V> m;
    m.load(a.min_in + size_t(col));
#pragma unroll
    for (int j = 0; j < V; ++j) m.v[j] = hist_height(m.v[j], a.bottom, a.range, a.zscale);
    m.store(a.min_out + size_t(col));
  }
}

// ---- screen reduction -----------------------------------------------------------------------------------------------
// G lanes per (row, column) cell; a lane keeps the first maximum of the bins it strides over, the group then takes the
// larger value and, between equal values, the smaller bin.
__global__ __launch_bounds__(kBlock) void hist_reduce_kernel(HistReduce a, int G) {
  const long long total = static_cast<long long>(a.rows) * a.columns;
  const long long cell = static_cast<long long>(blockIdx.x) * (kBlock / G) + threadIdx.x / G;
  const int lane = threadIdx.x % G;
  const bool live = cell < total;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if (live) {
    const int r = int(cell / a.columns), c = int(cell % a.columns);
    const int lo = int((static_cast<long long>(c) * a.src.n) / a.columns);
    const int hi = int((static_cast<long long>(c + 1) * a.src.n) / a.columns);
    const float* row = hist_row(a.src, r);
    for (int j = lo + lane; j < hi; j += G) {
      const float v = row[j];
      if (v > bv || bi == 0x7fffffff) bv = v, bi = j;
    }
  }
  for (int o = G >> 1; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi) || bi == 0x7fffffff) bv = ov, bi = oi;
  }
  if (live && lane == 0) {
    a.vals[cell] = bv;
    a.bins[cell] = bi;
  }
}

// ---- ribbon ---------------------------------------------------------------------------------------------------------
// float32 up to the hue, float64 from there (numpy's float64 `val` scalar is not weak, so the reference's hsv_to_rgb
// runs in float64 on the float32-rounded hue); one rounding to float32 at the end.  s = 1.
__device__ __forceinline__ float4 hist_ribbon_colour(float z, const HistRibbonRow& rc) {
  const float t = hist_clip(z / 8.0f, 0.f, 1.f);
  const float hue = ((1.0f - t) * 0.66f) * rc.hue_scale;
  const double h6 = double(hue) * 6.0;
  const int i = int(h6);
  const double f = h6 - double(i);
  const double v = rc.val;
  const double p = v * (1.0 - 1.0);
  const double q = v * (1.0 - f);
  const double u = v * (1.0 - (1.0 - f));
  double r, g, b;
  switch (i % 6) {
    case 0: r = v, g = u, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = u; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = u, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
  return make_float4(float(r), float(g), float(b), rc.alpha);
}

// grid (pieces of a row, rows).  VEC: 4 bins per lane = 6 16-byte stores of vertices and 8 of colours.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void hist_ribbon_kernel(HistRibbon a) {
  constexpr int V = VEC ? 4 : 1;
  const int r = blockIdx.y, n = a.src.n;
  const long long j = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (j >= n) return;
  const HistRibbonRow rc = a.row[r];
  Vec<V> z, x;
  z.load(hist_row(a.src, r) + j);
  if (a.bins) {
    const int* b = a.bins + size_t(r) * size_t(n) + size_t(j);
#pragma unroll
    for (int k = 0; k < V; ++k) x.v[k] = a.x[b[k]];
  } else {
    x.load(a.x + j);
  }
  float4 col[V];
#pragma unroll
  for (int k = 0; k < V; ++k) col[k] = hist_ribbon_colour(z.v[k], rc);
  float* vo = a.verts + (size_t(r) * size_t(n) + size_t(j)) * 6;
  float* co = a.colours + (size_t(r) * size_t(n) + size_t(j)) * 8;
  if constexpr (VEC) {
    float4* v4 = reinterpret_cast<float4*>(vo);
    float4* c4 = reinterpret_cast<float4*>(co);
#pragma unroll
    for (int k = 0; k < 4; k += 2) {   // (x, y_front, z), (x, y_back, z) of two bins = three stores
      v4[3 * (k / 2) + 0] = make_float4(x.v[k], rc.y_front, z.v[k], x.v[k]);
      v4[3 * (k / 2) + 1] = make_float4(rc.y_back, z.v[k], x.v[k + 1], rc.y_front);
      v4[3 * (k / 2) + 2] = make_float4(z.v[k + 1], x.v[k + 1], rc.y_back, z.v[k + 1]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) c4[2 * k] = col[k], c4[2 * k + 1] = col[k];
  } else {
    vo[0] = x.v[0], vo[1] = rc.y_front, vo[2] = z.v[0];
    vo[3] = x.v[0], vo[4] = rc.y_back, vo[5] = z.v[0];
    co[0] = col[0].x, co[1] = col[0].y, co[2] = col[0].z, co[3] = col[0].w;
    co[4] = col[0].x, co[5] = col[0].y, co[6] = col[0].z, co[7] = col[0].w;
  }
}

// ---- line stack -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int hist_line_index(float z) { return int(8.0f - z) % kHistHues; }

// one lane per V bins of the rows * n values of the view
template <bool VEC>
__global__ __launch_bounds__(kBlock) void hist_lines_kernel(HistLines a) {
  constexpr int V = VEC ? 4 : 1;
  const unsigned per_row = unsigned(a.src.n) / V;
  const unsigned long long gid = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (gid >= static_cast<unsigned long long>(per_row) * unsigned(a.rows)) return;
  const unsigned r = unsigned(gid / per_row);
  const unsigned j = unsigned(gid % per_row) * V;
  Vec<V> z;
  z.load(hist_row(a.src, int(r)) + j);
  const size_t at = size_t(r) * size_t(a.src.n) + j;
  z.store(a.z + at);
  const bool pushed = int(r) < a.valid;
  int idx[V];
#pragma unroll
  for (int k = 0; k < V; ++k) idx[k] = pushed ? hist_line_index(z.v[k]) : kHistNeverPushed;
  if (!a.rgba) {
    unsigned char* o = static_cast<unsigned char*>(a.colours) + at;
    if constexpr (VEC) {
      *reinterpret_cast<unsigned*>(o) = unsigned(idx[0]) | unsigned(idx[1]) << 8 | unsigned(idx[2]) << 16 | unsigned(idx[3]) << 24;
    } else {
      o[0] = static_cast<unsigned char>(idx[0]);
    }
    return;
  }
  float4* o = reinterpret_cast<float4*>(a.colours) + at;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int p = idx[k] < kHistHues ? idx[k] : 0;
    const float4 c = make_float4(a.palette[p][0], a.palette[p][1], a.palette[p][2], a.palette[p][3]);
    o[k] = idx[k] < kHistHues ? c : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ---- surface --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float hist_surface_norm(float level, const HistSurface& a) {
  if (a.flat) return 0.5f;
  double t = (double(level) - a.zmin) / a.span;
  t = t >= 0.0 ? t : (t != t ? t : 0.0);
  t = t <= 1.0 ? t : (t != t ? t : 1.0);
  return float(t);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void hist_surface_kernel(HistSurface a) {
  constexpr int V = VEC ? 4 : 1;
  const unsigned per_row = unsigned(a.src.n) / V;
  const unsigned long long gid = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (gid >= static_cast<unsigned long long>(per_row) * unsigned(a.rows)) return;
  const unsigned r = unsigned(gid / per_row);
  const unsigned j = unsigned(gid % per_row) * V;
  Vec<V> t;
  t.load(hist_row(a.src, int(r)) + j);
#pragma unroll
  for (int k = 0; k < V; ++k) t.v[k] = hist_surface_norm(t.v[k], a);
  const size_t at = size_t(r) * size_t(a.src.n) + j;
  t.store(a.z + at);
  float* c = a.colours + at * 3;
  if constexpr (VEC) {   // (t, 0, 1 - t) of four bins = three stores
    float4* c4 = reinterpret_cast<float4*>(c);
    c4[0] = make_float4(t.v[0], 0.f, 1.0f - t.v[0], t.v[1]);
    c4[1] = make_float4(0.f, 1.0f - t.v[1], t.v[2], 0.f);
    c4[2] = make_float4(1.0f - t.v[2], t.v[3], 0.f, 1.0f - t.v[3]);
  } else {
    c[0] = t.v[0], c[1] = 0.f, c[2] = 1.0f - t.v[0];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(unsigned long long items) { return unsigned((items + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_hist_push(const HistPush& a0, hipStream_t s) {
  HistPush a = a0;
  const bool vec = a.n % 4 == 0 && aligned16(a.in) && (!a.hold_in || aligned16(a.hold_in)) && (!a.min_in || aligned16(a.min_in));
  const int V = vec ? 4 : 1;
  const unsigned gx = blocks_for((unsigned long long)(a.n / V));
  unsigned gy = kHistPushMaxWgs / gx < 1 ? 1 : kHistPushMaxWgs / gx;
  if (gy > unsigned(a.n_rows)) gy = unsigned(a.n_rows);
  a.rows_per_wg = int((unsigned(a.n_rows) + gy - 1) / gy);
  gy = (unsigned(a.n_rows) + unsigned(a.rows_per_wg) - 1) / unsigned(a.rows_per_wg);
  if (vec)
    hipLaunchKernelGGL(hist_push_kernel<4>, dim3(gx, gy), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(hist_push_kernel<1>, dim3(gx, gy), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hist_reduce(const HistReduce& a, hipStream_t s) {
  const int cell = a.src.n / a.columns;
  const int G = cell >= 32 ? 64 : cell >= 8 ? 16 : 4;
  const unsigned long long total = (unsigned long long)a.rows * (unsigned long long)a.columns;
  const unsigned per_wg = unsigned(kBlock / G);
  hipLaunchKernelGGL(hist_reduce_kernel, dim3(unsigned((total + per_wg - 1) / per_wg)), dim3(kBlock), 0, s, a, G);
  return hipGetLastError();
}

hipError_t launch_hist_ribbon(const HistRibbon& a, hipStream_t s) {
  const bool vec = a.src.n % 4 == 0 && aligned16(a.src.base) && aligned16(a.x) && aligned16(a.verts) && aligned16(a.colours);
  const dim3 grid(blocks_for((unsigned long long)(a.src.n / (vec ? 4 : 1))), unsigned(a.rows));
  if (vec)
    hipLaunchKernelGGL(hist_ribbon_kernel<true>, grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(hist_ribbon_kernel<false>, grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hist_lines(const HistLines& a, hipStream_t s) {
  const bool vec = a.src.n % 4 == 0 && aligned16(a.src.base) && aligned16(a.z) && aligned16(a.colours);
  const unsigned grid = blocks_for((unsigned long long)(a.src.n / (vec ? 4 : 1)) * (unsigned long long)a.rows);
  if (vec)
    hipLaunchKernelGGL(hist_lines_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(hist_lines_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hist_surface(const HistSurface& a, hipStream_t s) {
  const bool vec = a.src.n % 4 == 0 && aligned16(a.src.base) && aligned16(a.z) && aligned16(a.colours);
  const unsigned grid = blocks_for((unsigned long long)(a.src.n / (vec ? 4 : 1)) * (unsigned long long)a.rows);
  if (vec)
    hipLaunchKernelGGL(hist_surface_kernel<true>, dim3(grid), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(hist_surface_kernel<false>, dim3(grid), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace tdsa
