// tdsa_seg_block.hpp - what the kernels of the segment analysers (tdsa_symsync.hip, tdsa_fsk.hip) and of the eye diagrams
// (tdsa_eye.hip) share, device only: the rotation, the discriminator and the boxcar of a tile, the workgroup's folds.  A kernel's bit-for-bit tests pin the tree of every float fold, and it is stated
// here and nowhere else: thread t's slot with that of t + 128, t + 64, ... 1, own slot first.
#pragma once
#include <hip/hip_runtime.h>

#include "tdsa_seg.hpp"
#include "tdsa_symsync_math.hpp"

namespace tdsa {

// exp(-2 pi i p / 2^32) from nco, [kSegNcoTable] (cos, -sin) of 2 pi k / 4096
__device__ inline float2 rot(const float2* nco, uint32_t p) {
  const float2 h = nco[p >> 20];
  float2 r;
  sym_rot(p, h.x, h.y, &r.x, &r.y);
  return r;
}

// d_j of a segment: the phase step from x[j] to x[j + 1] in half turns (IQ: complex64), or the input itself (float32)
template <bool IQ>
__device__ inline float seg_disc(const void* seg, int j) {
  if constexpr (IQ) {
    const float2* x = static_cast<const float2*>(seg);
    const float2 y0 = x[j], y1 = x[j + 1];
    return demod_fm(y1.x, y1.y, y0.x, y0.y);
  } else {
    return static_cast<const float*>(seg)[j];
  }
}

// The boxcar of a tile in LDS: tb[m] = (((td[m] + td[m + 1]) + ...) + td[m + B - 1]) * inv_b, m < nb, float32 adds in
// ascending order; consecutive threads read td at stride one.  The caller's barriers stand around it.
__device__ inline void seg_boxcar_tile(const float* td, float* tb, int nb, int B, float inv_b, int tid) {
  for (int m = tid; m < nb; m += kSegThreads) {
    float sum = td[m];
    for (int i = 1; i < B; ++i) sum = sum + td[m + i];
    tb[m] = sum * inv_b;
  }
}

// The workgroup's fold of one 16-byte slot a thread, every thread gets the result; the first barrier frees `red` from
// its last use.  fold(p, q) combines the slots of threads t and t + o into t's.
template <class T, class Fold>
__device__ inline T block_fold(T v, T* red, int tid, Fold fold) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = kSegThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = fold(red[tid], red[tid + o]);
    __syncthreads();
  }
  return red[0];
}

// four sums at once, or three (.w is 0)
__device__ inline float4 block_sum4(float4 v, float4* red, int tid) {
  return block_fold(v, red, tid, [](float4 p, float4 q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); });
}
__device__ inline float4 block_sum3(float x, float y, float z, float4* red, int tid) {
  return block_fold(make_float4(x, y, z, 0.0f), red, tid,
                    [](float4 p, float4 q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, 0.0f); });
}
__device__ inline double2 block_sum2(double x, double y, double2* red, int tid) {
  return block_fold(make_double2(x, y), red, tid, [](double2 p, double2 q) { return make_double2(p.x + q.x, p.y + q.y); });
}
// integers: exact, whatever the tree
__device__ inline int4 block_sum2i(int x, int y, int4* red, int tid) {
  return block_fold(make_int4(x, y, 0, 0), red, tid, [](int4 p, int4 q) { return make_int4(p.x + q.x, p.y + q.y, 0, 0); });
}
// .x the smallest, .y the largest, .z above zero where any thread's is: its flag for a value that is not finite
__device__ inline float4 block_minmax(float lo, float hi, float bad, float4* red, int tid) {
  return block_fold(make_float4(lo, hi, bad, 0.0f), red, tid, [](float4 p, float4 q) {
    return make_float4(q.x < p.x ? q.x : p.x, q.y > p.y ? q.y : p.y, q.z > p.z ? q.z : p.z, 0.0f);
  });
}
// (value, index) pairs in .x, .y: the largest value, among equals the lowest index - an order, so any tree gives the
// same pair ...
__device__ inline float4 block_argmax(float best, int idx, float4* red, int tid) {
  return block_fold(make_float4(best, __int_as_float(idx), 0.0f, 0.0f), red, tid, [](float4 p, float4 q) {
    const int pi = __float_as_int(p.y), qi = __float_as_int(q.y);
    return q.x > p.x || (q.x == p.x && qi < pi) ? q : p;
  });
}
// ... and with .z riding along as a sum
__device__ inline float4 block_argmax_sum(float best, int idx, float tot, float4* red, int tid) {
  return block_fold(make_float4(best, __int_as_float(idx), tot, 0.0f), red, tid, [](float4 p, float4 q) {
    const int pi = __float_as_int(p.y), qi = __float_as_int(q.y);
    if (q.x > p.x || (q.x == p.x && qi < pi)) {
      p.x = q.x;
      p.y = q.y;
    }
    p.z = p.z + q.z;
    return p;
  });
}

}  // namespace tdsa
