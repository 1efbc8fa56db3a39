// tdsa_unpack.hpp - raw IQ sample k of an input format as a complex float, for the kernels that take the formats at
// run time: the down-converter, the channelizer and the constellation kernels.  Zero span and
// the frame kernel unpack uint8 as (float(u) - 127.5) * (1 / 127.5) on purpose and do not use this.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

// the uint8 table, by a workgroup of 256 threads into 256 floats of LDS (a barrier before the first unpack_iq)
__device__ inline void fill_lut(int fmt, float* lut) {
  if (fmt == 1) lut[threadIdx.x] = float(double(threadIdx.x) / 127.5 - 1.0);   // pyrtlsdr's float64, then float32
}

__device__ inline float2 unpack_iq(int fmt, const void* in, long long k, const float* lut) {
  float re, im;
  if (fmt == 0) {
    const char2 v = static_cast<const char2*>(in)[k];
    re = float(v.x) * 0.0078125f;   // (I + jQ) / 128: exact
    im = float(v.y) * 0.0078125f;
  } else if (fmt == 1) {
    const uchar2 v = static_cast<const uchar2*>(in)[k];
    re = lut[v.x];
    im = lut[v.y];
  } else {
    const float2 v = static_cast<const float2*>(in)[k];
    re = v.x;
    im = v.y;
  }
  return make_float2(re, im);
}

}  // namespace tdsa
