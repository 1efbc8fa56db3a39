// tdsa_eye.hip - eye diagrams: segments of a stream folded on their symbol clock into a density
// image of P columns by H rows, kept as integers.
//
// eye_kernel<KIND>: workgroups of 256 threads walk work items, item w = (segment w / ips, run w % ips of spi symbols), in
// steps of the grid, and merge once at the end.  The launcher sizes the items so that a one-segment tick spreads over
// the device and a long call fills the tile (tdsa_eye.hpp: eye_plan_item), and the grid by what the LDS holds per CU.  The image is sums of integers, so neither the grid nor the order of the
// items shows in the result.  Per item:
//   stage   the samples of the series under the item's points into LDS: x itself (IQ), or the tile's d_j and their
//           boxcar sums b_j as stages 0 and 1 of fsk_kernel form them (FM, REAL) - a sample passes through the
//           arctangent once per item
//   points  point q = (symbol ka + q / P, column q % P): position, coefficients, cubic interpolation from LDS, the
//           rotation (IQ), the row, one LDS add per eye; consecutive lanes take consecutive columns of one symbol and
//           never share a bin among them, lanes P apart may (a clean signal's hot bins): the LDS add serialises those
//   merge   the workgroup's non-zero uint32 bins into the uint64 counts with integer atomics, its totals likewise
// A workgroup adds fewer than 2^31 to a bin before it merges (launch_eye splits a call that would bring more).
// The positions, the resampler, the rotation and the discriminator are tdsa_symsync_math.hpp's and
// tdsa_seg_block.hpp's, called and not restated: column P / 2 is the producer's symbol, bit for bit.
#include <hip/hip_runtime.h>

#include "tdsa_eye.hpp"
#include "tdsa_fsk_math.hpp"
#include "tdsa_seg_block.hpp"

// every rounding below is written out
#pragma clang fp contract(off)

namespace tdsa {
namespace {

constexpr int kT = kEyeThreads;
static_assert(kEyeThreads == kSegThreads, "seg_boxcar_tile strides by the segment analysers' workgroup");

// one value of one eye into the workgroup's image: t = (v - lo) * scale, two roundings
__device__ inline void eye_add(unsigned* hist, unsigned* tot, float v, float lo, float scale, int H, int log2p, int c) {
  const float t = (v - lo) * scale;
  if (t != t) atomicAdd(&tot[3], 1u);
  else if (t < 0.0f) atomicAdd(&tot[1], 1u);
  else if (t >= float(H)) atomicAdd(&tot[2], 1u);
  else atomicAdd(&hist[(int(t) << log2p) + c], 1u);
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int KIND>
__global__ __launch_bounds__(kT) void eye_kernel(EyeLaunch a, long long n_items, int ips, int spi) {
  extern __shared__ unsigned hist[];               // [eyes][H][P]
  __shared__ __attribute__((aligned(16))) float tile[kEyeTile + kEyeTileD];   // IQ: float2 x[kEyeTile]; FM, REAL: b[kEyeTile], then d[kEyeTileD]
  __shared__ unsigned tot[16];                     // per eye {-, under, over, nan}
  constexpr int kEyes = KIND == kEyeIq ? 2 : 1;
  const int tid = threadIdx.x;
  const int K = a.K, B = a.boxcar, H = a.rows, log2p = a.log2p, P = 1 << log2p;
  const int nbins = kEyes * (H << log2p);
  const int n_in = int(a.seg_len);                 // K <= 4096 at 64 samples per symbol: far inside an int
  for (int b = tid; b < nbins; b += kT) hist[b] = 0u;
  if (tid < 16) tot[tid] = 0u;
  __syncthreads();
  unsigned n_points = 0u, n_segs = 0u, n_skipped = 0u;   // thread 0's
  float* tb = tile;
  float* td = tile + kEyeTile;
  float2* tx = reinterpret_cast<float2*>(tile);
  const float inv_b = fsk_boxcar_scale(B);

  for (long long w = blockIdx.x; w < n_items; w += gridDim.x) {
    const long long s = w / ips;
    const int t = int(w - s * ips);
    const EyeClock ck = a.clocks[s];               // the same for every thread
    if (t == 0) {
      n_segs += 1u;
      if (ck.delta_fx == 0) n_skipped += 1u;
    }
    if (ck.delta_fx == 0) continue;
    const int ka = 1 + t * spi, kb = ka + spi < K - 1 ? ka + spi : K - 1;   // symbols [ka, kb)
    const int npts = (kb - ka) << log2p;
    n_points += unsigned(npts);
    // the first and the last position: columns 0 and P - 1 of the first and the last symbol
    const long long half = ((long long)(-(P >> 1)) * (long long)a.step) >> log2p;
    const long long last = ((long long)((P >> 1) - 1) * (long long)a.step) >> log2p;
    const uint64_t pos_a = ck.delta_fx + uint64_t(ka) * a.step + uint64_t(half);
    const uint64_t pos_b = ck.delta_fx + uint64_t(kb - 1) * a.step + uint64_t(last);
    const int j0 = int(sym_index(pos_a)) - 1;
    int nb = int(sym_index(pos_b)) + 3 - j0;       // taps j0 .. i_b + 2; spi keeps it within the tile
    nb = nb > kEyeTile ? kEyeTile : nb;

    // ---- stage.  The contract keeps every tap inside the series; the clamps cost nothing and keep a clock that broke
    // it inside the segment.
    if constexpr (KIND == kEyeIq) {
      const float2* x = static_cast<const float2*>(a.in) + s * a.hop;
      for (int m = tid; m < nb; m += kT) tx[m] = x[clampi(j0 + m, 0, n_in - 1)];
    } else {
      const void* seg = KIND == kEyeFm ? static_cast<const void*>(static_cast<const float2*>(a.in) + s * a.hop)
                                       : static_cast<const void*>(static_cast<const float*>(a.in) + s * a.hop);
      const int nd = nb + B - 1, n_d = n_in - (KIND == kEyeFm ? 1 : 0);
      for (int m = tid; m < nd; m += kT) td[m] = seg_disc<KIND == kEyeFm>(seg, clampi(j0 + m, 0, n_d - 1));
      __syncthreads();
      seg_boxcar_tile(td, tb, nb, B, inv_b, tid);
    }
    __syncthreads();

    // ---- points
    for (int q = tid; q < npts; q += kT) {
      const int k = ka + (q >> log2p), c = q & (P - 1);
      const long long off = ((long long)(c - (P >> 1)) * (long long)a.step) >> log2p;
      const uint64_t pos = ck.delta_fx + uint64_t(k) * a.step + uint64_t(off);
      const int i = clampi(int(sym_index(pos)) - j0, 1, kEyeTile - 3);
      float cf[4];
      sym_coeffs(sym_mu(pos), cf);
      const long long at = (((s * (K - 2) + (k - 1))) << log2p) + c;
      if constexpr (KIND == kEyeIq) {
        const float2 x0 = tx[i - 1], x1 = tx[i], x2 = tx[i + 1], x3 = tx[i + 2];
        const float2 y = make_float2(sym_interp(cf, x0.x, x1.x, x2.x, x3.x), sym_interp(cf, x0.y, x1.y, x2.y, x3.y));
        const long long offf = ((long long)(c - (P >> 1)) * (long long)int32_t(ck.step_f)) >> log2p;
        const uint32_t phi = ck.theta_fx + uint32_t(k) * ck.step_f + uint32_t(uint64_t(offf));
        const float2 r = rot(a.nco, phi);
        float2 v;
        sym_cmul(y.x, y.y, r.x, r.y, &v.x, &v.y);
        if (a.traces) static_cast<float2*>(a.traces)[at] = v;
        eye_add(hist, tot, v.x, a.lo, a.scale, H, log2p, c);
        eye_add(hist + (H << log2p), tot + 4, v.y, a.lo, a.scale, H, log2p, c);
      } else {
        const float v = sym_interp(cf, tb[i - 1], tb[i], tb[i + 1], tb[i + 2]);
        if (a.traces) static_cast<float*>(a.traces)[at] = v;
        eye_add(hist, tot, v, a.lo, a.scale, H, log2p, c);
      }
    }
    __syncthreads();   // the next item writes the tile behind this barrier
  }

  // ---- merge: most bins of most workgroups are empty
  __syncthreads();
  for (int b = tid; b < nbins; b += kT) {
    const unsigned v = hist[b];
    if (v) atomicAdd(&a.counts[b], (unsigned long long)v);
  }
  if (tid < 4 * kEyes && (tid & 3) != 0 && tot[tid]) atomicAdd(&a.totals[tid], (unsigned long long)tot[tid]);
  if (tid == 0) {
    if (n_points) {
      atomicAdd(&a.totals[0], (unsigned long long)n_points);
      if (kEyes == 2) atomicAdd(&a.totals[4], (unsigned long long)n_points);
    }
    if (n_segs) atomicAdd(&a.totals[8], (unsigned long long)n_segs);
    if (n_skipped) atomicAdd(&a.totals[9], (unsigned long long)n_skipped);
  }
}

template <int KIND>
hipError_t launch_kind(EyeLaunch a, hipStream_t s) {
  const int eyes = eye_count(KIND);
  const size_t lds = size_t(eyes) * size_t(a.rows << a.log2p) * sizeof(unsigned);
  const long long fit = (long long)a.num_cu * eye_groups_per_cu(lds);
  const long long groups_most = fit < kEyeMaxGroups ? fit : kEyeMaxGroups;
  const int spi = eye_plan_item(a.step, a.K, a.log2p, a.n_seg, groups_most);
  const int ips = (a.K - 2 + spi - 1) / spi;
  const long long seg_most = groups_most * kEyeItemsPerGroup / ips;     // segments one launch may bring
  const size_t in_unit = KIND == kEyeReal ? sizeof(float) : sizeof(float2);
  const size_t tr_unit = (KIND == kEyeIq ? sizeof(float2) : sizeof(float)) * size_t(a.K - 2) << a.log2p;
  const int n_seg = a.n_seg;
  for (long long s0 = 0; s0 < n_seg; s0 += seg_most) {
    EyeLaunch b = a;
    b.n_seg = int(n_seg - s0 < seg_most ? n_seg - s0 : seg_most);
    b.in = static_cast<const char*>(a.in) + size_t(s0) * size_t(a.hop) * in_unit;
    b.clocks = a.clocks + s0;
    if (a.traces) b.traces = static_cast<char*>(a.traces) + size_t(s0) * tr_unit;
    const long long n_items = (long long)b.n_seg * ips;
    const unsigned grid = unsigned(n_items < groups_most ? n_items : groups_most);
    hipLaunchKernelGGL(eye_kernel<KIND>, dim3(grid), dim3(kT), lds, s, b, n_items, ips, spi);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t eye_allow_lds() {
  const int most = kEyeMaxLdsBytes - kEyeStaticLdsBytes;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eye_kernel<kEyeIq>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, most);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eye_kernel<kEyeFm>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eye_kernel<kEyeReal>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
  return e;
}

hipError_t launch_eye(const EyeLaunch& a, hipStream_t s) {
  if (a.n_seg < 1) return hipSuccess;
  const int bins = a.rows << a.log2p;
  if (a.K < kEyeMinSymbols || a.K > kSegMaxSymbols || bins > kEyeMaxBins || a.step < kSegMinStep || a.step > kSegMaxStep)
    return hipErrorInvalidValue;
  if (a.kind == kEyeIq) return launch_kind<kEyeIq>(a, s);
  if (a.kind == kEyeFm) return launch_kind<kEyeFm>(a, s);
  return launch_kind<kEyeReal>(a, s);
}

}  // namespace tdsa
