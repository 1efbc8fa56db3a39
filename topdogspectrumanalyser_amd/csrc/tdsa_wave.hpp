// tdsa_wave.hpp - the lane-level idioms of the kernels, once (device only): the xor butterfly across a wave64 or a
// segment of it, the scan from lane 0 up, the DPP controls and the reduction ladders built from them, and float max /
// min through integer atomics.  What a kernel's bit-for-bit tests pin about a reduction - the order in which the operands are combined,
// the lanes that hold the result, whether a NaN is dropped - is stated here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace tdsa {

// ---- xor butterfly ---------------------------------------------------------------------------------------------
// (value, index) as the peak searches carry it
struct PeakPair {
  float v;
  int i;
};

// v = op(v, the value of lane ^ o) for o = W / 2, W / 4 .. 1: every lane of a segment of W lanes (a power of two, 64 =
// the wave) ends with the result of its segment.  The step order (the widest first) and the operand order (own value
// first) are the contract: a float sum rounds by them, an op with ties decides by them.  A commutative op gives every
// lane the same bits - a + b on one lane, b + a on its partner - which is what lets any lane speak for the wave.
template <int W = 64, class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}
template <int W = 64, class T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce<W>(v, [](T a, T b) { return a + b; });
}
__device__ __forceinline__ int wave_max(int v) {
  return wave_reduce(v, [](int a, int b) { return b > a ? b : a; });
}
// the same butterfly for a pair: the lane takes its partner's pair where better(partner's, own) says so, e.g. in
// np.argmax order.  (Written out: with the pair passed through wave_reduce's op by value the compiler lays the
// branches of a comparison like analytics' `better` out differently.)
template <class Better>
__device__ __forceinline__ PeakPair wave_best(PeakPair p, Better better) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    PeakPair q{__shfl_xor(p.v, o), __shfl_xor(p.i, o)};
    if (better(q, p)) p = q;
  }
  return p;
}
// A kernel that folds several values side by side in ONE butterfly (min, max and a NaN flag; the I and the Q of a
// frame) keeps its own loop: taken apart into calls of the above, one value's steps come behind the other's and the
// kernel's instruction stream changes.  tests/test_isa_frozen.py lists those loops.

// ---- scan --------------------------------------------------------------------------------------------------------
// Inclusive scan from lane 0 up: lane l ends with the op over lanes 0 .. l.  Steps at distance 1, 2 .. 32, own value
// first: the order a float scan rounds by.  wave_lane_below hands every lane the value of the lane below it (lane 0:
// `first`), which turns the inclusive scan into the exclusive one.
template <class T, class Op>
__device__ __forceinline__ T wave_scan_inclusive(T v, Op op) {
  const int lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v = op(v, o);
  }
  return v;
}
template <class T>
__device__ __forceinline__ T wave_lane_below(T v, T first) {
  const T o = __shfl_up(v, 1);
  return __lane_id() == 0 ? first : o;
}

// ---- DPP ---------------------------------------------------------------------------------------------------------
// One type per control: the dpp_ctrl operand and the row mask it is used with.  A row is 16 lanes; the two
// broadcasts write rows 1, 3 and rows 2, 3 only, which is what makes a ladder end in lane 63.
template <int CTRL, int ROW_MASK>
struct Dpp {
  static constexpr int ctrl = CTRL, row_mask = ROW_MASK;
};
using QuadSwap1 = Dpp<0xB1, 0xf>;        // quad_perm [1,0,3,2]
using QuadSwap2 = Dpp<0x4E, 0xf>;        // quad_perm [2,3,0,1]
using RowHalfMirror = Dpp<0x141, 0xf>;   // row_half_mirror
using RowMirror = Dpp<0x140, 0xf>;       // row_mirror: after the four steps every lane holds its row's result
using RowBcast15 = Dpp<0x142, 0xa>;      // row_bcast:15 -> rows 1, 3: lanes 31 and 63 hold their half's result
using RowBcast31 = Dpp<0x143, 0xc>;      // row_bcast:31 -> rows 2, 3: lane 63 holds the wave's result

// the source lane's x; a lane without a source lane (or masked off) keeps its own, the identity of min / max / "better"
template <class D>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(x, x, D::ctrl, D::row_mask, 0xf, false);
}
template <class D>
__device__ __forceinline__ float dpp_f(float x) {
  return __uint_as_float(dpp_i<D>(__float_as_uint(x)));
}
// ... gets 0, the identity of a sum.  BOUND_CTRL where every source lane exists and the mask is full: `old` is never read
template <class D, bool BOUND_CTRL>
__device__ __forceinline__ int dpp_or0(int x) {
  return __builtin_amdgcn_update_dpp(0, x, D::ctrl, D::row_mask, 0xf, BOUND_CTRL);
}
template <class D, bool BOUND_CTRL>
__device__ __forceinline__ float dpp_or0(float x) {
  return __uint_as_float(dpp_or0<D, BOUND_CTRL>(int(__float_as_uint(x))));
}

// every lane: the minimum of its row of 16 lanes (fminf: a NaN operand is ignored)
__device__ __forceinline__ float row_min(float x) {
  x = fminf(x, dpp_f<QuadSwap1>(x));
  x = fminf(x, dpp_f<QuadSwap2>(x));
  x = fminf(x, dpp_f<RowHalfMirror>(x));
  x = fminf(x, dpp_f<RowMirror>(x));
  return x;
}
// lanes 31 and 63 only: the minimum of their half of the wave
__device__ __forceinline__ float half_min_to_lanes31_63(float x) {
  x = row_min(x);
  return fminf(x, dpp_f<RowBcast15>(x));
}
// lane 63 only: the minimum of the wave
__device__ __forceinline__ float wave_min_to_lane63(float x) {
  x = half_min_to_lanes31_63(x);
  return fminf(x, dpp_f<RowBcast31>(x));
}
// the stronger of a candidate and the one its source lane holds; equal values: the larger index (the order of a
// reversed ascending sort)
__device__ __forceinline__ void take_stronger(PeakPair& p, float qv, int qi) {
  if (qv > p.v || (qv == p.v && qi > p.i)) p = PeakPair{qv, qi};
}
// every lane: the strongest of its row of 16 lanes
__device__ __forceinline__ PeakPair row_strongest(PeakPair p) {
  take_stronger(p, dpp_f<QuadSwap1>(p.v), dpp_i<QuadSwap1>(p.i));
  take_stronger(p, dpp_f<QuadSwap2>(p.v), dpp_i<QuadSwap2>(p.i));
  take_stronger(p, dpp_f<RowHalfMirror>(p.v), dpp_i<RowHalfMirror>(p.i));
  take_stronger(p, dpp_f<RowMirror>(p.v), dpp_i<RowMirror>(p.i));
  return p;
}
// lane 63 only: the strongest of the wave
__device__ __forceinline__ PeakPair wave_strongest_to_lane63(PeakPair p) {
  p = row_strongest(p);
  take_stronger(p, dpp_f<RowBcast15>(p.v), dpp_i<RowBcast15>(p.i));
  take_stronger(p, dpp_f<RowBcast31>(p.v), dpp_i<RowBcast31>(p.i));
  return p;
}

// integer sum over the first LANES lanes' worth of a row (a power of two up to 16): every lane of an aligned group of
// LANES lanes holds the group's sum
template <int LANES>
__device__ __forceinline__ int dpp_row_sum(int x) {
  if constexpr (LANES >= 2) x += dpp_or0<QuadSwap1, false>(x);
  if constexpr (LANES >= 4) x += dpp_or0<QuadSwap2, false>(x);
  if constexpr (LANES >= 8) x += dpp_or0<RowHalfMirror, false>(x);
  if constexpr (LANES >= 16) x += dpp_or0<RowMirror, false>(x);
  return x;
}
// wave64 sums with DPP adds (no LDS round trips): x + source at every step, rows first.  The int total is valid in lanes
// 48 .. 63, the float total (rounded in that order) in lane 63
template <class T>
__device__ __forceinline__ T dpp_sum_ladder(T x) {
  x += dpp_or0<QuadSwap1, true>(x);
  x += dpp_or0<QuadSwap2, true>(x);
  x += dpp_or0<RowHalfMirror, true>(x);
  x += dpp_or0<RowMirror, true>(x);
  x += dpp_or0<RowBcast15, false>(x);
  x += dpp_or0<RowBcast31, false>(x);
  return x;
}
__device__ __forceinline__ int dpp_wave_sum(int x) { return dpp_sum_ladder(x); }
__device__ __forceinline__ float dpp_wave_sum63(float x) { return dpp_sum_ladder(x); }
// wave64 float maximum (NaN operands ignored); valid in lane 63
__device__ __forceinline__ float dpp_wave_max63(float x) {
  // v_max_f32 with the DPP operand in ONE instruction each (through the builtins it is v_mov, v_mov_dpp, v_max and three
  // s_nop per step); the two wait states a DPP read of a freshly written VGPR needs sit inside every statement, whatever
  // the compiler puts in front of it (its hazard recognizer does not look into inline assembly)
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(x));
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 0" : "+v"(x));
  return x;
}

// ---- float atomics -----------------------------------------------------------------------------------------------
// float max / min through integer atomics (IEEE-754 order trick: non-negative floats order like signed integers,
// negative ones like unsigned integers reversed).  A NaN candidate is skipped (np.fmax / np.fmin): it fails both tests.
__device__ __forceinline__ void atomic_fmax(float* addr, float v) {
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else if (v < 0.f) atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_fmin(float* addr, float v) {
  if (v >= 0.f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
  else if (v < 0.f) atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

}  // namespace tdsa
