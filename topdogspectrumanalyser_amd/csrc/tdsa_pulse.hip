// tdsa_pulse.hip - pulse descriptors of IQ streams: one record per pulse (time of arrival, width, peak, energy, the
// lag-one product that gives the carrier), a summary per stream (the contract is the comment
// block of tdsa_pulse_* in include/tdsa_hip.h and tests/pulse_contract.py).
//
//   power   p = fl(fl(re re) + fl(im im)), as tdsa_pstat.hip: the Makefile compiles this file with -ffp-contract=off
//   class   A: p >= on_level.  B: p < off_level or NaN.  C: neither.  A switches the stream on, B off, C keeps it
//   run     everything kept about a stretch of on samples is a PulseRecord; two stretches that touch join (run_join)
//
// The state machine is a scan, layered three times over the same operator:
//   thread      walks kPulseSamplesPerThread consecutive samples held in registers (walk)
//   workgroup   first the classes: the last class that is not C, scanned over the threads, tells every thread the state
//               it starts in - on, off, or U: no sample of the tile before it decides, so it is the state the tile
//               starts in.  Then the runs: a thread hands up (through, run) - the run still on at its end, and whether
//               it reaches back past the thread's start - and the scan of tdsa_wave.hpp plus four LDS slots give every
//               thread the run it continues.  The leading U samples are a run like any other.
//   launch      pulse_tile_kernel writes per tile what cannot be decided without the state coming in (PulseTileInfo).
//               pulse_stitch_kernel, one workgroup per stream, scans the tiles' summaries 256 at a time with the same
//               two scans, starting from the handle's state: it completes the pulses that cross tiles (the join runs
//               in tile order), writes them, numbers every tile's interior pulses, and leaves the open pulse, the
//               state and the counters in the handle.  pulse_tile_kernel<true> then writes the interior pulses.
// Three launches on one stream, the tile kernels with one workgroup per tile; no workgroup ever waits for another.
// The third pass reads the input again instead of buffering records: a tile can hold kPulseTile / 2 pulses of 64 bytes,
// 16 times the tile's int8 samples, while a tile without an interior pulse leaves the third pass after one word.
// Loads: a thread whose 16 samples are all there and whose stream starts on 16 bytes reads them as 16-byte vectors, any
// other by elements; both unpack with tdsa_unpack.hpp's arithmetic.  No float atomics: the sums are joined in scan order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tdsa_pulse.hpp"
#include "tdsa_unpack.hpp"
#include "tdsa_wave.hpp"

namespace tdsa {
namespace {

constexpr int kC = kPulseSamplesPerThread;
constexpr int U = 0, ON = 1, OFF = 2;            // a thread's or a tile's state; ON and OFF are the classes A and B
constexpr unsigned kInf = 1u, kIsF = 2u;         // flags: the public one; inside a tile, the run from its first A sample
static_assert(kC == 16 && kPulseThreads == 256, "the loaders and the LDS slots are written for 256 threads of 16 samples");
static_assert((long long)kPulseMaxLaunchTiles * kPulseTile < (1ll << 31), "a launch's sample indices fit an int");
static_assert(kPulseTile % 8 == 0, "a tile keeps its stream's 16-byte alignment");

using Run = PulseRecord;

__device__ __forceinline__ Run run_empty() {
  Run r;
  r.toa = 0, r.width = 0, r.peak_index = 0;
  r.peak_bits = 0u, r.flags = 0u;
  r.energy = 0.0, r.acc_re = 0.0, r.acc_im = 0.0;
  r.reserved = 0ull;
  return r;
}

// a's samples, then b's.  An empty run has peak_bits 0, below any on sample's, so it is the identity on both sides
__device__ __forceinline__ Run run_join(const Run& a, const Run& b) {
  Run r;
  r.toa = a.width ? a.toa : b.toa;
  r.width = a.width + b.width;
  const bool later = b.peak_bits > a.peak_bits;     // a tie keeps the first index
  r.peak_bits = later ? b.peak_bits : a.peak_bits;
  r.peak_index = later ? b.peak_index : a.peak_index;
  r.flags = a.flags | b.flags;
  r.energy = a.energy + b.energy;
  r.acc_re = a.acc_re + b.acc_re;
  r.acc_im = a.acc_im + b.acc_im;
  r.reserved = 0ull;
  return r;
}

// what a unit hands to the scan: the run still on at its end, and whether that run reaches back past the unit's start
// (then it continues whatever run comes in)
struct Elem {
  int through;
  Run r;
};
__device__ __forceinline__ Elem elem_identity() { return Elem{1, run_empty()}; }
struct ElemJoin {
  __device__ __forceinline__ Elem operator()(const Elem& a, const Elem& b) const {
    if (!b.through) return b;
    return Elem{a.through, run_join(a.r, b.r)};
  }
};
// found by wave_scan_inclusive and wave_lane_below (tdsa_wave.hpp) for an Elem
__device__ __forceinline__ Elem __shfl_up(const Elem& e, int d) {
  Elem o;
  o.through = ::__shfl_up(e.through, d);
  o.r.toa = ::__shfl_up(e.r.toa, d);
  o.r.width = ::__shfl_up(e.r.width, d);
  o.r.peak_index = ::__shfl_up(e.r.peak_index, d);
  o.r.peak_bits = ::__shfl_up(e.r.peak_bits, d);
  o.r.flags = ::__shfl_up(e.r.flags, d);
  o.r.energy = ::__shfl_up(e.r.energy, d);
  o.r.acc_re = ::__shfl_up(e.r.acc_re, d);
  o.r.acc_im = ::__shfl_up(e.r.acc_im, d);
  o.r.reserved = 0ull;
  return o;
}

// Exclusive scan over the 256 threads of a workgroup in thread order: join(lower, upper).  slots: four T of LDS, free
// again when the call returns.  *total: the join of all 256, in every thread.
template <class T, class Join>
__device__ __forceinline__ T block_scan_exclusive(const T& v, Join join, const T& ident, T* slots, T* total) {
  const T inc = wave_scan_inclusive(v, [join](const T& own, const T& lower) { return join(lower, own); });
  const T exc = wave_lane_below(inc, ident);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) slots[wave] = inc;
  __syncthreads();
  T pre = ident, all = ident;
#pragma unroll
  for (int w = 0; w < kPulseThreads / 64; ++w) {
    const T s = slots[w];
    if (w < wave) pre = join(pre, s);
    all = join(all, s);
  }
  __syncthreads();
  *total = all;
  return join(pre, exc);
}
struct LastClass {
  __device__ __forceinline__ int operator()(int lower, int upper) const { return upper ? upper : lower; }
};
struct IntSum {
  __device__ __forceinline__ int operator()(int a, int b) const { return a + b; }
};

struct Lds {
  float lut[256];
  Elem slots[4];
  int islots[4];
  int cnt[4];                    // n_nan, n_on, kept, n_short of the tile
  PulseTileInfo info;
};
static_assert(sizeof(Lds) <= kPulseLdsBudget, "the header states the LDS budget");

// ---- a thread's samples ------------------------------------------------------------------------------------------
struct Samples {
  float re[kC], im[kC];
  float pre, pim;                // the sample before the first
};

__device__ __forceinline__ void decode_bytes(int fmt, unsigned w, const float* lut, float& re0, float& im0, float& re1, float& im1) {
  const unsigned b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
  if (fmt == 1) {
    re0 = lut[b0], im0 = lut[b1], re1 = lut[b2], im1 = lut[b3];
  } else {
    re0 = float(int(int8_t(b0))) * 0.0078125f, im0 = float(int(int8_t(b1))) * 0.0078125f;
    re1 = float(int(int8_t(b2))) * 0.0078125f, im1 = float(int(int8_t(b3))) * 0.0078125f;
  }
}

// samples g0 .. g0 + nv - 1 of the stream at sb (nv <= 16; the rest zero); vec: 16-byte loads, only with nv = 16
__device__ __forceinline__ void load_samples(int fmt, const char* sb, int g0, int nv, bool vec, const float* lut, Samples& x) {
  if (vec && fmt == 2) {
    const uint4* vp = reinterpret_cast<const uint4*>(sb + size_t(g0) * 8);
#pragma unroll
    for (int k = 0; k < kC / 2; ++k) {
      const uint4 w = vp[k];
      x.re[2 * k] = __uint_as_float(w.x), x.im[2 * k] = __uint_as_float(w.y);
      x.re[2 * k + 1] = __uint_as_float(w.z), x.im[2 * k + 1] = __uint_as_float(w.w);
    }
  } else if (vec) {
    const uint4* vp = reinterpret_cast<const uint4*>(sb + size_t(g0) * 2);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint4 w = vp[k];
      decode_bytes(fmt, w.x, lut, x.re[8 * k + 0], x.im[8 * k + 0], x.re[8 * k + 1], x.im[8 * k + 1]);
      decode_bytes(fmt, w.y, lut, x.re[8 * k + 2], x.im[8 * k + 2], x.re[8 * k + 3], x.im[8 * k + 3]);
      decode_bytes(fmt, w.z, lut, x.re[8 * k + 4], x.im[8 * k + 4], x.re[8 * k + 5], x.im[8 * k + 5]);
      decode_bytes(fmt, w.w, lut, x.re[8 * k + 6], x.im[8 * k + 6], x.re[8 * k + 7], x.im[8 * k + 7]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kC; ++j) {
      float2 v = make_float2(0.0f, 0.0f);
      if (j < nv) v = unpack_iq(fmt, sb, g0 + j, lut);
      x.re[j] = v.x, x.im[j] = v.y;
    }
  }
}

__device__ __forceinline__ int classify(float p, float on_level, float off_level) {
  return p >= on_level ? ON : (p < off_level || p != p) ? OFF : 0;
}

__device__ __forceinline__ Run run_start(long long idx, float p, unsigned flags) {
  Run r = run_empty();
  r.toa = idx, r.width = 1, r.peak_index = idx;
  r.peak_bits = __float_as_uint(p);
  r.flags = flags | (r.peak_bits == 0x7f800000u ? kInf : 0u);
  r.energy = double(p);
  return r;
}

// x[n] conj(x[n - 1]): the products in float64, where they are exact, each sum rounded once
__device__ __forceinline__ void pair_add(Run& r, float re, float im, float qre, float qim) {
  r.acc_re += double(re) * double(qre) + double(im) * double(qim);
  r.acc_im += double(im) * double(qre) - double(re) * double(qim);
}

// What walk() leaves behind for the scans
struct Walked {
  Run head;            // the run that came in, up to where it ended or to the thread's end
  int head_closed;     // it ended inside the thread ...
  int closer;          // ... by a sample of this class (U only: the tile's first that is not C)
  Elem out;
  int n_on;
};

// The state machine over the thread's nv samples, which start at index i0 in state s_in.  A run that starts and ends
// inside the thread goes to done(run).  In state U the leading C samples are collected like a run that came in; the
// sample that ends them, if it is A, adds its pair to them (it belongs to the pulse exactly when they do) and starts
// the run marked kIsF.  FAST = false: the caller knows that a run ends inside the thread.
template <bool FAST, class Done>
__device__ __forceinline__ Walked walk(const Samples& x, unsigned cls, int nv, long long i0, int s_in, Done done) {
  Walked w;
  w.head = run_empty(), w.head_closed = 0, w.closer = 0, w.n_on = 0;
  // Most threads of a capture see no edge.  Off throughout: nothing to keep.  On throughout: the run that came in grows
  // by 16 samples, added in the order of the general walk below, so both give the same bits.
  const unsigned any_a = cls & 0x55555555u, any_b = cls & 0xaaaaaaaau;
  if (FAST && nv > 0 && s_in == OFF && !any_a) {
    w.out = Elem{0, run_empty()};
    return w;
  }
  if (FAST && nv == kC && s_in == ON && !any_b) {
    Run cur = run_empty();
    int at = 0;
#pragma unroll
    for (int j = 0; j < kC; ++j) {
      const float re = x.re[j], im = x.im[j];
      const float p = re * re + im * im;
      const unsigned bits = __float_as_uint(p);
      if (bits > cur.peak_bits) cur.peak_bits = bits, at = j;
      cur.energy += double(p);
      pair_add(cur, re, im, j ? x.re[j ? j - 1 : 0] : x.pre, j ? x.im[j ? j - 1 : 0] : x.pim);
    }
    cur.toa = i0, cur.width = kC, cur.peak_index = i0 + at;
    cur.flags = cur.peak_bits == 0x7f800000u ? kInf : 0u;
    w.head = cur, w.n_on = kC;
    w.out = Elem{1, cur};
    return w;
  }
  int s = s_in;
  bool in_head = s != OFF;
  Run cur = run_empty();
#pragma unroll
  for (int j = 0; j < kC; ++j) {
    if (j < nv) {
      const int code = int(cls >> (2 * j)) & 3;
      const float re = x.re[j], im = x.im[j];
      const float qre = j ? x.re[j ? j - 1 : 0] : x.pre, qim = j ? x.im[j ? j - 1 : 0] : x.pim;
      const float p = re * re + im * im;
      if (s == OFF) {
        if (code == ON) {
          cur = run_start(i0 + j, p, 0u);
          s = ON;
          ++w.n_on;
        }
      } else if (code == OFF || (s == U && code == ON)) {
        const bool starts = code == ON;
        if (starts) pair_add(cur, re, im, qre, qim);
        if (in_head) {
          w.head = cur, w.head_closed = 1, w.closer = code;
          in_head = false;
        } else {
          done(cur);
        }
        cur = starts ? run_start(i0 + j, p, kIsF) : run_empty();
        s = starts ? ON : OFF;
        w.n_on += starts ? 1 : 0;
      } else {
        if (cur.width == 0) cur.toa = i0 + j;
        ++cur.width;
        const unsigned bits = __float_as_uint(p);
        if (bits > cur.peak_bits) cur.peak_bits = bits, cur.peak_index = i0 + j;
        if (bits == 0x7f800000u) cur.flags |= kInf;
        cur.energy += double(p);
        pair_add(cur, re, im, qre, qim);
        w.n_on += s == ON ? 1 : 0;
      }
    }
  }
  if (nv <= 0) {
    w.out = elem_identity();
  } else if (in_head) {
    w.head = cur;
    w.out = Elem{1, cur};
  } else {
    w.out = Elem{0, s == ON ? cur : run_empty()};
  }
  return w;
}

__device__ __forceinline__ void store_record(PulseRecord* dst, Run r) {
  r.flags &= kInf;
  r.reserved = 0ull;
  *dst = r;
}

// ---- pass 1 (EMIT = false) and pass 3 (EMIT = true) ----------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(kPulseThreads) void pulse_tile_kernel(PulseLaunch a) {
  __shared__ Lds l;
  const int tid = threadIdx.x;
  const int c = blockIdx.y;
  fill_lut(a.fmt, l.lut);
  const size_t unit = a.fmt == 2 ? 8 : 2;
  const char* sb = static_cast<const char*>(a.in) + size_t(c) * a.in_stride * unit;
  const bool aligned = (reinterpret_cast<uintptr_t>(sb) & 15u) == 0u;
  const int n = int(a.n);                             // of a launch: at most kPulseMaxLaunchTiles tiles
  const int tiles = (n + kPulseTile - 1) / kPulseTile;
  const int min_width = a.min_width;
  PulseRecord* records = a.records + size_t(c) * size_t(a.capacity);

  const int tile = blockIdx.x;                        // one workgroup per tile: the launcher cuts a call into launches
  PulseTileInfo* ti = a.tiles + size_t(c) * size_t(tiles) + tile;
  if (EMIT && ti->kept == 0) return;                // the same word for every thread
  if (tid < 4) l.cnt[tid] = 0;
  if (tid == 0) {
    PulseTileInfo z{};
    l.info = z;
  }
  __syncthreads();                                  // also: the table is filled

  const int g0 = tile * kPulseTile + tid * kC;      // the thread's first sample, in the launch
  const int rest = n - g0;
  const int nv = rest >= kC ? kC : rest > 0 ? rest : 0;
  Samples x;
  load_samples(a.fmt, sb, g0, nv, aligned && nv == kC, l.lut, x);
  x.pre = 0.0f, x.pim = 0.0f;
  if (nv > 0) {
    const float2 q = g0 > 0 ? unpack_iq(a.fmt, sb, g0 - 1, l.lut) : a.prev[2 * c + a.parity];
    x.pre = q.x, x.pim = q.y;
  }

  // the classes, two bits a sample
  unsigned cls = 0u;
  int last = 0, n_nan = 0;
  bool not_b = false;
#pragma unroll
  for (int j = 0; j < kC; ++j) {
    if (j < nv) {
      const float p = x.re[j] * x.re[j] + x.im[j] * x.im[j];
      const int code = classify(p, a.on_level, a.off_level);
      cls |= unsigned(code) << (2 * j);
      last = code ? code : last;
      n_nan += p != p ? 1 : 0;
      not_b = not_b || code != OFF;
    }
  }
  if (!EMIT) {
    if (n_nan) atomicAdd(&l.cnt[0], n_nan);
    if (!__syncthreads_or(not_b)) {                 // nothing but B: off whatever comes in
      if (tid == 0) {
        ti->first = OFF, ti->last = OFF, ti->lead = 0, ti->f_closed = 0, ti->has_t = 0;
        ti->kept = 0, ti->n_short = 0, ti->n_on = 0, ti->n_nan = l.cnt[0], ti->slot = 0;
      }
      return;
    }
  }

  int last_all;
  const int s_in = block_scan_exclusive(last, LastClass(), 0, l.islots, &last_all);

  const long long i0 = a.base + g0;
  int kept = 0, n_short = 0;
  auto count = [&](const Run& r) {
    if (r.flags & kIsF) {
      if (!EMIT) l.info.F = r, l.info.f_closed = 1;
    } else if (r.width >= min_width) {
      ++kept;
    } else {
      ++n_short;
    }
  };
  const Walked w = walk<true>(x, cls, nv, i0, s_in, count);
  const int kept_inside = kept;
  Elem all;
  const Elem before = block_scan_exclusive(w.out, ElemJoin(), elem_identity(), l.slots, &all);
  Run full = run_empty();
  bool full_kept = false;
  if (w.head_closed) {
    full = run_join(before.r, w.head);
    if (s_in == U) {                                 // one thread of the tile at the most
      if (!EMIT) l.info.L = full, l.info.lead = int(full.width), l.info.first = w.closer;
    } else {
      const int k0 = kept;
      count(full);
      full_kept = kept > k0;
    }
  }

  if (EMIT) {
    int kept_all;
    long long slot = ti->slot + block_scan_exclusive(kept, IntSum(), 0, l.islots, &kept_all);
    auto emit = [&](const Run& r) {
      if (!(r.flags & kIsF) && r.width >= min_width) {
        if (slot < a.capacity) store_record(records + slot, r);
        ++slot;
      }
    };
    if (full_kept) emit(full);
    if (kept_inside) (void)walk<false>(x, cls, nv, i0, s_in, emit);
  } else {
    if (w.n_on) atomicAdd(&l.cnt[1], w.n_on);
    if (kept) atomicAdd(&l.cnt[2], kept);
    if (n_short) atomicAdd(&l.cnt[3], n_short);
    if (tid == 0) {
      l.info.last = last_all;
      if (all.through) {                             // C samples only
        l.info.L = all.r, l.info.lead = int(all.r.width);
      } else if (all.r.width) {
        if (all.r.flags & kIsF) l.info.F = all.r;
        else l.info.T = all.r, l.info.has_t = 1;
      }
    }
    __syncthreads();
    if (tid == 0) l.info.n_nan = l.cnt[0], l.info.n_on = l.cnt[1], l.info.kept = l.cnt[2], l.info.n_short = l.cnt[3];
    __syncthreads();
    constexpr int kWords = int(sizeof(PulseTileInfo) / 4);
    if (tid < kWords) reinterpret_cast<unsigned*>(ti)[tid] = reinterpret_cast<const unsigned*>(&l.info)[tid];
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------
struct StitchLds {
  Elem slots[4];
  int islots[4];
  unsigned long long cnt[3];     // n_on, n_short, n_nan of the launch
};

__global__ __launch_bounds__(kPulseThreads) void pulse_stitch_kernel(PulseLaunch a) {
  __shared__ StitchLds l;
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const long long n = (long long)a.n;
  const int tiles = int((n + kPulseTile - 1) / kPulseTile);
  PulseTileInfo* tis = a.tiles + size_t(c) * size_t(tiles);
  PulseRecord* records = a.records + size_t(c) * size_t(a.capacity);
  PulseSummary* sum = a.sum + c;
  if (tid < 3) l.cnt[tid] = 0ull;
  __syncthreads();

  // the same in every thread: the state, the open pulse, the pulses kept so far
  int state = sum->open ? ON : OFF;
  Run carry = state == ON ? a.open[c] : run_empty();
  unsigned long long n_pulses = sum->n_pulses;
  unsigned long long my_on = 0ull, my_short = 0ull, my_nan = 0ull;

  for (int t0 = 0; t0 < tiles; t0 += kPulseThreads) {
    const int tile = t0 + tid;
    const bool valid = tile < tiles;
    PulseTileInfo* ti = tis + (valid ? tile : 0);
    int first = 0, last = 0, lead = 0, f_closed = 0, has_t = 0, kept_in = 0;
    if (valid) {
      first = ti->first, last = ti->last, lead = ti->lead, f_closed = ti->f_closed, has_t = ti->has_t, kept_in = ti->kept;
      my_short += unsigned(ti->n_short), my_on += unsigned(ti->n_on), my_nan += unsigned(ti->n_nan);
    }
    int last_all;
    const int before_state = block_scan_exclusive(last, LastClass(), 0, l.islots, &last_all);
    const int s_in = before_state ? before_state : state;
    state = last_all ? last_all : state;

    Elem e = elem_identity();
    Run part = run_empty();        // what the tile adds to the pulse that ends in it
    bool ends = false, alone = false;
    if (valid) {
      Run tail = run_empty();
      if (has_t) tail = ti->T, tail.flags &= kInf;
      if (s_in == ON) {
        my_on += unsigned(lead);
        if (lead > 0 || first == ON) part = ti->L;
        if (first == ON) part = run_join(part, ti->F);
        part.flags &= kInf;
        ends = first == OFF || (first == ON && f_closed);
        e = ends ? Elem{0, tail} : Elem{1, part};
      } else if (first == ON) {
        part = ti->F;
        part.flags &= kInf;
        alone = f_closed != 0;
        e = alone ? Elem{0, tail} : Elem{0, part};
      } else {
        e = Elem{0, tail};
      }
    }
    Elem all;
    const Elem before = block_scan_exclusive(e, ElemJoin(), elem_identity(), l.slots, &all);
    const Run coming = before.through ? run_join(carry, before.r) : before.r;
    carry = all.through ? run_join(carry, all.r) : all.r;

    Run pulse = run_empty();
    int kept_x = 0;
    if (ends || alone) {
      pulse = alone ? part : run_join(coming, part);
      if (pulse.width >= a.min_width) kept_x = 1;
      else ++my_short;
    }
    int kept_all;
    const int kept_before = block_scan_exclusive(valid ? kept_x + kept_in : 0, IntSum(), 0, l.islots, &kept_all);
    const unsigned long long ord = n_pulses + (unsigned long long)kept_before;
    if (kept_x && ord < (unsigned long long)a.capacity) store_record(records + ord, pulse);
    if (valid) {
      const unsigned long long s = ord + (unsigned long long)kept_x;
      ti->slot = s < (unsigned long long)a.capacity ? int(s) : a.capacity;
    }
    n_pulses += (unsigned long long)kept_all;
  }

  if (my_on) atomicAdd(&l.cnt[0], my_on);
  if (my_short) atomicAdd(&l.cnt[1], my_short);
  if (my_nan) atomicAdd(&l.cnt[2], my_nan);
  __syncthreads();
  if (tid == 0) {
    sum->n_total += (unsigned long long)n;
    sum->n_on += l.cnt[0];
    sum->n_short += l.cnt[1];
    sum->n_nan += l.cnt[2];
    sum->n_pulses = n_pulses;
    sum->n_lost = n_pulses > (unsigned long long)a.capacity ? n_pulses - (unsigned long long)a.capacity : 0ull;
    const bool on = state == ON;
    sum->open = on ? 1 : 0;
    sum->open_toa = on ? carry.toa : 0;
    sum->open_width = on ? carry.width : 0;
    store_record(a.open + c, on ? carry : run_empty());
    // the stream's last sample, for the pair that crosses into the next launch
    const size_t unit = a.fmt == 2 ? 8 : 2;
    const char* sb = static_cast<const char*>(a.in) + size_t(c) * a.in_stride * unit;
    float2 q;
    if (a.fmt == 1) {
      const uchar2 v = reinterpret_cast<const uchar2*>(sb)[n - 1];
      q = make_float2(float(double(v.x) / 127.5 - 1.0), float(double(v.y) / 127.5 - 1.0));
    } else {
      q = unpack_iq(a.fmt, sb, n - 1, nullptr);
    }
    a.prev[2 * c + (a.parity ^ 1)] = q;
  }
}

}  // namespace

hipError_t launch_pulse(const PulseLaunch& a, hipStream_t s, int* launches) {
  if (launches) *launches = 0;
  if (a.n == 0 || a.C <= 0) return hipSuccess;
  const size_t unit = a.fmt == 2 ? 8 : 2;
  const int tiles_most = a.max_launch_tiles / a.C > 0 ? a.max_launch_tiles / a.C : 1;     // per stream and launch
  const size_t step = size_t(tiles_most) * size_t(kPulseTile);
  int parity = a.parity;
  for (size_t off = 0; off < a.n; off += step) {
    PulseLaunch b = a;
    b.in = static_cast<const char*>(a.in) + off * unit;
    b.n = a.n - off < step ? a.n - off : step;
    b.base = a.base + (long long)off;
    b.parity = parity;
    const size_t tiles = (b.n + kPulseTile - 1) / kPulseTile;
    const unsigned gx = unsigned(tiles);
    if (a.passes & 1) hipLaunchKernelGGL(pulse_tile_kernel<false>, dim3(gx, unsigned(a.C)), dim3(kPulseThreads), 0, s, b);
    if (a.passes & 2) hipLaunchKernelGGL(pulse_stitch_kernel, dim3(unsigned(a.C)), dim3(kPulseThreads), 0, s, b);
    if (a.passes & 4) hipLaunchKernelGGL(pulse_tile_kernel<true>, dim3(gx, unsigned(a.C)), dim3(kPulseThreads), 0, s, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    parity ^= 1;
    if (launches) ++*launches;
  }
  return hipSuccess;
}

}  // namespace tdsa
