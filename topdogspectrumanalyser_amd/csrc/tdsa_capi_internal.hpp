// tdsa_capi_internal.hpp - what the translation units of the C-ABI layer (tdsa_capi_*.cpp, one per handle type or
// concern) share: error reporting, the status macros, the host idioms they all use, the few functions that cross files,
// the plan itself, and - at the end, because they need the plan - Lane, the base of the handle types: their stream,
// their lifetime, the timer entry points, and the one rule that orders a handle's launches whichever stream each goes
// on.  Over Lane stand four bases, each with the checks of a call and both entry points: Feed for the streaming filters
// (down-converter, channelizer, demodulator: taps, history, input count), IqAccum for the accumulators over IQ streams
// (power statistics, pulse analysis, correlation search), RowAnalyser for the analysers of dB rows (signal detection, channel
// measurements: the records grown on demand and the tail of a call) and SegAnalyser for the analysers of segments
// (symbol recovery, FSK analysis: the symbol clock, the staged outputs, create and destroy).  All four stage a host
// block through Staging.  Every device buffer and pinned block of the plan, the handles and the bases is a Dev<T> or a
// Pinned<T> (tdsa_capi_mem.hpp): pointer and capacity under one name, freed by the destructor of what holds them, so a
// destroy is drain() and delete and names no buffer.  The public face of the library is include/tdsa_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/tdsa_hip.h"
#include "tdsa_kernels.hpp"
#include "tdsa_seg.hpp"

namespace tdsa {
#pragma GCC visibility push(hidden)

// writes the text tdsa_last_error_string returns (one thread_local buffer: tdsa_capi_plan.cpp) and hands `code` back
int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return tdsa::fail(TDSA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// a status that is not TDSA_OK leaves the function as it is
#define TRY(expr)                              \
  do {                                         \
    const int rc_try_ = (expr);                \
    if (rc_try_ != TDSA_OK) return rc_try_;    \
  } while (0)

#pragma GCC visibility pop
}  // namespace tdsa
#include "tdsa_capi_mem.hpp"   // Dev<T>, Pinned<T>: who owns memory here (over fail and HIPCHK)
namespace tdsa {
#pragma GCC visibility push(hidden)

// Order the plan's main stream after everything in flight on the auxiliary streams.  Every entry point
// that touches plan state or enqueues on the main stream calls this first; work it enqueues afterwards
// is in turn waited for by the next overlapped launch (state_dirty).
int join_streams(tdsa_plan p);
#define JOIN(p) TRY(tdsa::join_streams(p))

// a consumer with a stream of its own (histogram, waterfall, constellation) behind the rows the plan has in flight:
// the plan's main stream signals, `consumer` waits
int plan_order_before(tdsa_plan p, hipStream_t consumer);

// of a format its caller has range-checked (TDSA_IN_I8 .. _C64, zero span: .. _F32R)
inline int bytes_per_sample(int fmt) { return fmt == TDSA_IN_C64 ? 8 : fmt == TDSA_IN_F32R ? 4 : 2; }

// how a raw sample of an input format becomes a float: (float(byte ^ its byte of xor_mask) - off) * scale; complex64 as is
struct InFormat {
  unsigned xor_mask;
  float off, scale;
};
inline InFormat in_format_consts(int fmt) {
  if (fmt == TDSA_IN_I8) return {0x80808080u, 128.0f, 1.0f / 128.0f};
  if (fmt == TDSA_IN_U8) return {0u, 127.5f, 1.0f / 127.5f};
  return {0u, 0.0f, 1.0f};
}

constexpr size_t kPinnedBounceMax = size_t(1) << 20;    // host calls up to 1 MiB each way go through pinned bounce buffers
constexpr size_t kZeroCopyMax = size_t(256) << 10;       // ... and up to 256 KiB in + out are read / written in place by the kernels

inline bool avg_active(const tdsa_mode& m) { return m.avg_mode != TDSA_AVG_OFF && m.avg_n > 1; }

// plan tables (tdsa_capi_plan.cpp): exp(-2 pi i k / n), k < n, evaluated in double, rounded once ...
std::vector<float2> unit_circle(int n);
// ... and the seeds of the column pass's twiddles of an n = 2^log2n point long transform ([big_seed_rows][16384])
std::vector<float2> seed_table(int n, int log2n);
// a host table into a device buffer of its own
template <class T>
int upload(const std::vector<T>& v, Dev<T>& dst) {
  HIPCHK(dst.alloc(v.size()));
  HIPCHK(hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return TDSA_OK;
}

// tdsa_capi_process.cpp
struct SegInfo;
int process_dev_impl(tdsa_plan p, int in_format, const void* iq_dev, size_t n_samples, int hop, int n_frames,
                     float* out_db_dev, hipEvent_t before, hipEvent_t after, const SegInfo* seg = nullptr);
int ensure_pins(tdsa_plan p, size_t in_bytes, size_t out_bytes);
int launch_spectrum_profiled(tdsa_plan p, int in_c64, const SpecParams& sp, const LaunchGeom& g, hipStream_t s = nullptr);
AvgParams avg_params(tdsa_plan p, const float* lin, int n_frames, int n, float* out_db);
int avg_use_ranges(tdsa_plan p, AvgParams& ap, int n_frames, hipStream_t s);
void avg_advance(tdsa_plan p, int n_frames);

// tdsa_capi_big.cpp
int process_big(tdsa_plan p, int in_format, const void* iq_dev, int hop, int n_frames, float* out_db_dev);
int big_materialize_mean(tdsa_plan p);

// tdsa_capi_chirp.cpp
struct ChirpPost;
int chirp_plan_init(tdsa_plan p);
int chirp_transform(tdsa_plan p, const void* in, int in_format, long long stride, int n_frames, const float2* dc_sub,
                    unsigned xor_mask, float in_off, const ChirpPost* post = nullptr);
int process_chirp(tdsa_plan p, int in_format, const void* iq_dev, int hop, int n_frames, float* out_db_dev);
int smooth_radices(int n, int* radix);

#pragma GCC visibility pop
}  // namespace tdsa

struct tdsa_plan_s {
  int device = 0, nfft = 0, log2n = 0, max_frames = 0, num_cu = 256;
  hipStream_t stream = nullptr;
  // tdsa_set_overlap: extra streams consecutive order-independent launches rotate over, so the ragged
  // tail of one persistent launch (and the inter-kernel gap) is filled by the head of the next
  static constexpr int kMaxOverlap = 4;
  hipStream_t aux[kMaxOverlap - 1] = {};
  hipEvent_t ev_aux[kMaxOverlap - 1] = {};
  hipEvent_t ev_state = nullptr;
  int n_overlap = 1, rr = 0;
  int overlap_share = 50;                // percent of the CUs an overlapped launch is sized for (3+ streams)
  bool aux_busy = false, state_dirty = true;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  tdsa_mode mode{};
  bool window_set = false;
  tdsa::Dev<float> d_window[3];   // window * input scale, per input format
  tdsa::Dev<float> d_window_perm[3];   // the same in the frame kernel's thread order (N >= 2048)
  tdsa::Dev<float2> d_tw;
  tdsa::Dev<float> d_hold_max;
  tdsa::Dev<float> d_hold_min;
  long long held_max = 0, held_min = 0;
  tdsa::Dev<double> d_avg;
  int avg_count = 0;
  tdsa::Dev<float> d_lin;                // [max_frames][N] linear power scratch (averaging modes)
  tdsa::Dev<double> d_carry;             // [chunks][N] chunk carries of the averager scan
  tdsa::Dev<float> d_agg;                // [grid][N] chunk aggregates formed by the frame kernel's workgroups (sizes >= 4096)
  tdsa::Dev<float> d_agg_w;              // [max_frames] weight of each frame in its workgroup's aggregate
  tdsa::Dev<double> d_chunk_a;           // [kAvgMaxWgChunks + 64] per chunk: product of its frames' multipliers
  tdsa::Dev<float> d_chunk_v;            // [kAvgMaxWgChunks + 64] per chunk: 1 = has frames
  long long agg_w_key[7] = {-1, -1, -1, -1, -1, -1, -1};   // (count, mode, n, frames, chunks, frames per unit, path) the weights in d_agg_w were made for
  tdsa::Dev<float2> d_cplx;              // [max_frames][N] complex spectra (real-input path)
  tdsa::Dev<float2> d_real;              // real-input path: the selected signal(s) as complex streams (two for stereo)
  tdsa::Dev<float> d_lin1;               // [max_frames][2][N/2+1] one-sided linear power (real-input path)
  tdsa::Dev<float> d_db1;                // same shape, dB
  tdsa::Dev<float2> d_dc_state;
  tdsa::Dev<float2> d_sums;
  tdsa::Dev<float2> d_dc_sub;
  tdsa::Dev<float> d_tare_base;
  tdsa::Dev<float> d_tare_acc;
  bool tare_active = false;
  int tare_count = 0;
  tdsa::Dev<char> d_in_stage;
  // pinned bounce buffers of the host entry points for small calls (the one-frame-per-GUI-tick case): a copy from / to
  // pageable memory costs ~10 us each way in the runtime's own staging, a memcpy through pinned memory ~2 us
  tdsa::Pinned<char> h_in_pin;
  tdsa::Pinned<char> h_out_pin;
  tdsa::Dev<float> d_out_stage;
  tdsa::Dev<float> d_trace_in;
  tdsa::Dev<float> d_trace_live;
  long long frames_seen = 0;             // frames processed since the last hold reset (nan_safe rule)
  tdsa::Dev<unsigned long long> d_dbg;   // TDSA_TIMELINE developer builds
  // long-frame plans, N = 2^15 .. 2^20 = N1 x 16384 (tdsa_big.hip)
  bool big = false;
  tdsa::Dev<float2> d_z;                 // [group][N1][16384] complex64 rows after the column pass
  tdsa::Dev<float> d_acc;                // [N1][16384] power sums of the current call (row pass output)
  tdsa::Dev<double> d_sum;               // [N] fftshift-ed sums over the segments averaged so far
  tdsa::Dev<char> d_welch;               // staging of tdsa_welch_export (one partial) / tdsa_welch_combine (all of them)
  tdsa::Dev<float> d_clock;              // scratch of tdsa_shader_clock
  bool big_mean_in_sum = false;          // Welch calls leave the running mean as d_sum / avg_count; d_avg is formed when someone asks
  tdsa::Dev<double> d_lin64;             // [N] fftshift-ed power of one frame (exp / capped lin averaging)
  tdsa::Dev<double> d_sums64;            // [max_frames][2] exact I / Q sums of the frames of a call
  tdsa::Dev<float2> d_tw_seed;           // [big_seed_rows][16384] per-column twiddle seeds of the column pass
  tdsa::Dev<float2> d_tw_row;            // W_16384^m : the row pass's twiddle table
  tdsa::Dev<float> d_ones;               // [16384] unit window for the row pass
  tdsa::BigWindow big_win[3] = {};             // the column pass's window per input format (tdsa_set_window: table or one value)
  int avg_wg_min = 128;                  // batches of more frames than this take the workgroup-chunk scan (tdsa_debug_knob "avg_wg_min")
  bool avg_f64_chunks = false;           // tdsa_debug_knob "avg_f64_chunks": always the scan over fixed 64-frame chunks with float64 aggregates
  // frame lengths made of 2, 3, 5 only (up to 10 000 points in one LDS pass, two passes above): mixed-radix FFT of exactly nfft points (tdsa_smooth.hip) for the
  // complex path; the plan stays a chirp-z plan for everything else (real input)
  bool smooth = false;
  int smooth_on = 1;                     // tdsa_debug_knob "smooth": 0 = such sizes run as chirp-z convolutions like every other
  int smooth_stages = 0;
  int smooth_radix[tdsa::kSmoothMaxStages] = {0};
  // ... above 10 000 points (up to 2^20): two passes, nfft = smooth_n1 * smooth_n2, both within the LDS limit
  int smooth_n1 = 0, smooth_n2 = 0;
  int smooth_stages2 = 0;
  int smooth_radix2[tdsa::kSmoothMaxStages] = {0};   // the stages of smooth_n2 (smooth_radix: those of smooth_n1)
  tdsa::Dev<float2> d_smooth_z;          // [max_frames][n1][n2] between the passes
  tdsa::Dev<float2> d_smooth_tw;         // [nfft] exp(-2 pi i k / nfft)
  int chirp_fuse_big = 1;                // tdsa_debug_knob "chirp_fuse_big": 0 = long chirp-z frames run chirp_pre / chirp_post as their own passes
  int chirp_single = 1;                  // tdsa_debug_knob "chirp_single": 0 = chirp-z plans run chirp_pre / two transforms / chirp_post as separate
                                         // kernels (M <= 16384; developer builds: two launches that carry the passes), separate row passes (M > 16384)
  int big_pre_wgs = 0;                   // developer builds, tdsa_debug_knob "big_pre_wgs": empty workgroups launched ahead of every column pass
  int big_group = 64;                    // segments per column-pass / row-pass round (one round for the K = 64 Welch capture)
  int big_fuse_gather = 0;               // tdsa_debug_knob "big_fuse_gather": 1 = Welch captures of one round run row pass + gather + finish as ONE
                                         // launch with a ticket queue (measured: profiles/r06_c5_fused_gather.txt)
  tdsa::Dev<char> d_bigq;                // the queue's counters (32 bytes, zeroed once; they only grow)
  unsigned long long bigq_tickets = 0, bigq_rows = 0;   // what the next launch starts from
  // frame lengths that are not a power of two (tdsa_chirp.hip): chirp-z on the m_fft-point frame kernel
  bool chirp = false;
  int m_fft = 0, log2m = 0;              // M = 2^log2m >= 2 nfft - 1
  bool chirp_big = false;                // M > 16384: the two M-point transforms run on the long-frame kernels (N1 x 16384)
  int chirp_split = 0;                   // frames above 2^19 points: H = ceil(N / 2); the convolution runs as four half-length
                                         // sub-convolutions of M = 2^20 points on rows [2F][M] (tdsa_chirp.hip)
  tdsa::Dev<float2> d_chirp_bm;          // [M] spectra of the filter segments b[m - H], b[m + H] (d_chirp_b: b[m]), split plans only
  tdsa::Dev<float2> d_chirp_bp;
  tdsa::Dev<float2> d_chirp_a;           // [nfft] a[n] = exp(-i pi n^2 / nfft)
  tdsa::Dev<float2> d_chirp_b;           // [M]    FFT_M of conj(a) wrapped around M
  tdsa::Dev<float2> d_chirp_aw[3];   // [nfft] window * input scale * a[n] per input format (M <= 16384: the
                                         // unpack / window / chirp pass rides the first transform's loads)
  tdsa::Dev<float2> d_u0;                // [max_frames][M] work rows (allocated on first use)
  tdsa::Dev<float2> d_u1;
  tdsa::Dev<char> d_scratch;             // grows on demand: results of tdsa_rows_stats / tdsa_rows_top_peaks
  // per-frame scalars (tdsa_set_frame_stats): the results of the last kFsKeep calls.  A call takes the next of ITS stream's
  // kFsKeep slots, so a slot is only ever rewritten by later work of the stream that wrote it (in order, no events between
  // the frame-kernel launches), and the last kFsKeep calls overall are always still there.
  static constexpr int kFsKeep = 4;
  struct FsSlot {
    tdsa::Dev<char> d_part;              // [frames][waves per frame] records of the frame kernel's STATS epilogue
    tdsa::Dev<float> d_peak;             // [frames]
    tdsa::Dev<int> d_bin;
    tdsa::Dev<double> d_band;
    int n_frames = 0;
    int state = 0;                       // 0: nothing, 1: results (in flight on `stream`), 2: the call produced no rows to take them from
    bool pending = false;                // the frame kernel's records are there, frame_stats_finish_kernel has not run yet
    int wpf = 1;
    double cal_lin = 1.0;
    hipStream_t stream = nullptr;
  } fs[kMaxOverlap][kFsKeep];
  unsigned fs_count[kMaxOverlap] = {};   // calls that took a slot, per stream
  FsSlot* fs_hist[kFsKeep] = {};         // the slots of the last calls, newest at fs_seq - 1
  bool fs_on = false;
  int fs_lo = 1, fs_hi = 0;              // band: inclusive display-bin range, lo > hi = none
  unsigned long long fs_seq = 0;         // calls that left (or tried to leave) statistics
  hipStream_t fs_stream = nullptr;       // folds and reads back a slot
  bool profiling = false;
  bool sync_call = false;                // set by the synchronous host entry points around their device call
  std::vector<hipEvent_t> prof_events;   // pairs (begin, end) around frame-kernel launches
  size_t prof_used = 0;
};

namespace tdsa {
#pragma GCC visibility push(hidden)

// The base of the handle types: a device, a stream of the handle's own and what creates, drains and destroys them.
//
// The down-converter, the sweep assembler, zero span and the history also launch on a producer plan's stream, and ONE
// rule keeps their state coherent when it moves between streams: a handle's launches are totally ordered through
// ev_done, whichever stream each goes on.  Every launch on a stream s is bracketed by order(s) and done(s): s first
// waits for ev_done if the last launch went elsewhere, and afterwards ev_done stands for this one.  The handles that
// wait for their stream in every call (constellation, density, waterfall, trace) use device, stream and drain only;
// they go behind a producer with plan_order_before.
//
// A handle is deleted only after drain(), which also makes its device current: tdsa_<x>_destroy is null check, drain(),
// delete - also of a handle whose create failed half way.  The members of the derived handle, its buffers, go first;
// then ~Lane destroys the events and the stream.
struct Lane {
  int device = 0;
  hipStream_t stream = nullptr;    // the handle's own: host entry points, views, the timer
  hipEvent_t ev_done = nullptr;    // the last launch, on whichever stream it went
  hipStream_t last = nullptr;      // that stream
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // timer_begin / timer_end

  // create: the stream, ev_done and, for a handle with a timer, its two events
  hipError_t open(bool timer) {
    hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_done, hipEventDisableTiming);
    if (e == hipSuccess && timer) e = hipEventCreate(&ev_t0);
    if (e == hipSuccess && timer) e = hipEventCreate(&ev_t1);
    return e;
  }
  // before delete: nothing of the handle's is in flight any more, on any stream
  void drain() {
    (void)hipSetDevice(device);
    if (ev_done) (void)hipEventSynchronize(ev_done);
    if (stream) (void)hipStreamSynchronize(stream);
  }
  Lane() = default;
  Lane(const Lane&) = delete;
  Lane& operator=(const Lane&) = delete;
  // after the buffers: the events, then the stream
  ~Lane() {
    for (hipEvent_t ev : {ev_done, ev_t0, ev_t1})
      if (ev) (void)hipEventDestroy(ev);
    if (stream) (void)hipStreamDestroy(stream);
  }

  // order stream s behind the last launch if that went elsewhere
  int order(hipStream_t s) {
    if (last && last != s) HIPCHK(hipStreamWaitEvent(s, ev_done, 0));
    return TDSA_OK;
  }
  // the launch on s is the last one
  int done(hipStream_t s) {
    HIPCHK(hipEventRecord(ev_done, s));
    last = s;
    return TDSA_OK;
  }
  // the handle's own stream behind whatever ran last on another
  int own_stream() {
    HIPCHK(hipSetDevice(device));
    return order(stream);
  }
  // where a call fed by plan p launches: on the producer's main stream - ordered after everything the plan has in
  // flight, and the plan's later work after us - or without a plan on the handle's own
  int producer_stream(tdsa_plan p, hipStream_t* s) {
    HIPCHK(hipSetDevice(device));
    *s = stream;
    if (!p) return TDSA_OK;
    JOIN(p);
    *s = p->stream;
    return TDSA_OK;
  }

  // tdsa_<x>_timer_begin / _timer_end of a handle type that `who` names ("null <who>"): device time on the handle's
  // stream between the two calls; both first put it behind the last launch, so work that went on a plan's stream in
  // between is inside the interval
  static int timer_begin(Lane* h, const char* who) {
    if (!h) return fail(TDSA_ERR_ARG, "null %s", who);
    TRY(h->own_stream());
    HIPCHK(hipEventRecord(h->ev_t0, h->stream));
    return TDSA_OK;
  }
  static int timer_end(Lane* h, const char* who, float* elapsed_ms) {
    if (!h) return fail(TDSA_ERR_ARG, "null %s", who);
    if (!elapsed_ms) return fail(TDSA_ERR_ARG, "null elapsed_ms");
    TRY(h->own_stream());
    HIPCHK(hipEventRecord(h->ev_t1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev_t1));
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev_t0, h->ev_t1));
    return TDSA_OK;
  }
};

// The staging of a synchronous host entry point: a pinned block and the device block it is copied to.  The host call
// that filled it has waited for its stream before it returned, so the next one finds it free.
struct Staging {
  Pinned<char> h_in;
  Dev<char> d_in;

  // create, inside the chain that began with open()
  hipError_t alloc(size_t bytes) {
    const hipError_t e = h_in.alloc(bytes, hipHostMallocDefault);
    return e == hipSuccess ? d_in.alloc(bytes) : e;
  }
  // `rows` rows of n units of `unit` bytes, row r at in + r * stride units, back to back into h_in; then one copy to
  // d_in, enqueued on s
  int fill(hipStream_t s, const void* in, size_t rows, size_t n, size_t stride, size_t unit) {
    const size_t row = n * unit;
    for (size_t r = 0; r < rows; ++r)
      std::memcpy(h_in + r * row, static_cast<const char*>(in) + r * stride * unit, row);
    HIPCHK(hipMemcpyAsync(d_in, h_in, rows * row, hipMemcpyHostToDevice, s));
    return TDSA_OK;
  }
};

// What the messages of a streaming filter call it: "null <handle>", "the <noun> takes ...", "tdsa_<prefix>_set_taps".
struct FeedNames {
  const char *handle, *noun, *prefix;
};

// One process call of a streaming filter, as both entry points see it: `in_rows` rows of n_in samples of in_unit bytes
// each, row r at in + r * in_stride samples, and out_rows rows of out_unit-byte outputs at out + r * out_stride.
// in_align / out_align: what the pointer must be a multiple of, in bytes; 0 for a host pointer that is only memcpy'd.
struct FeedCall {
  int fmt = TDSA_IN_C64;      // of the input; a filter that takes complex64 rows only leaves it
  const void* in = nullptr;
  size_t n_in = 0, in_stride = 0, in_rows = 1, in_unit = 8;
  unsigned in_align = 0;
  void* out = nullptr;
  size_t out_stride = 0, out_rows = 1, out_unit = 8;
  unsigned out_align = 0;
  size_t* n_out = nullptr;
};

// The base of the streaming filters (down-converter, channelizer, demodulator) over Lane: a decimating FIR fed in
// pieces, one output per D inputs, output m from the call that delivers input m D.  It owns the zero-padded tap table,
// the ping-pong pair of history buffers and which half is current, the count of inputs since the last reset, and the
// pinned and device staging of the synchronous host entry point.  A filter supplies its kernel's launch struct (the
// callable of enqueue), its FeedCall, whatever set_taps makes it recompute, and state of its own, which it clears next
// to clear() and flips with `cur`.
//
// The checks of a call come in ONE order, for both entry points of every filter (check): what needs no handle - format,
// pointer alignment, in_stride - then null handle, null n_out, null samples, null output when outputs complete,
// out_stride, "no taps"; host() adds the block size after them, dev() the plan's device.
//
// clear() only enqueues; reset and set_taps wait for the stream after it, so both return with the stream idle.
struct Feed : Lane {
  int D = 1;                          // inputs per output
  int max_taps = 1, n_taps = 0;
  size_t taps_len = 0;                // floats of d_taps: the filter's padded [rows][row length]
  Dev<float> d_taps;                  // zero beyond n_taps
  Dev<char> d_hist[2];                // hist_bytes each, ping-pong
  size_t hist_bytes = 0;
  int cur = 0;
  long long n_total = 0;              // inputs (per row) since the last reset
  size_t max_host = 0;                // samples, all rows together, one host call stages
  Staging in;                         // of a host block, rows back to back ...
  Dev<char> d_out;                    // ... and of its outputs
  Pinned<char> h_out;

  long long m_first() const { return (n_total + D - 1) / D; }   // the next output
  size_t outputs(size_t n_in) const { return size_t((n_total + (long long)n_in + D - 1) / D - m_first()); }

  // create, in the chain that began with open(); D, max_taps, taps_len, hist_bytes and max_host are set.  A host call
  // brings at most max_host / in_rows samples per row, which complete at most that / D + 1 outputs per row.
  hipError_t alloc(size_t in_rows, size_t out_rows, size_t out_unit) {
    const size_t ob = ((max_host / in_rows) / size_t(D) + 1) * out_rows * out_unit;
    hipError_t e = d_taps.alloc(taps_len);
    if (e == hipSuccess) e = d_hist[0].alloc(hist_bytes);
    if (e == hipSuccess) e = d_hist[1].alloc(hist_bytes);
    if (e == hipSuccess) e = in.alloc(max_host * 8);
    if (e == hipSuccess) e = d_out.alloc(ob);
    if (e == hipSuccess) e = h_out.alloc(ob, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(d_taps, 0, taps_len * sizeof(float), stream);
    return e;
  }

  // zero history and input count, enqueued on the handle's own stream
  int clear() {
    TRY(own_stream());
    HIPCHK(hipMemsetAsync(d_hist[0], 0, hist_bytes, stream));
    HIPCHK(hipMemsetAsync(d_hist[1], 0, hist_bytes, stream));
    TRY(done(stream));
    n_total = 0;
    return TDSA_OK;
  }

  // new taps (tap k at float k of the padded table) and a clear(); on return the stream is idle and taps_host released
  int set_taps(const float* taps_host, int n) {
    if (!taps_host) return fail(TDSA_ERR_ARG, "null taps");
    if (n < 1 || n > max_taps) return fail(TDSA_ERR_ARG, "n_taps=%d: 1 .. %d (the handle's max_taps)", n, max_taps);
    for (int k = 0; k < n; ++k)
      if (!std::isfinite(taps_host[k])) return fail(TDSA_ERR_ARG, "tap %d is not finite", k);
    std::vector<float> pad(taps_len, 0.0f);
    std::memcpy(pad.data(), taps_host, size_t(n) * sizeof(float));
    TRY(own_stream());
    HIPCHK(hipMemcpyAsync(d_taps, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    n_taps = n;
    TRY(clear());
    HIPCHK(hipStreamSynchronize(stream));
    return TDSA_OK;
  }

  // One call on stream s: launch(m_first, n_out) enqueues the kernels over the n_out outputs the call completes, from
  // d_hist[cur] into d_hist[cur ^ 1], and returns a hipError_t.
  template <class Launch>
  int enqueue(hipStream_t s, size_t n_in, size_t* n_out, Launch&& launch) {
    *n_out = outputs(n_in);
    if (n_in == 0) return TDSA_OK;
    TRY(order(s));
    HIPCHK(launch(m_first(), (long long)*n_out));
    TRY(done(s));
    cur ^= 1;
    n_total += (long long)n_in;
    return TDSA_OK;
  }

  // the shared checks of a call, before any HIP call (f may be null: that is one of them)
  static int check(const Feed* f, const FeedNames& who, const FeedCall& c) {
    if (c.fmt != TDSA_IN_I8 && c.fmt != TDSA_IN_U8 && c.fmt != TDSA_IN_C64)
      return fail(TDSA_ERR_ARG, "in_format=%d: the %s takes complex IQ (TDSA_IN_I8 / _U8 / _C64)", c.fmt, who.noun);
    const auto unit = [](unsigned align) { return align == 8 ? "complex64 sample" : "float32"; };
    if (c.in_align && reinterpret_cast<uintptr_t>(c.in) % c.in_align != 0)
      return fail(TDSA_ERR_ARG, "input pointer must be aligned to one %s (%u bytes)", unit(c.in_align), c.in_align);
    if (c.out_align && reinterpret_cast<uintptr_t>(c.out) % c.out_align != 0)
      return fail(TDSA_ERR_ARG, "output pointer must be aligned to one %s (%u bytes)", unit(c.out_align), c.out_align);
    if (c.in_stride < c.n_in)
      return fail(TDSA_ERR_ARG, "in_stride=%zu: below the call's %zu samples per channel", c.in_stride, c.n_in);
    if (!f) return fail(TDSA_ERR_ARG, "null %s", who.handle);
    if (!c.n_out) return fail(TDSA_ERR_ARG, "null n_out");
    if (c.n_in > 0 && !c.in) return fail(TDSA_ERR_ARG, "null samples");
    const size_t n = f->outputs(c.n_in);
    if (n > 0 && !c.out) return fail(TDSA_ERR_ARG, "null output");
    if (c.out_stride < n)
      return fail(TDSA_ERR_ARG, "out_stride=%zu: the call completes %zu outputs per channel", c.out_stride, n);
    if (f->n_taps < 1) return fail(TDSA_ERR_STATE, "no taps: call tdsa_%s_set_taps first", who.prefix);
    return TDSA_OK;
  }

  // The two entry points.  run(s, in, in_stride, out, out_stride, n_out) is the filter's call on stream s over device
  // memory; it ends in enqueue.
  //
  // host: through the staging, rows back to back both ways, on the handle's own stream; returns when the outputs are
  // in the caller's memory
  template <class Run>
  static int host(Feed* f, const FeedNames& who, const FeedCall& c, Run&& run) {
    TRY(check(f, who, c));
    const size_t most = f->max_host / c.in_rows;
    if (c.n_in > most)
      return c.in_rows == 1
                 ? fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", c.n_in, most)
                 : fail(TDSA_ERR_ARG, "block of %zu samples per channel, the handle stages at most %zu (max_host_samples / "
                        "channels)", c.n_in, most);
    *c.n_out = 0;
    if (c.n_in == 0) return TDSA_OK;
    HIPCHK(hipSetDevice(f->device));
    TRY(f->in.fill(f->stream, c.in, c.in_rows, c.n_in, c.in_stride, c.in_unit));
    size_t n = 0;
    TRY(run(f->stream, static_cast<const void*>(f->in.d_in), c.n_in, f->d_out, f->outputs(c.n_in), &n));
    const size_t orow = n * c.out_unit;
    if (n) HIPCHK(hipMemcpyAsync(f->h_out, f->d_out, c.out_rows * orow, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    for (size_t r = 0; n && r < c.out_rows; ++r)
      std::memcpy(static_cast<char*>(c.out) + r * c.out_stride * c.out_unit, f->h_out + r * orow, orow);
    *c.n_out = n;
    return TDSA_OK;
  }
  // dev: in place, on plan p's stream (null: the handle's own), no host wait
  template <class Run>
  static int dev(Feed* f, const FeedNames& who, tdsa_plan p, const FeedCall& c, Run&& run) {
    TRY(check(f, who, c));
    if (p && p->device != f->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", who.noun);
    *c.n_out = 0;
    if (c.n_in == 0) return TDSA_OK;
    hipStream_t s;
    TRY(f->producer_stream(p, &s));
    return run(s, c.in, c.in_stride, c.out, c.out_stride, c.n_out);
  }
};

// What the messages of an accumulator over IQ streams call it: "null <handle>", "the <takes> complex IQ".
struct IqNames {
  const char *handle, *takes;
};

// The base of the accumulators over IQ streams (power statistics, pulse analysis, correlation search) over Lane: C streams of n_in samples
// each in I8, U8 or C64, stream c at in + c * in_stride samples.  Neither entry point leaves anything in the caller's
// memory: the state stays on the device until the handle's _read, and the device entry point does not wait.  A handle
// type H supplies its state and H::run(s, fmt, in, n_in, in_stride), its launches on stream s between order(s) and
// done(s).
//
// The checks of a call come in ONE order (check): format, alignment to one sample of a pointer that is read in place,
// null handle, null samples, in_stride; host() adds the block size after them, dev() the plan's device.
struct IqAccum : Lane {
  int C = 1;
  size_t max_host = 0;             // samples, all streams together, one host call stages
  Staging in;                      // of a host block, streams back to back

  static int check(const IqAccum* h, const IqNames& who, int fmt, const void* in, size_t n_in, size_t in_stride, bool dev) {
    if (fmt != TDSA_IN_I8 && fmt != TDSA_IN_U8 && fmt != TDSA_IN_C64)
      return fail(TDSA_ERR_ARG, "in_format=%d: the %s complex IQ (TDSA_IN_I8 / _U8 / _C64)", fmt, who.takes);
    if (dev && reinterpret_cast<uintptr_t>(in) % unsigned(bytes_per_sample(fmt)) != 0)
      return fail(TDSA_ERR_ARG, "input pointer must be aligned to one sample (%d bytes)", bytes_per_sample(fmt));
    if (!h) return fail(TDSA_ERR_ARG, "null %s", who.handle);
    if (n_in > 0 && !in) return fail(TDSA_ERR_ARG, "null samples");
    if (h->C > 1 && in_stride < n_in)
      return fail(TDSA_ERR_ARG, "in_stride=%zu: below the call's %zu samples per stream", in_stride, n_in);
    return TDSA_OK;
  }

  // host: through the staging on the handle's own stream; returns when the staging is free for the next host call
  template <class H>
  static int host(H* h, const IqNames& who, int fmt, const void* in, size_t n_in, size_t in_stride) {
    TRY(check(h, who, fmt, in, n_in, in_stride, false));
    const size_t most = h->max_host / size_t(h->C);
    if (n_in > most)
      return h->C == 1
                 ? fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", n_in, most)
                 : fail(TDSA_ERR_ARG, "block of %zu samples per stream, the handle stages at most %zu (max_host_samples / "
                        "streams)", n_in, most);
    if (n_in == 0) return TDSA_OK;
    TRY(h->own_stream());
    TRY(h->in.fill(h->stream, in, size_t(h->C), n_in, in_stride, size_t(bytes_per_sample(fmt))));
    TRY(h->run(h->stream, fmt, static_cast<const void*>(h->in.d_in), n_in, n_in));
    HIPCHK(hipStreamSynchronize(h->stream));
    return TDSA_OK;
  }
  // dev: in place, on plan p's stream (null: the handle's own), no host wait
  template <class H>
  static int dev(H* h, const IqNames& who, tdsa_plan p, int fmt, const void* in, size_t n_in, size_t in_stride) {
    TRY(check(h, who, fmt, in, n_in, in_stride, true));
    if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", who.handle);
    if (n_in == 0) return TDSA_OK;
    hipStream_t s;
    TRY(h->producer_stream(p, &s));
    return h->run(s, fmt, in, n_in, in_stride);
  }

  // the streams a _read names
  int stream_range(int first_stream, int n_streams) const {
    if (first_stream < 0 || n_streams < 1 || first_stream > C - n_streams)
      return fail(TDSA_ERR_ARG, "streams %d .. %d: inside the handle's %d", first_stream, first_stream + n_streams - 1, C);
    return TDSA_OK;
  }
};

// What the messages of an analyser of dB rows call it: "null <handle>", "tdsa_<prefix>_configure", "null <sub> records".
struct RowNames {
  const char *handle, *prefix, *sub;
};

// The base of the analysers of dB rows (signal detection, channel measurements) over Lane: n_rows rows of n_bins
// float32 back to back, and per call two kinds of records in the caller's memory, one per row and sub_per_row per row,
// through device buffers that grow on demand.  Both entry points return when the records have arrived.  A handle type H
// supplies H::launch(s, rows, n_rows), which enqueues its kernel on s and returns a hipError_t, and H::tally(row_host,
// n_rows), which reads the call's row records for the handle's second total.
//
// The checks of a call come in ONE order (check): null handle, not configured, null rows, the two null record pointers;
// host() adds the block size after them, dev() the alignment of the rows and the plan's device.
struct RowAnalyser : Lane {
  int n_bins = 0;
  size_t max_host = 0;             // rows one host call stages
  Staging in;
  Dev<char> d_row;                 // the records of either entry point ...
  Dev<char> d_sub;
  size_t row_unit = 0, sub_unit = 0, sub_per_row = 1;  // ... of so many bytes each; d_sub holds sub_per_row per row
  uint64_t rows_seen = 0;
  bool configured = false;

  // create, inside the chain that began with open(); n_bins and max_host are set
  hipError_t alloc() { return in.alloc(max_host * size_t(n_bins) * sizeof(float)); }

  static int check(const RowAnalyser* h, const RowNames& who, const void* rows, const void* row_rec, const void* sub_rec) {
    if (!h) return fail(TDSA_ERR_ARG, "null %s", who.handle);
    if (!h->configured) return fail(TDSA_ERR_ARG, "not configured: call tdsa_%s_configure first", who.prefix);
    if (!rows) return fail(TDSA_ERR_ARG, "null rows");
    if (!row_rec) return fail(TDSA_ERR_ARG, "null row records");
    if (!sub_rec) return fail(TDSA_ERR_ARG, "null %s records", who.sub);
    return TDSA_OK;
  }

  // one call on stream s, which the caller has put behind the last launch, over device rows
  template <class H, class R>
  static int run(H* h, hipStream_t s, const float* rows, size_t n_rows, R* row_host, void* sub_host) {
    TRY(h->d_row.grow(n_rows * h->row_unit, h->last));
    TRY(h->d_sub.grow(n_rows * h->sub_per_row * h->sub_unit, h->last));
    HIPCHK(h->launch(s, rows, n_rows));
    HIPCHK(hipMemcpyAsync(row_host, h->d_row, n_rows * h->row_unit, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sub_host, h->d_sub, n_rows * h->sub_per_row * h->sub_unit, hipMemcpyDeviceToHost, s));
    TRY(h->done(s));
    HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
    h->rows_seen += n_rows;
    h->tally(row_host, n_rows);
    return TDSA_OK;
  }

  // host: through the staging, on the handle's own stream
  template <class H, class R>
  static int host(H* h, const RowNames& who, const float* rows, size_t n_rows, R* row_host, void* sub_host) {
    TRY(check(h, who, rows, row_host, sub_host));
    if (n_rows > h->max_host)
      return fail(TDSA_ERR_ARG, "block of %zu rows, the handle stages at most %zu (max_host_rows)", n_rows, h->max_host);
    if (n_rows == 0) return TDSA_OK;
    TRY(h->own_stream());
    TRY(h->in.fill(h->stream, rows, 1, n_rows * size_t(h->n_bins), 0, sizeof(float)));
    return run(h, h->stream, h->in.d_in.template as<const float>(), n_rows, row_host, sub_host);
  }
  // dev: in place, on plan p's stream (null: the handle's own)
  template <class H, class R>
  static int dev(H* h, const RowNames& who, tdsa_plan p, const float* rows, size_t n_rows, R* row_host, void* sub_host) {
    TRY(check(h, who, rows, row_host, sub_host));
    if (reinterpret_cast<uintptr_t>(rows) % 4 != 0)
      return fail(TDSA_ERR_ARG, "rows_dev must be aligned to one float32 (4 bytes)");
    if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", who.handle);
    if (n_rows == 0) return TDSA_OK;
    hipStream_t s;
    TRY(h->producer_stream(p, &s));
    TRY(h->order(s));
    return run(h, s, rows, n_rows, row_host, sub_host);
  }
};

// What the messages of a segment analyser call it: "null <handle>", "tdsa_<prefix>_configure" and "<prefix> create",
// "TDSA_<mode>_AUTO or _FIXED", "null <out>".
struct SegNames {
  const char *handle, *prefix, *mode, *out;
};

static_assert(TDSA_SYMSYNC_AUTO == TDSA_FSK_AUTO && TDSA_SYMSYNC_FIXED == TDSA_FSK_FIXED, "one timing_mode for both");

// The base of the segment analysers (symbol recovery, FSK analysis) over Lane: n_seg segments of seg_len samples, `hop`
// apart, each with the symbol clock of _configure; per segment K outputs into rows out_stride wide, an optional second
// output of the same shape, and one record in the caller's memory, through a device buffer that grows on demand.  Both
// entry points return when the records have arrived.  A handle type H supplies
//   H::who, H::out_unit, H::aux_unit, H::rec_unit   its names; the bytes of an output of either kind and of a record
//   h->in_unit()                                    the bytes of an input sample
//   h->symbols(seg_len)                             its K, as a long long that may lie outside 2 .. kSegMaxSymbols
//   h->aligned(in, out, aux, rec)                   the alignment of a call's pointers, with its own messages
//   h->launch(s, in, seg_len, hop, n_seg, out, out_stride, aux, K)   its kernel on s, returning a hipError_t
// and, to create, what it does on the device before there is a handle.
//
// The checks of a call come in ONE order (check): null handle, not configured, null samples, null output, null
// records, alignment, n_seg, hop, K, out_stride; host() adds the block and the staging limit after them, dev() the
// plan's device.  None of them makes a HIP call.
struct SegAnalyser : Lane {
  size_t max_host = 0;             // samples one host call stages
  Dev<float2> d_nco;               // [kSegNcoTable]
  Staging in;                      // of a host block, 8 bytes a sample at most ...
  Dev<char> d_out;                 // ... of its outputs, [out_cap()] of out_unit bytes, then [out_cap()] of aux_unit ...
  Pinned<char> h_out;
  Dev<char> d_rec;                 // ... and of the records of either entry point, grown on demand
  bool configured = false;
  uint64_t step = 0, delta_fx = 0;
  uint32_t nu = 0;
  int fixed = 0;

  size_t out_cap() const { return max_host / 4 + 1; }   // K n_seg < seg_len n_seg / 4

  // (cos, -sin) of 2 pi k / 4096 from the first quarter turn, so that whole quarter turns are exact
  static std::vector<float2> nco_table() {
    std::vector<float2> nco(kSegNcoTable);
    const int q = kSegNcoTable / 4;
    for (int k = 0; k < kSegNcoTable; ++k) {
      const double th = 2.0 * 3.14159265358979323846 * double(k % q) / double(kSegNcoTable);
      const float c = k % q ? float(std::cos(th)) : 1.0f, s = k % q ? float(std::sin(th)) : 0.0f;
      const float cs[4] = {c, -s, -c, s}, sn[4] = {s, c, -s, -c};   // cos, sin of th + quarter turns
      nco[k] = make_float2(cs[k / q], -sn[k / q]);
    }
    return nco;
  }

  // tdsa_<x>_create; prepare() runs on the device before there is a handle and returns a status
  template <class H, class Prepare>
  static int create(int device_id, size_t max_host_samples, H** out, Prepare&& prepare) {
    if (!out) return fail(TDSA_ERR_ARG, "null out");
    *out = nullptr;
    if (max_host_samples < 16) return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least 16", max_host_samples);
    HIPCHK(hipSetDevice(device_id));
    TRY(prepare());
    H* h = new (std::nothrow) H();
    if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
    h->device = device_id;
    h->max_host = max_host_samples;
    const std::vector<float2> nco = nco_table();
    const size_t out_bytes = h->out_cap() * (H::out_unit + H::aux_unit);
    hipError_t e = h->open(true);
    if (e == hipSuccess) e = h->d_nco.alloc(kSegNcoTable);
    if (e == hipSuccess) e = h->in.alloc(max_host_samples * sizeof(float2));
    if (e == hipSuccess) e = h->d_out.alloc(out_bytes);
    if (e == hipSuccess) e = h->h_out.alloc(out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_nco, nco.data(), kSegNcoTable * sizeof(float2), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the host copy of the table is released
    if (e != hipSuccess) {
      (void)destroy(h);
      return fail(TDSA_ERR_HIP, "%s create: %s", H::who.prefix, hipGetErrorString(e));
    }
    *out = h;
    return TDSA_OK;
  }
  // tdsa_<x>_destroy, also of a handle whose create failed half way
  template <class H>
  static int destroy(H* h) {
    if (!h) return TDSA_OK;
    h->drain();
    delete h;
    return TDSA_OK;
  }

  // The clock of _configure and _symbols_per_segment.  A _configure checks step and nu, then its own arguments, then
  // the timing, and last hands the clock to the handle, which may be null.
  static int check_step(uint64_t step) {
    if (step < kSegMinStep || step > kSegMaxStep)
      return fail(TDSA_ERR_ARG, "step=%llu: 4 .. 64 samples per symbol in 32.32 fixed point", (unsigned long long)step);
    return TDSA_OK;
  }
  static int check_rate(uint64_t step, uint32_t nu) {
    TRY(check_step(step));
    const unsigned __int128 turn = (unsigned __int128)1 << 64;
    const uint64_t want = uint64_t((turn + step / 2) / step);   // round(2^32 / sps)
    if (uint64_t(nu) + 1 < want || uint64_t(nu) > want + 1)
      return fail(TDSA_ERR_ARG, "nu=%u: the phase step of this symbol rate is %llu", nu, (unsigned long long)want);
    return TDSA_OK;
  }
  static int check_timing(const SegNames& who, uint64_t step, int timing_mode, uint64_t delta_fx) {
    if (timing_mode != TDSA_SYMSYNC_AUTO && timing_mode != TDSA_SYMSYNC_FIXED)
      return fail(TDSA_ERR_ARG, "timing_mode=%d: TDSA_%s_AUTO or _FIXED", timing_mode, who.mode);
    if (timing_mode == TDSA_SYMSYNC_FIXED && (delta_fx < kSegOne || delta_fx >= step + kSegOne))
      return fail(TDSA_ERR_ARG, "delta_fx=%llu: 2^32 <= delta_fx < step + 2^32", (unsigned long long)delta_fx);
    return TDSA_OK;
  }
  static int set_clock(SegAnalyser* h, const SegNames& who, uint64_t step, uint32_t nu, int timing_mode, uint64_t delta_fx) {
    if (!h) return fail(TDSA_ERR_ARG, "null %s", who.handle);
    h->step = step;
    h->nu = nu;
    h->fixed = timing_mode == TDSA_SYMSYNC_FIXED;
    h->delta_fx = h->fixed ? delta_fx : 0;
    h->configured = true;
    return TDSA_OK;
  }
  // what _symbols_per_segment hands back of a K that may lie outside an int
  static int clamp_k(long long k) { return k < 0 ? 0 : k > 0x7fffffff ? 0x7fffffff : int(k); }

  // the checks both entry points share; *K_out = symbols per segment
  template <class H>
  static int check(const H* h, const void* in, size_t seg_len, size_t hop, int n_seg, const void* out, size_t out_stride,
                   const void* aux, const void* rec, int* K_out) {
    if (!h) return fail(TDSA_ERR_ARG, "null %s", H::who.handle);
    if (!h->configured) return fail(TDSA_ERR_STATE, "not configured: call tdsa_%s_configure first", H::who.prefix);
    if (!in) return fail(TDSA_ERR_ARG, "null samples");
    if (!out) return fail(TDSA_ERR_ARG, "null %s", H::who.out);
    if (!rec) return fail(TDSA_ERR_ARG, "null records");
    TRY(h->aligned(in, out, aux, rec));
    if (n_seg < 1) return fail(TDSA_ERR_ARG, "n_seg=%d: at least one segment", n_seg);
    if (hop < 1) return fail(TDSA_ERR_ARG, "hop=%zu: at least one sample", hop);
    const long long K = h->symbols(seg_len);
    if (K < 2 || K > kSegMaxSymbols)
      return fail(TDSA_ERR_ARG, "seg_len=%zu gives %lld symbols per segment: 2 .. %d", seg_len, K, kSegMaxSymbols);
    if (out_stride < size_t(K)) return fail(TDSA_ERR_ARG, "out_stride=%zu: a segment gives %lld symbols", out_stride, K);
    *K_out = int(K);
    return TDSA_OK;
  }

  // host: through the staging on the handle's own stream, the outputs K wide back to back on the way, the second
  // kind's behind the room of the first; returns when outputs and records are in the caller's memory
  template <class H>
  static int host(H* h, const void* in, size_t n_samples, size_t seg_len, size_t hop, int n_seg, void* out,
                  size_t out_stride, void* aux, void* rec) {
    int K = 0;
    TRY(check(h, in, seg_len, hop, n_seg, out, out_stride, aux, rec, &K));
    // hop first, so that the product below cannot wrap
    if (seg_len > n_samples || (n_seg > 1 && hop > (n_samples - seg_len) / (size_t(n_seg) - 1)))
      return fail(TDSA_ERR_ARG, "%d segments of %zu samples every %zu need %zu samples, the block has %zu", n_seg, seg_len,
                  hop, (size_t(n_seg) - 1) * hop + seg_len, n_samples);
    if (n_samples > h->max_host || size_t(n_seg) * seg_len > h->max_host)
      return fail(TDSA_ERR_ARG, "block of %zu samples in %d segments of %zu, the handle stages at most %zu "
                  "(max_host_samples)", n_samples, n_seg, seg_len, h->max_host);
    TRY(h->own_stream());
    TRY(h->d_rec.grow(size_t(n_seg) * H::rec_unit, h->stream));
    // the previous host call has waited: the staging is free
    TRY(h->in.fill(h->stream, in, 1, n_samples, n_samples, h->in_unit()));
    const size_t rows = size_t(n_seg) * size_t(K), aux_at = h->out_cap() * H::out_unit;
    HIPCHK(h->launch(h->stream, h->in.d_in, seg_len, hop, n_seg, h->d_out, size_t(K), aux ? h->d_out + aux_at : nullptr, K));
    TRY(h->done(h->stream));
    HIPCHK(hipMemcpyAsync(h->h_out, h->d_out, rows * H::out_unit, hipMemcpyDeviceToHost, h->stream));
    if (aux) HIPCHK(hipMemcpyAsync(h->h_out + aux_at, h->d_out + aux_at, rows * H::aux_unit, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(rec, h->d_rec, size_t(n_seg) * H::rec_unit, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t orow = size_t(K) * H::out_unit, arow = size_t(K) * H::aux_unit;
    for (size_t s = 0; s < size_t(n_seg); ++s) {
      std::memcpy(static_cast<char*>(out) + s * out_stride * H::out_unit, h->h_out + s * orow, orow);
      if (aux) std::memcpy(static_cast<char*>(aux) + s * out_stride * H::aux_unit, h->h_out + aux_at + s * arow, arow);
    }
    return TDSA_OK;
  }
  // dev: in place, on plan p's stream (null: the handle's own)
  template <class H>
  static int dev(H* h, tdsa_plan p, const void* in, size_t seg_len, size_t hop, int n_seg, void* out, size_t out_stride,
                 void* aux, void* rec) {
    int K = 0;
    TRY(check(h, in, seg_len, hop, n_seg, out, out_stride, aux, rec, &K));
    if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", H::who.handle);
    hipStream_t s;
    TRY(h->producer_stream(p, &s));
    TRY(h->order(s));
    TRY(h->d_rec.grow(size_t(n_seg) * H::rec_unit, h->last));
    HIPCHK(h->launch(s, in, seg_len, hop, n_seg, out, out_stride, aux, K));
    HIPCHK(hipMemcpyAsync(rec, h->d_rec, size_t(n_seg) * H::rec_unit, hipMemcpyDeviceToHost, s));
    TRY(h->done(s));
    HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
    return TDSA_OK;
  }
};

#pragma GCC visibility pop
}  // namespace tdsa
