// tdsa_capi_eye.cpp - tdsa_eye_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_eye.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_eye_clock) == sizeof(EyeClock), "the public clock is the kernel's");
static_assert(TDSA_EYE_IQ == kEyeIq && TDSA_EYE_FM == kEyeFm && TDSA_EYE_REAL == kEyeReal, "the kinds are the kernel's");
static_assert(TDSA_EYE_MAX_BINS == kEyeMaxBins && TDSA_EYE_TOTALS == kEyeTotals, "the public constants are the kernel's");

// ---- eye diagrams (tdsa_eye.hip) -----------------------------------------------------------------------------------
// The state is one device block: counts[2][kEyeMaxBins] uint64 (the configured eyes H P of them in use, back to back),
// then totals[kEyeTotals].  The clocks of a call go through one of two pinned blocks and one of two device blocks of
// max_segments clocks each, taken in turn: a call waits only for the call before the last, whose kernel read the pair
// it is about to overwrite.
struct tdsa_eye_s : Lane {
  size_t max_host = 0;             // samples one host call stages
  int max_seg = 0;
  int num_cu = 256;
  Dev<float2> d_nco;               // [kSegNcoTable]
  Staging in;                      // of a host block, 8 bytes a sample at most
  Dev<unsigned long long> d_state;
  Pinned<EyeClock> h_clk[2];
  Dev<EyeClock> d_clk[2];
  hipEvent_t ev_clk[2] = {nullptr, nullptr};
  bool clk_busy[2] = {false, false};
  int clk_next = 0;
  Dev<char> d_tr;                  // the traces of a host call, grown on demand ...
  Pinned<char> h_tr;
  bool configured = false;
  uint64_t step = 0;
  int kind = kEyeIq, boxcar = 1, log2p = 5, rows = 128;
  float lo = -1.0f, scale = 64.0f;

  static constexpr size_t kStateWords = 2 * size_t(kEyeMaxBins) + kEyeTotals;
  unsigned long long* d_totals() const { return d_state + 2 * size_t(kEyeMaxBins); }
  size_t in_unit() const { return kind == kEyeReal ? sizeof(float) : sizeof(float2); }
  size_t trace_unit() const { return kind == kEyeIq ? sizeof(float2) : sizeof(float); }
  size_t bins() const { return size_t(eye_count(kind)) * (size_t(rows) << log2p); }

  // the state as no segment has touched it, enqueued on the handle's own stream behind the last launch; waits
  int clear() {
    TRY(own_stream());
    HIPCHK(hipMemsetAsync(d_state, 0, kStateWords * 8, stream));
    TRY(done(stream));
    HIPCHK(hipStreamSynchronize(stream));
    return TDSA_OK;
  }

  // one call on stream s, which the caller has put behind the last launch; does not wait for the kernel
  int run(hipStream_t s, const void* in, size_t seg_len, size_t hop, int n_seg, const tdsa_eye_clock* clocks, void* traces, int K) {
    const int slot = clk_next;
    if (clk_busy[slot]) HIPCHK(hipEventSynchronize(ev_clk[slot]));   // the call before the last has read this pair
    std::memcpy(h_clk[slot], clocks, size_t(n_seg) * sizeof(EyeClock));
    HIPCHK(hipMemcpyAsync(d_clk[slot], h_clk[slot], size_t(n_seg) * sizeof(EyeClock), hipMemcpyHostToDevice, s));
    EyeLaunch a;
    a.in = in;
    a.seg_len = (long long)seg_len;
    a.hop = (long long)hop;
    a.n_seg = n_seg;
    a.kind = kind;
    a.step = step;
    a.boxcar = boxcar;
    a.log2p = log2p;
    a.rows = rows;
    a.lo = lo;
    a.scale = scale;
    a.K = K;
    a.clocks = d_clk[slot];
    a.nco = d_nco;
    a.traces = traces;
    a.counts = d_state;
    a.totals = d_totals();
    a.num_cu = num_cu;
    HIPCHK(launch_eye(a, s));
    HIPCHK(hipEventRecord(ev_clk[slot], s));
    clk_busy[slot] = true;
    clk_next = slot ^ 1;
    TRY(done(s));
    return TDSA_OK;
  }
};

namespace {

constexpr const char* kWho = "eye diagram handle";

int eye_check_kind(int kind) {
  if (kind != TDSA_EYE_IQ && kind != TDSA_EYE_FM && kind != TDSA_EYE_REAL)
    return fail(TDSA_ERR_ARG, "kind=%d: TDSA_EYE_IQ, _FM or _REAL", kind);
  return TDSA_OK;
}
int eye_check_boxcar(int boxcar) {
  if (boxcar < 1 || boxcar > kEyeMaxBoxcar) return fail(TDSA_ERR_ARG, "boxcar=%d: 1 .. %d samples", boxcar, kEyeMaxBoxcar);
  return TDSA_OK;
}

// The checks both entry points share, in one order: null handle, not configured, null samples, null clocks, alignment,
// n_seg, hop, K, the clocks.  None of them makes a HIP call.
int eye_check(const tdsa_eye_s* h, const void* in, size_t seg_len, size_t hop, int n_seg, const tdsa_eye_clock* clocks,
              const void* traces, bool dev, int* K_out) {
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  if (!h->configured) return fail(TDSA_ERR_STATE, "not configured: call tdsa_eye_configure first");
  if (!in) return fail(TDSA_ERR_ARG, "null samples");
  if (!clocks) return fail(TDSA_ERR_ARG, "null clocks");
  if (dev && reinterpret_cast<uintptr_t>(in) % h->in_unit() != 0)
    return fail(TDSA_ERR_ARG, "input pointer must be aligned to one %s (%zu bytes)",
                h->kind == kEyeReal ? "float32" : "complex64 sample", h->in_unit());
  if (reinterpret_cast<uintptr_t>(clocks) % 8 != 0) return fail(TDSA_ERR_ARG, "clocks must be aligned to 8 bytes");
  if (dev && reinterpret_cast<uintptr_t>(traces) % h->trace_unit() != 0)
    return fail(TDSA_ERR_ARG, "traces pointer must be aligned to one %s (%zu bytes)",
                h->kind == kEyeIq ? "complex64 point" : "float32", h->trace_unit());
  if (n_seg < 1 || n_seg > h->max_seg)
    return fail(TDSA_ERR_ARG, "n_seg=%d: 1 .. %d (the handle's max_segments)", n_seg, h->max_seg);
  if (hop < 1) return fail(TDSA_ERR_ARG, "hop=%zu: at least one sample", hop);
  const long long K = eye_symbols_per_segment(h->step, seg_len, h->kind, h->boxcar);
  if (K < kEyeMinSymbols || K > kSegMaxSymbols)
    return fail(TDSA_ERR_ARG, "seg_len=%zu gives %lld symbols per segment: %d .. %d", seg_len, K, kEyeMinSymbols, kSegMaxSymbols);
  for (int s = 0; s < n_seg; ++s) {
    const uint64_t d = clocks[s].delta_fx;
    if (d != 0 && (d < kSegOne || d >= h->step + kSegOne))
      return fail(TDSA_ERR_ARG, "clock of segment %d: delta_fx=%llu: 0 (skip) or 2^32 <= delta_fx < step + 2^32", s,
                  (unsigned long long)d);
  }
  *K_out = int(K);
  return TDSA_OK;
}

}  // namespace

int tdsa_eye_symbols_per_segment(uint64_t step, size_t seg_len, int kind, int boxcar, int* K) {
  if (!K) return fail(TDSA_ERR_ARG, "null K");
  TRY(SegAnalyser::check_step(step));
  TRY(eye_check_kind(kind));
  TRY(eye_check_boxcar(boxcar));
  *K = SegAnalyser::clamp_k(eye_symbols_per_segment(step, seg_len, kind, boxcar));
  return TDSA_OK;
}

int tdsa_eye_create(int device_id, size_t max_host_samples, int max_segments, tdsa_eye* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (max_host_samples < 16) return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least 16", max_host_samples);
  if (max_segments < 1) return fail(TDSA_ERR_ARG, "max_segments=%d: at least 1", max_segments);
  HIPCHK(hipSetDevice(device_id));
  {
    const hipError_t e = eye_allow_lds();
    if (e != hipSuccess)
      return fail(TDSA_ERR_HIP, "eye create: the device refuses %d bytes of LDS per workgroup: %s",
                  kEyeMaxLdsBytes - kEyeStaticLdsBytes, hipGetErrorString(e));
  }
  tdsa_eye h = new (std::nothrow) tdsa_eye_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->max_host = max_host_samples;
  h->max_seg = max_segments;
  const std::vector<float2> nco = SegAnalyser::nco_table();
  int cus = 0;
  hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id);
  if (e == hipSuccess && cus > 0) h->num_cu = cus;
  if (e == hipSuccess) e = h->open(true);
  if (e == hipSuccess) e = h->d_nco.alloc(kSegNcoTable);
  if (e == hipSuccess) e = h->in.alloc(max_host_samples * sizeof(float2));
  if (e == hipSuccess) e = h->d_state.alloc(tdsa_eye_s::kStateWords);
  for (int i = 0; i < 2; ++i) {
    if (e == hipSuccess) e = h->h_clk[i].alloc(size_t(max_segments), hipHostMallocDefault);
    if (e == hipSuccess) e = h->d_clk[i].alloc(size_t(max_segments));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_clk[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_nco, nco.data(), kSegNcoTable * sizeof(float2), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->d_state, 0, tdsa_eye_s::kStateWords * 8, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the host copy of the table is released
  if (e != hipSuccess) {
    (void)tdsa_eye_destroy(h);
    return fail(TDSA_ERR_HIP, "eye create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_eye_destroy(tdsa_eye h) {
  if (!h) return TDSA_OK;
  h->drain();
  for (hipEvent_t ev : h->ev_clk)
    if (ev) (void)hipEventDestroy(ev);
  delete h;
  return TDSA_OK;
}

int tdsa_eye_configure(tdsa_eye h, uint64_t step, int kind, int boxcar, int points, int rows, float lo, float hi) {
  TRY(SegAnalyser::check_step(step));
  TRY(eye_check_kind(kind));
  TRY(eye_check_boxcar(boxcar));
  int log2p = 0;
  while ((1 << log2p) < points && log2p < 8) ++log2p;
  if (points < kEyeMinPoints || points > kEyeMaxPoints || (1 << log2p) != points)
    return fail(TDSA_ERR_ARG, "points=%d: 4, 8, 16, 32 or 64 per symbol", points);
  if (rows < kEyeMinRows || rows > kEyeMaxRows) return fail(TDSA_ERR_ARG, "rows=%d: %d .. %d", rows, kEyeMinRows, kEyeMaxRows);
  if (points * rows > kEyeMaxBins)
    return fail(TDSA_ERR_ARG, "points=%d x rows=%d = %d bins: at most %d", points, rows, points * rows, kEyeMaxBins);
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
    return fail(TDSA_ERR_ARG, "range %g .. %g: finite, lo < hi", double(lo), double(hi));
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  TRY(h->clear());                 // the clock, the series and the rows decide every point's bin: the state starts again
  h->step = step;
  h->kind = kind;
  h->boxcar = boxcar;
  h->log2p = log2p;
  h->rows = rows;
  h->lo = lo;
  h->scale = float(double(rows) / (double(hi) - double(lo)));
  h->configured = true;
  return TDSA_OK;
}

int tdsa_eye_reset(tdsa_eye h) {
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  return h->clear();
}

int tdsa_eye_process(tdsa_eye h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                     const tdsa_eye_clock* clocks_host, void* traces_host) {
  int K = 0;
  TRY(eye_check(h, in_host, seg_len, hop, n_seg, clocks_host, traces_host, false, &K));
  // hop first, so that the product below cannot wrap
  if (seg_len > n_samples || (n_seg > 1 && hop > (n_samples - seg_len) / (size_t(n_seg) - 1)))
    return fail(TDSA_ERR_ARG, "%d segments of %zu samples every %zu need %zu samples, the block has %zu", n_seg, seg_len, hop,
                (size_t(n_seg) - 1) * hop + seg_len, n_samples);
  if (n_samples > h->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", n_samples, h->max_host);
  TRY(h->own_stream());
  const size_t seg_bytes = (size_t(K - 2) << h->log2p) * h->trace_unit(), tr_bytes = size_t(n_seg) * seg_bytes;
  if (traces_host) {
    TRY(h->d_tr.grow(tr_bytes, h->stream));
    TRY(h->h_tr.grow(tr_bytes, h->stream));
  }
  // the previous host call has waited: the staging is free
  TRY(h->in.fill(h->stream, in_host, 1, n_samples, n_samples, h->in_unit()));
  TRY(h->run(h->stream, h->in.d_in, seg_len, hop, n_seg, clocks_host, traces_host ? h->d_tr : nullptr, K));
  if (traces_host) HIPCHK(hipMemcpyAsync(h->h_tr, h->d_tr, tr_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t s = 0; traces_host && s < size_t(n_seg); ++s)
    if (clocks_host[s].delta_fx != 0)   // a skipped segment's traces are left untouched
      std::memcpy(static_cast<char*>(traces_host) + s * seg_bytes, static_cast<const char*>(h->h_tr) + s * seg_bytes, seg_bytes);
  return TDSA_OK;
}

int tdsa_eye_process_dev(tdsa_eye h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                         const tdsa_eye_clock* clocks_host, void* traces_dev) {
  int K = 0;
  TRY(eye_check(h, in_dev, seg_len, hop, n_seg, clocks_host, traces_dev, true, &K));
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", kWho);
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  TRY(h->order(s));
  return h->run(s, in_dev, seg_len, hop, n_seg, clocks_host, traces_dev, K);   // no wait: the state stays on the device until _read
}

int tdsa_eye_read(tdsa_eye h, uint64_t* counts_host, uint64_t* totals_host) {
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  if (!h->configured) return fail(TDSA_ERR_STATE, "not configured: call tdsa_eye_configure first");
  if (!counts_host) return fail(TDSA_ERR_ARG, "null counts");
  if (!totals_host) return fail(TDSA_ERR_ARG, "null totals");
  TRY(h->own_stream());            // behind the last launch, whichever stream it went on
  HIPCHK(hipMemcpyAsync(counts_host, h->d_state, h->bins() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(totals_host, h->d_totals(), kEyeTotals * 8, hipMemcpyDeviceToHost, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return TDSA_OK;
}

int tdsa_eye_timer_begin(tdsa_eye h) { return Lane::timer_begin(h, kWho); }

int tdsa_eye_timer_end(tdsa_eye h, float* elapsed_ms) { return Lane::timer_end(h, kWho, elapsed_ms); }
