// tdsa_capi_corr.cpp - tdsa_corr_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_corr.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_corr_record) == sizeof(CorrRecord) && sizeof(tdsa_corr_record) == 32, "the public record is the kernel's");
static_assert(sizeof(tdsa_corr_summary) == sizeof(CorrSummary) && sizeof(tdsa_corr_summary) == 56, "the public summary is the kernel's");
static_assert(offsetof(tdsa_corr_record, metric) == 8 && offsetof(tdsa_corr_record, c1_re) == 16 &&
                  offsetof(tdsa_corr_record, c2_im) == 28 && offsetof(tdsa_corr_summary, n_bad) == 40 &&
                  offsetof(tdsa_corr_summary, flushed) == 48,
              "record and summary layout");
static_assert(TDSA_CORR_MAX_STREAMS == kCorrMaxStreams && TDSA_CORR_MAX_RECORDS == kCorrMaxRecords && TDSA_CORR_MIN_REF == kCorrMinRef &&
                  TDSA_CORR_MAX_REF == kCorrMaxRef && TDSA_CORR_MAX_DISTANCE == kCorrMaxDistance && TDSA_CORR_TILE == kCorrTile &&
                  TDSA_CORR_WINDOWS_PER_THREAD == kCorrWindowsPerThread && TDSA_CORR_MAX_LAUNCH_TILES == kCorrMaxLaunchTiles,
              "the public constants are the kernel's");
static_assert(kCorrRingEntryBytes == sizeof(float) * 2 + sizeof(float4), "a ring entry is m, e and the four components of c1, c2");

// ---- correlation search (tdsa_corr.hip) ----------------------------------------------------------------------------
struct tdsa_corr_s : IqAccum {
  int capacity = 1;
  long long trace = 0;             // K, after the cap
  int L = 0, W = 0;
  float threshold = 1.0f, e_ref = 1.0f;
  Dev<float2> d_ref;               // [kCorrMaxRef]
  Dev<float2> d_hist;              // [2][C][kCorrMaxRef]
  Dev<CorrSummary> d_sum;          // [C]
  Dev<CorrRecord> d_rec;           // [C][capacity]
  Dev<float> d_ring_m;             // the ring and the scratch of the match passes: sized by configure for its min_distance
  Dev<float> d_ring_e;
  Dev<float4> d_ring_c;
  Dev<unsigned> d_bmax;
  Dev<int> d_cnt;
  Dev<unsigned long long> d_bits;
  size_t ring = 0, blocks = 0;     // entries / blocks per stream in use
  long long seen = 0;              // samples per stream since the last reset
  long long decided = 0;           // windows decided
  int parity = 0;
  bool flushed = false;
  int max_launch_tiles = kCorrMaxLaunchTiles, passes = 15, variant = 0;

  long long windows(long long samples) const { return samples >= L ? samples - L + 1 : 0; }
  // samples per stream of a launch at the most
  size_t step(int tiles) const { return size_t(tiles / C > 0 ? tiles / C : 1) * size_t(kCorrTile); }

  CorrLaunch launch_args() const {
    CorrLaunch a;
    a.C = C;
    a.L = L;
    a.W = W;
    a.threshold = threshold;
    a.e_ref = e_ref;
    a.capacity = capacity;
    a.max_launch_tiles = max_launch_tiles;
    a.passes = passes;
    a.variant = variant;
    a.ring_mask = unsigned(ring - 1);
    a.ref = d_ref;
    a.hist = d_hist;
    a.ring_m = d_ring_m;
    a.ring_e = d_ring_e;
    a.ring_c = d_ring_c;
    a.bmax = d_bmax;
    a.tile_cnt = d_cnt;
    a.tile_bits = d_bits;
    a.blocks = int(blocks);
    a.sum = d_sum;
    a.records = d_rec;
    return a;
  }

  // the launches of one call on stream s over device samples; does not wait.  A launch that fails leaves the cuts
  // before it enqueued and counted: the streams are undefined until a reset, as the header says of TDSA_ERR_HIP
  int run(hipStream_t s, int fmt, const void* in, size_t n_in, size_t in_stride) {
    const size_t unit = size_t(bytes_per_sample(fmt));
    const size_t most = step(max_launch_tiles);
    TRY(order(s));
    for (size_t off = 0; off < n_in; off += most) {
      CorrLaunch a = launch_args();
      a.in = static_cast<const char*>(in) + off * unit;
      a.fmt = fmt;
      a.n = int(n_in - off < most ? n_in - off : most);
      a.in_stride = in_stride;
      a.s0 = seen;
      a.w0 = windows(seen);
      a.w1 = windows(seen + a.n);
      a.d0 = decided;
      a.d1 = a.w1 - W > decided ? a.w1 - W : decided;
      a.parity = parity;
      HIPCHK(launch_corr(a, s));
      seen += a.n;
      decided = a.d1;
      parity ^= 1;
    }
    TRY(done(s));
    return TDSA_OK;
  }
};

namespace {

constexpr IqNames kNames = {"correlator", "correlation search takes"};

size_t pow2_at_least(size_t v) {
  size_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// the state as no sample has touched it, enqueued on the handle's own stream behind the last launch; returns when
// earlier calls have finished.  The ring and the records are left: the counters say what of them counts
int corr_clear(tdsa_corr_s* h) {
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_sum, 0, size_t(h->C) * sizeof(CorrSummary), h->stream));
  HIPCHK(hipMemsetAsync(h->d_hist, 0, size_t(2) * size_t(h->C) * kCorrMaxRef * sizeof(float2), h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->seen = 0;
  h->decided = 0;
  h->parity = 0;
  h->flushed = false;
  return TDSA_OK;
}

int params_check(float threshold, int min_distance) {
  if (!(threshold > 0.0f && threshold <= 1.0f)) return fail(TDSA_ERR_ARG, "threshold=%g: above 0 and at most 1", double(threshold));
  if (min_distance < 1 || min_distance > kCorrMaxDistance)
    return fail(TDSA_ERR_ARG, "min_distance=%d: 1 .. %d", min_distance, kCorrMaxDistance);
  return TDSA_OK;
}

// E_r of a reference that passes, in *e_ref
int ref_check(const void* ref, int len, float* e_ref) {
  if (len < kCorrMinRef || len > kCorrMaxRef) return fail(TDSA_ERR_ARG, "ref_len=%d: %d .. %d", len, kCorrMinRef, kCorrMaxRef);
  if (!ref) return fail(TDSA_ERR_ARG, "null reference");
  const float* r = static_cast<const float*>(ref);
  double e = 0.0;
  for (int k = 0; k < 2 * len; ++k) {
    if (!std::isfinite(r[k])) return fail(TDSA_ERR_ARG, "reference sample %d is not finite", k / 2);
    e += double(r[k]) * double(r[k]);
  }
  const float ef = float(e);
  if (!(ef > 0.0f && std::isfinite(ef))) return fail(TDSA_ERR_ARG, "reference energy %g: finite and above 0", e);
  *e_ref = ef;
  return TDSA_OK;
}

// the ring and the scratch of the match passes for min_distance W; the stream is idle
int corr_size(tdsa_corr_s* h, int W) {
  const size_t most = h->step(kCorrMaxLaunchTiles);
  const size_t ring = pow2_at_least(most + 2 * size_t(W) + 2 * size_t(kCorrBlock) + size_t(h->trace));
  const size_t blocks = (most + 2 * size_t(W)) / size_t(kCorrBlock) + 4;
  const size_t C = size_t(h->C);
  TRY(h->d_ring_m.grow(C * ring, nullptr));
  TRY(h->d_ring_e.grow(C * ring, nullptr));
  TRY(h->d_ring_c.grow(C * ring, nullptr));
  TRY(h->d_bmax.grow(C * blocks, nullptr));
  TRY(h->d_cnt.grow(C * blocks, nullptr));
  TRY(h->d_bits.grow(4 * C * blocks, nullptr));
  h->ring = ring;
  h->blocks = blocks;
  return TDSA_OK;
}

int ref_upload(tdsa_corr_s* h, const void* ref, int len, float e_ref) {
  TRY(h->own_stream());
  HIPCHK(hipStreamSynchronize(h->stream));   // no launch reads the old reference any more
  HIPCHK(hipMemcpy(h->d_ref, ref, size_t(len) * sizeof(float2), hipMemcpyHostToDevice));
  h->L = len;
  h->e_ref = e_ref;
  return TDSA_OK;
}

}  // namespace

int tdsa_corr_create(int device_id, int streams, int capacity, int64_t trace, size_t max_host_samples, const void* ref_c64,
                     int ref_len, tdsa_corr* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (streams < 1 || streams > kCorrMaxStreams) return fail(TDSA_ERR_ARG, "streams=%d: 1 .. %d", streams, kCorrMaxStreams);
  if (capacity < 1 || (long long)streams * capacity > kCorrMaxRecords)
    return fail(TDSA_ERR_ARG, "capacity=%d: at least 1, streams * capacity at most %lld", capacity, kCorrMaxRecords);
  if (trace < 0) return fail(TDSA_ERR_ARG, "trace=%lld: not negative", (long long)trace);
  if (max_host_samples < size_t(streams))
    return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least one sample per stream (%d)", max_host_samples, streams);
  float e_ref = 0.0f;
  TRY(ref_check(ref_c64, ref_len, &e_ref));
  HIPCHK(hipSetDevice(device_id));
  tdsa_corr h = new (std::nothrow) tdsa_corr_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->C = streams;
  h->capacity = capacity;
  const long long most = kCorrTraceBytes / (kCorrRingEntryBytes * (long long)streams);
  h->trace = trace < most ? (long long)trace : most;
  h->max_host = max_host_samples;
  h->W = ref_len;
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->in.alloc(max_host_samples * 8);
  if (e == hipSuccess) e = h->d_ref.alloc(size_t(kCorrMaxRef));
  if (e == hipSuccess) e = h->d_hist.alloc(size_t(2) * size_t(streams) * kCorrMaxRef);
  if (e == hipSuccess) e = h->d_sum.alloc(size_t(streams));
  if (e == hipSuccess) e = h->d_rec.alloc(size_t(streams) * size_t(capacity));
  if (e != hipSuccess) {
    (void)tdsa_corr_destroy(h);
    return fail(TDSA_ERR_HIP, "correlator create: %s", hipGetErrorString(e));
  }
  int rc = ref_upload(h, ref_c64, ref_len, e_ref);
  if (rc == TDSA_OK) rc = corr_size(h, h->W);
  if (rc == TDSA_OK) rc = corr_clear(h);
  if (rc != TDSA_OK) {
    (void)tdsa_corr_destroy(h);
    return rc;
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_corr_destroy(tdsa_corr h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_corr_set_reference(tdsa_corr h, const void* ref_c64, int ref_len) {
  float e_ref = 0.0f;
  TRY(ref_check(ref_c64, ref_len, &e_ref));
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  TRY(ref_upload(h, ref_c64, ref_len, e_ref));
  return corr_clear(h);
}

int tdsa_corr_configure(tdsa_corr h, float threshold, int min_distance) {
  TRY(params_check(threshold, min_distance));
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  TRY(corr_clear(h));              // the stream is idle: the ring may move
  TRY(corr_size(h, min_distance));
  h->threshold = threshold;
  h->W = min_distance;
  return TDSA_OK;
}

int tdsa_corr_reset(tdsa_corr h) {
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  return corr_clear(h);
}

static int flushed_check(tdsa_corr h) {
  if (h && h->flushed) return fail(TDSA_ERR_ARG, "the correlator was flushed: it takes no samples until tdsa_corr_reset");
  return TDSA_OK;
}

int tdsa_corr_process(tdsa_corr h, int in_format, const void* in_host, size_t n_in, size_t in_stride) {
  TRY(IqAccum::check(h, kNames, in_format, in_host, n_in, in_stride, false));
  TRY(flushed_check(h));
  return IqAccum::host(h, kNames, in_format, in_host, n_in, in_stride);
}

int tdsa_corr_process_dev(tdsa_corr h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride) {
  TRY(IqAccum::check(h, kNames, in_format, in_dev, n_in, in_stride, true));
  TRY(flushed_check(h));
  return IqAccum::dev(h, kNames, p, in_format, in_dev, n_in, in_stride);   // no wait: the state stays on the device until _read
}

int tdsa_corr_flush(tdsa_corr h) {
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  if (h->flushed) return TDSA_OK;
  TRY(h->own_stream());
  CorrLaunch a = h->launch_args();
  a.in = nullptr;
  a.fmt = TDSA_IN_C64;
  a.n = 0;
  a.s0 = h->seen;
  a.w0 = a.w1 = h->windows(h->seen);
  a.d0 = h->decided;
  a.d1 = a.w1;
  a.parity = h->parity;
  a.flush = 1;
  HIPCHK(launch_corr(a, h->stream));
  TRY(h->done(h->stream));
  h->decided = a.d1;
  h->flushed = true;
  return TDSA_OK;
}

int tdsa_corr_read(tdsa_corr h, int first_stream, int n_streams, tdsa_corr_record* records_host, tdsa_corr_summary* summaries_host) {
  if (!summaries_host) return fail(TDSA_ERR_ARG, "null summaries");
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  TRY(h->stream_range(first_stream, n_streams));
  TRY(h->own_stream());            // behind the last launch, whichever stream it went on
  HIPCHK(hipMemcpyAsync(summaries_host, h->d_sum + first_stream, size_t(n_streams) * sizeof(CorrSummary), hipMemcpyDeviceToHost,
                        h->stream));
  if (records_host)
    HIPCHK(hipMemcpyAsync(records_host, h->d_rec + size_t(first_stream) * size_t(h->capacity),
                          size_t(n_streams) * size_t(h->capacity) * sizeof(CorrRecord), hipMemcpyDeviceToHost, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return TDSA_OK;
}

int tdsa_corr_read_trace(tdsa_corr h, int stream, int64_t first, int64_t count, float* m_out, void* c_out_c64) {
  if (first < 0 || count < 0) return fail(TDSA_ERR_ARG, "first=%lld, count=%lld: not negative", (long long)first, (long long)count);
  if (count > 0 && !m_out) return fail(TDSA_ERR_ARG, "null m_out");
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  if (stream < 0 || stream >= h->C) return fail(TDSA_ERR_ARG, "stream=%d: inside the handle's %d", stream, h->C);
  const long long have = h->windows(h->seen);
  const long long from = have > h->trace ? have - h->trace : 0;
  if (first < from || count > have - first || first > have)
    return fail(TDSA_ERR_ARG, "windows %lld .. %lld: the trace holds %lld .. %lld", (long long)first, (long long)(first + count - 1),
                from, have - 1);
  if (count == 0) return TDSA_OK;
  TRY(h->own_stream());
  std::vector<float4> cc(c_out_c64 ? size_t(count) : 0);
  const size_t mask = h->ring - 1;
  for (long long k = 0; k < count;) {          // the range wraps around the ring once at the most
    const size_t at = size_t(first + k) & mask;
    const size_t run = size_t(count - k) < h->ring - at ? size_t(count - k) : h->ring - at;
    HIPCHK(hipMemcpyAsync(m_out + k, h->d_ring_m + size_t(stream) * h->ring + at, run * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (c_out_c64)
      HIPCHK(hipMemcpyAsync(cc.data() + k, h->d_ring_c + size_t(stream) * h->ring + at, run * sizeof(float4), hipMemcpyDeviceToHost,
                            h->stream));
    k += (long long)run;
  }
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float* c = static_cast<float*>(c_out_c64);
  for (size_t k = 0; k < cc.size(); ++k) {     // c = fl(c1 + c2): one IEEE addition per component, here as on the device
    const volatile float re = cc[k].x + cc[k].z, im = cc[k].y + cc[k].w;
    c[2 * k] = re;
    c[2 * k + 1] = im;
  }
  return TDSA_OK;
}

int tdsa_corr_debug_limits(tdsa_corr h, int max_launch_tiles, int passes, int variant) {
  if (!h) return fail(TDSA_ERR_ARG, "null correlator");
  if (max_launch_tiles < h->C || max_launch_tiles > kCorrMaxLaunchTiles)
    return fail(TDSA_ERR_ARG, "max_launch_tiles=%d: streams (%d) .. %d", max_launch_tiles, h->C, kCorrMaxLaunchTiles);
  if (passes < 0 || passes > 15) return fail(TDSA_ERR_ARG, "passes=%d: a mask of four bits", passes);
  if (variant < 0 || variant > 7) return fail(TDSA_ERR_ARG, "variant=%d: 0 .. 7", variant);
  h->max_launch_tiles = max_launch_tiles;
  h->passes = passes;
  h->variant = variant;
  return TDSA_OK;
}

int tdsa_corr_timer_begin(tdsa_corr h) { return Lane::timer_begin(h, kNames.handle); }

int tdsa_corr_timer_end(tdsa_corr h, float* elapsed_ms) { return Lane::timer_end(h, kNames.handle, elapsed_ms); }
