// tdsa_capi_pulse.cpp - tdsa_pulse_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_pulse.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_pulse_record) == sizeof(PulseRecord) && sizeof(tdsa_pulse_record) == 64,
              "the public record is the kernel's");
static_assert(sizeof(tdsa_pulse_summary) == sizeof(PulseSummary) && sizeof(tdsa_pulse_summary) == 72,
              "the public summary is the kernel's");
static_assert(offsetof(tdsa_pulse_record, peak_bits) == 24 && offsetof(tdsa_pulse_record, energy) == 32 &&
                  offsetof(tdsa_pulse_record, acc_im) == 48 && offsetof(tdsa_pulse_summary, open_toa) == 48 &&
                  offsetof(tdsa_pulse_summary, open) == 64,
              "record and summary layout");
static_assert(TDSA_PULSE_MAX_STREAMS == kPulseMaxStreams && TDSA_PULSE_MAX_RECORDS == kPulseMaxRecords &&
                  TDSA_PULSE_TILE == kPulseTile && TDSA_PULSE_SAMPLES_PER_THREAD == kPulseSamplesPerThread,
              "the public constants are the kernel's");

// ---- pulse analysis (tdsa_pulse.hip) -----------------------------------------------------------------------------
struct tdsa_pulse_s : IqAccum {
  int capacity = 1;
  Dev<PulseTileInfo> d_tiles;         // the tile summaries of one launch ...
  Dev<PulseSummary> d_sum;         // ... and the state: [C] summaries, [C] open pulses, [C][2] last samples, [C][capacity] records
  Dev<PulseRecord> d_open;
  Dev<float2> d_prev;
  Dev<PulseRecord> d_rec;
  float on_level = 1.0f, off_level = 1.0f;
  long long min_width = 1;
  long long seen = 0;              // samples per stream since the last reset: the index of the next call's first
  int parity = 0;
  int max_launch_tiles = kPulseMaxLaunchTiles, passes = 7;

  // the launches of one call on stream s over device samples; does not wait
  int run(hipStream_t s, int fmt, const void* in, size_t n_in, size_t in_stride) {
    PulseLaunch a;
    a.in = in;
    a.fmt = fmt;
    a.C = C;
    a.n = n_in;
    a.in_stride = in_stride;
    a.base = seen;
    a.on_level = on_level;
    a.off_level = off_level;
    a.min_width = int(min_width);
    a.capacity = capacity;
    a.parity = parity;
    a.max_launch_tiles = max_launch_tiles;
    a.passes = passes;
    a.tiles = d_tiles;
    a.sum = d_sum;
    a.open = d_open;
    a.prev = d_prev;
    a.records = d_rec;
    TRY(order(s));
    int launches = 0;
    HIPCHK(launch_pulse(a, s, &launches));
    TRY(done(s));
    seen += (long long)n_in;
    parity ^= launches & 1;
    return TDSA_OK;
  }
};

namespace {

constexpr IqNames kNames = {"pulse handle", "pulse analysis takes"};

// the state as no sample has touched it, enqueued on the handle's own stream behind the last launch.  The records are
// left: n_pulses says how many of them count
int pulse_clear(tdsa_pulse_s* h) {
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_sum, 0, size_t(h->C) * sizeof(PulseSummary), h->stream));
  HIPCHK(hipMemsetAsync(h->d_open, 0, size_t(h->C) * sizeof(PulseRecord), h->stream));
  HIPCHK(hipMemsetAsync(h->d_prev, 0, size_t(h->C) * 2 * sizeof(float2), h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // earlier calls have finished
  h->seen = 0;
  h->parity = 0;
  return TDSA_OK;
}

int levels_check(float on_level, float off_level, long long min_width) {
  if (!(std::isfinite(on_level) && on_level > 0.0f))
    return fail(TDSA_ERR_ARG, "on_level=%g: a finite float32 above 0", double(on_level));
  if (!(off_level > 0.0f && off_level <= on_level))
    return fail(TDSA_ERR_ARG, "off_level=%g: above 0 and at most on_level=%g", double(off_level), double(on_level));
  if (min_width < 1 || min_width >= (1ll << 31)) return fail(TDSA_ERR_ARG, "min_width=%lld: 1 .. 2^31 - 1", min_width);
  return TDSA_OK;
}

}  // namespace

int tdsa_pulse_create(int device_id, int streams, int capacity, size_t max_host_samples, tdsa_pulse* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (streams < 1 || streams > kPulseMaxStreams) return fail(TDSA_ERR_ARG, "streams=%d: 1 .. %d", streams, kPulseMaxStreams);
  if (capacity < 1 || (long long)streams * capacity > kPulseMaxRecords)
    return fail(TDSA_ERR_ARG, "capacity=%d: at least 1, streams * capacity at most %lld", capacity, kPulseMaxRecords);
  if (max_host_samples < size_t(streams))
    return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least one sample per stream (%d)", max_host_samples, streams);
  HIPCHK(hipSetDevice(device_id));
  tdsa_pulse h = new (std::nothrow) tdsa_pulse_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->C = streams;
  h->capacity = capacity;
  h->max_host = max_host_samples;
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->in.alloc(max_host_samples * 8);
  if (e == hipSuccess) e = h->d_tiles.alloc(size_t(kPulseMaxLaunchTiles));
  if (e == hipSuccess) e = h->d_sum.alloc(size_t(streams));
  if (e == hipSuccess) e = h->d_open.alloc(size_t(streams));
  if (e == hipSuccess) e = h->d_prev.alloc(size_t(streams) * 2);
  if (e == hipSuccess) e = h->d_rec.alloc(size_t(streams) * size_t(capacity));
  if (e != hipSuccess) {
    (void)tdsa_pulse_destroy(h);
    return fail(TDSA_ERR_HIP, "pulse create: %s", hipGetErrorString(e));
  }
  const int rc = pulse_clear(h);
  if (rc != TDSA_OK) {
    (void)tdsa_pulse_destroy(h);
    return rc;
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_pulse_destroy(tdsa_pulse h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_pulse_configure(tdsa_pulse h, float on_level, float off_level, int64_t min_width) {
  TRY(levels_check(on_level, off_level, (long long)min_width));
  if (!h) return fail(TDSA_ERR_ARG, "null pulse handle");
  TRY(pulse_clear(h));             // the levels decide every sample's class: the state starts again
  h->on_level = on_level;
  h->off_level = off_level;
  h->min_width = (long long)min_width;
  return TDSA_OK;
}

int tdsa_pulse_reset(tdsa_pulse h) {
  if (!h) return fail(TDSA_ERR_ARG, "null pulse handle");
  return pulse_clear(h);
}

int tdsa_pulse_process(tdsa_pulse h, int in_format, const void* in_host, size_t n_in, size_t in_stride) {
  return IqAccum::host(h, kNames, in_format, in_host, n_in, in_stride);
}

int tdsa_pulse_process_dev(tdsa_pulse h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride) {
  return IqAccum::dev(h, kNames, p, in_format, in_dev, n_in, in_stride);   // no wait: the state stays on the device until _read
}

int tdsa_pulse_read(tdsa_pulse h, int first_stream, int n_streams, tdsa_pulse_summary* summaries_host) {
  if (!summaries_host) return fail(TDSA_ERR_ARG, "null summaries");
  if (!h) return fail(TDSA_ERR_ARG, "null pulse handle");
  TRY(h->stream_range(first_stream, n_streams));
  TRY(h->own_stream());            // behind the last launch, whichever stream it went on
  HIPCHK(hipMemcpyAsync(summaries_host, h->d_sum + first_stream, size_t(n_streams) * sizeof(PulseSummary), hipMemcpyDeviceToHost,
                        h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return TDSA_OK;
}

int tdsa_pulse_read_pulses(tdsa_pulse h, int stream, int first, int count, tdsa_pulse_record* records_host, int* n_out) {
  if (!n_out) return fail(TDSA_ERR_ARG, "null n_out");
  *n_out = 0;
  if (!h) return fail(TDSA_ERR_ARG, "null pulse handle");
  if (stream < 0 || stream >= h->C) return fail(TDSA_ERR_ARG, "stream=%d: inside the handle's %d", stream, h->C);
  if (first < 0 || count < 0) return fail(TDSA_ERR_ARG, "first=%d, count=%d: not negative", first, count);
  if (count > 0 && !records_host) return fail(TDSA_ERR_ARG, "null records");
  TRY(h->own_stream());
  PulseSummary s;
  HIPCHK(hipMemcpyAsync(&s, h->d_sum + stream, sizeof(s), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const long long stored = s.n_pulses < (unsigned long long)h->capacity ? (long long)s.n_pulses : h->capacity;
  const long long n = first >= stored ? 0 : stored - first < count ? stored - first : count;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(records_host, h->d_rec + size_t(stream) * size_t(h->capacity) + size_t(first),
                          size_t(n) * sizeof(PulseRecord), hipMemcpyDeviceToHost, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *n_out = int(n);
  return TDSA_OK;
}

int tdsa_pulse_debug_limits(tdsa_pulse h, int max_launch_tiles, int passes) {
  if (!h) return fail(TDSA_ERR_ARG, "null pulse handle");
  if (max_launch_tiles < h->C || max_launch_tiles > kPulseMaxLaunchTiles)
    return fail(TDSA_ERR_ARG, "max_launch_tiles=%d: streams (%d) .. %d", max_launch_tiles, h->C, kPulseMaxLaunchTiles);
  if (passes < 0 || passes > 7) return fail(TDSA_ERR_ARG, "passes=%d: a mask of three bits", passes);
  h->max_launch_tiles = max_launch_tiles;
  h->passes = passes;
  return TDSA_OK;
}

int tdsa_pulse_timer_begin(tdsa_pulse h) { return Lane::timer_begin(h, kNames.handle); }

int tdsa_pulse_timer_end(tdsa_pulse h, float* elapsed_ms) { return Lane::timer_end(h, kNames.handle, elapsed_ms); }
