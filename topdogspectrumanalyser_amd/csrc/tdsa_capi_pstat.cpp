// tdsa_capi_pstat.cpp - tdsa_pstat_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_pstat.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_pstat_record) == sizeof(PstatRecord) && sizeof(tdsa_pstat_record) == 72,
              "the public record is the kernel's");
static_assert(TDSA_PSTAT_MAX_STREAMS == kPstatMaxStreams && TDSA_PSTAT_BINS == kPstatBins &&
                  TDSA_PSTAT_BINS_PER_OCTAVE == kPstatBinsPerOctave && TDSA_PSTAT_EXPONENTS == kPstatExponents &&
                  TDSA_PSTAT_EXP_LO_MIN == kPstatExpLoMin && TDSA_PSTAT_EXP_LO_MAX == kPstatExpLoMax,
              "the public constants are the kernel's");

// ---- power statistics (tdsa_pstat.hip) ---------------------------------------------------------------------------
struct tdsa_pstat_s : IqAccum {
  Dev<PstatRecord> d_rec;          // the state: [C] records, [C][256] mantissa sums, [C][2048] counts
  Dev<unsigned long long> d_msum;
  Dev<unsigned long long> d_hist;
  std::vector<PstatRecord> fresh;  // [C] what a reset writes: zeros, min_bits all ones
  int exp_lo = -40;
  float gate = 0.0f;

  // one launch on stream s over device samples; does not wait
  int run(hipStream_t s, int fmt, const void* in, size_t n_in, size_t in_stride) {
    PstatLaunch a;
    a.in = in;
    a.fmt = fmt;
    a.C = C;
    a.n = n_in;
    a.in_stride = in_stride;
    a.bin_base = (exp_lo + 127) << 5;
    a.gate = gate;
    a.rec = d_rec;
    a.msum = d_msum;
    a.hist = d_hist;
    TRY(order(s));
    HIPCHK(launch_pstat(a, s));
    TRY(done(s));
    return TDSA_OK;
  }
};

namespace {

constexpr IqNames kNames = {"power statistics handle", "power statistics take"};

// the state as no sample has touched it, enqueued on the handle's own stream behind the last launch
int pstat_clear(tdsa_pstat_s* h) {
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_msum, 0, size_t(h->C) * kPstatExponents * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->d_hist, 0, size_t(h->C) * kPstatBins * 8, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_rec, h->fresh.data(), size_t(h->C) * sizeof(PstatRecord), hipMemcpyHostToDevice, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // earlier calls have finished; `fresh` is read
  return TDSA_OK;
}

}  // namespace

int tdsa_pstat_create(int device_id, int streams, size_t max_host_samples, tdsa_pstat* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (streams < 1 || streams > kPstatMaxStreams) return fail(TDSA_ERR_ARG, "streams=%d: 1 .. %d", streams, kPstatMaxStreams);
  if (max_host_samples < size_t(streams))
    return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least one sample per stream (%d)", max_host_samples, streams);
  HIPCHK(hipSetDevice(device_id));
  tdsa_pstat h = new (std::nothrow) tdsa_pstat_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->C = streams;
  h->max_host = max_host_samples;
  PstatRecord zero{};
  zero.min_bits = 0xffffffffu;
  h->fresh.assign(size_t(streams), zero);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->in.alloc(max_host_samples * 8);
  if (e == hipSuccess) e = h->d_rec.alloc(size_t(streams));
  if (e == hipSuccess) e = h->d_msum.alloc(size_t(streams) * kPstatExponents);
  if (e == hipSuccess) e = h->d_hist.alloc(size_t(streams) * kPstatBins);
  if (e != hipSuccess) {
    (void)tdsa_pstat_destroy(h);
    return fail(TDSA_ERR_HIP, "pstat create: %s", hipGetErrorString(e));
  }
  const int rc = pstat_clear(h);
  if (rc != TDSA_OK) {
    (void)tdsa_pstat_destroy(h);
    return rc;
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_pstat_destroy(tdsa_pstat h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_pstat_configure(tdsa_pstat h, int exp_lo, float gate) {
  if (exp_lo < kPstatExpLoMin || exp_lo > kPstatExpLoMax)
    return fail(TDSA_ERR_ARG, "exp_lo=%d: %d .. %d", exp_lo, kPstatExpLoMin, kPstatExpLoMax);
  if (!std::isfinite(gate) || gate < 0.0f) return fail(TDSA_ERR_ARG, "gate=%g: finite and not negative (0 = off)", double(gate));
  if (!h) return fail(TDSA_ERR_ARG, "null power statistics handle");
  TRY(pstat_clear(h));             // the window and the gate decide every sample's class: the state starts again
  h->exp_lo = exp_lo;
  h->gate = gate;
  return TDSA_OK;
}

int tdsa_pstat_reset(tdsa_pstat h) {
  if (!h) return fail(TDSA_ERR_ARG, "null power statistics handle");
  return pstat_clear(h);
}

int tdsa_pstat_process(tdsa_pstat h, int in_format, const void* in_host, size_t n_in, size_t in_stride) {
  return IqAccum::host(h, kNames, in_format, in_host, n_in, in_stride);
}

int tdsa_pstat_process_dev(tdsa_pstat h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride) {
  return IqAccum::dev(h, kNames, p, in_format, in_dev, n_in, in_stride);   // no wait: the state stays on the device until _read
}

int tdsa_pstat_read(tdsa_pstat h, int first_stream, int n_streams, tdsa_pstat_record* records_host, uint64_t* msum_host,
                    uint64_t* hist_host) {
  if (!records_host) return fail(TDSA_ERR_ARG, "null records");
  if (!h) return fail(TDSA_ERR_ARG, "null power statistics handle");
  TRY(h->stream_range(first_stream, n_streams));
  TRY(h->own_stream());            // behind the last launch, whichever stream it went on
  const size_t a = size_t(first_stream), n = size_t(n_streams);
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec + a, n * sizeof(PstatRecord), hipMemcpyDeviceToHost, h->stream));
  if (msum_host)
    HIPCHK(hipMemcpyAsync(msum_host, h->d_msum + a * kPstatExponents, n * kPstatExponents * 8, hipMemcpyDeviceToHost, h->stream));
  if (hist_host)
    HIPCHK(hipMemcpyAsync(hist_host, h->d_hist + a * kPstatBins, n * kPstatBins * 8, hipMemcpyDeviceToHost, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return TDSA_OK;
}

int tdsa_pstat_timer_begin(tdsa_pstat h) { return Lane::timer_begin(h, kNames.handle); }

int tdsa_pstat_timer_end(tdsa_pstat h, float* elapsed_ms) { return Lane::timer_end(h, kNames.handle, elapsed_ms); }
