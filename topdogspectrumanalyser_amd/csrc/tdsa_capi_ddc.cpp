// tdsa_capi_ddc.cpp - tdsa_ddc_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_ddc.hpp"

using namespace tdsa;

// ---- zoom front end: digital down-conversion (tdsa_ddc.hip) ------------------------------------------------------
struct tdsa_ddc_s : Feed {
  int max_phases = kDdcBlock, phases = kDdcBlock;
  Dev<float2> d_nco;                  // [kDdcNcoTable]
  // the base's d_taps: [max_phases][D], tap q D + r at q * D + r; d_hist: [max_phases * D] mixed inputs (float2) each
  uint32_t p_b = 0, step = 0;         // NCO: p[n] = p_b + (n - n_b) step (mod 2^32)
  long long n_b = 0;
};

namespace {

const FeedNames kDdc = {"ddc", "down-converter", "ddc"};

uint32_t ddc_phase_at(const tdsa_ddc d, long long n) {
  return d->p_b + uint32_t(uint64_t(n - d->n_b)) * d->step;
}

// zero history, input count and phase (the step is kept)
int ddc_clear(tdsa_ddc d) {
  TRY(d->clear());
  d->n_b = 0;
  d->p_b = 0;
  return TDSA_OK;
}

// both process entry points: FIR of the outputs the call completes, then the history for the next call
int ddc_process(tdsa_ddc d, tdsa_plan p, bool host, int fmt, const void* in, size_t n_in, void* out, size_t* n_out) {
  FeedCall c;
  c.fmt = fmt;
  c.in = in;
  c.n_in = c.in_stride = n_in;
  c.in_unit = size_t(bytes_per_sample(fmt));
  c.out = out;
  c.out_stride = size_t(-1);   // one row: no stride to fall short
  c.out_align = host ? 0 : 8;
  c.n_out = n_out;
  const auto run = [&](hipStream_t s, const void* src, size_t, void* dst, size_t, size_t* n) {
    return d->enqueue(s, n_in, n, [&](long long m_first, long long n_new) {
      DdcLaunch a;
      a.in = src;
      a.fmt = fmt;
      a.n_in = (long long)n_in;
      a.n0 = d->n_total;
      a.p0 = ddc_phase_at(d, d->n_total);
      a.step = d->step;
      a.nco = d->d_nco;
      a.taps = d->d_taps;
      a.D = d->D;
      a.n_taps = d->n_taps;
      a.phases = d->phases;
      a.hist = d->d_hist[d->cur].as<float2>();
      a.hist_out = d->d_hist[d->cur ^ 1].as<float2>();
      a.out = static_cast<float2*>(dst);
      a.m_first = m_first;
      a.n_out = n_new;
      return launch_ddc(a, s);
    });
  };
  return host ? Feed::host(d, kDdc, c, run) : Feed::dev(d, kDdc, p, c, run);
}

}  // namespace

int tdsa_ddc_create(int device_id, int decimation, int max_taps, size_t max_host_samples, tdsa_ddc* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (decimation < kDdcMinDecimation || decimation > kDdcMaxDecimation)
    return fail(TDSA_ERR_ARG, "decimation=%d: %d .. %d", decimation, kDdcMinDecimation, kDdcMaxDecimation);
  if (max_taps < 1 || max_taps > kDdcMaxTapsPerPhase * decimation)
    return fail(TDSA_ERR_ARG, "max_taps=%d: 1 .. %d (64 per phase at decimation %d)", max_taps,
                kDdcMaxTapsPerPhase * decimation, decimation);
  if (max_host_samples < 1) return fail(TDSA_ERR_ARG, "max_host_samples=%zu", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_ddc d = new (std::nothrow) tdsa_ddc_s();
  if (!d) return fail(TDSA_ERR_NOMEM, "out of host memory");
  d->device = device_id;
  d->D = decimation;
  d->max_taps = max_taps;
  d->max_phases = ddc_phases(max_taps, decimation);
  d->max_host = max_host_samples;
  d->taps_len = size_t(d->max_phases) * decimation;
  d->hist_bytes = d->taps_len * sizeof(float2);
  std::vector<float2> nco(kDdcNcoTable);
  for (int k = 0; k < kDdcNcoTable; ++k) {
    const double th = 2.0 * M_PI * double(k) / double(kDdcNcoTable);
    nco[k] = make_float2(float(std::cos(th)), float(-std::sin(th)));
  }
  hipError_t e = d->open(false);
  if (e == hipSuccess) e = d->d_nco.alloc(kDdcNcoTable);
  if (e == hipSuccess) e = d->alloc(1, 1, sizeof(float2));
  if (e == hipSuccess) e = hipMemcpyAsync(d->d_nco, nco.data(), kDdcNcoTable * sizeof(float2), hipMemcpyHostToDevice, d->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream);   // the host copy of the table is released
  if (e != hipSuccess) {
    (void)tdsa_ddc_destroy(d);
    return fail(TDSA_ERR_HIP, "ddc create: %s", hipGetErrorString(e));
  }
  const int rc = ddc_clear(d);
  if (rc != TDSA_OK) {
    (void)tdsa_ddc_destroy(d);
    return rc;
  }
  *out = d;
  return TDSA_OK;
}

int tdsa_ddc_destroy(tdsa_ddc d) {
  if (!d) return TDSA_OK;
  d->drain();
  delete d;
  return TDSA_OK;
}

int tdsa_ddc_set_taps(tdsa_ddc d, const float* taps_host, int n_taps) {
  if (!d) return fail(TDSA_ERR_ARG, "null ddc");
  TRY(d->set_taps(taps_host, n_taps));
  d->phases = ddc_phases(n_taps, d->D);
  d->n_b = 0;
  d->p_b = 0;
  return TDSA_OK;
}

int tdsa_ddc_set_nco(tdsa_ddc d, uint32_t phase_step) {
  if (!d) return fail(TDSA_ERR_ARG, "null ddc");
  d->p_b = ddc_phase_at(d, d->n_total);
  d->n_b = d->n_total;
  d->step = phase_step;
  return TDSA_OK;
}

int tdsa_ddc_reset(tdsa_ddc d) {
  if (!d) return fail(TDSA_ERR_ARG, "null ddc");
  TRY(ddc_clear(d));
  HIPCHK(hipStreamSynchronize(d->stream));   // every earlier call of the handle has finished too
  return TDSA_OK;
}

int tdsa_ddc_process(tdsa_ddc d, int in_format, const void* iq_host, size_t n_in, float* out_host, size_t* n_out) {
  return ddc_process(d, nullptr, true, in_format, iq_host, n_in, out_host, n_out);
}

int tdsa_ddc_process_dev(tdsa_ddc d, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                         size_t* n_out) {
  return ddc_process(d, p, false, in_format, iq_dev, n_in, out_dev, n_out);
}
