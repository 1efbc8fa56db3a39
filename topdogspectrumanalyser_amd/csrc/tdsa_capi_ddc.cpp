// tdsa_capi_ddc.cpp - tdsa_ddc_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_ddc.hpp"

using namespace tdsa;

// ---- zoom front end: digital down-conversion (tdsa_ddc.hip) ------------------------------------------------------
struct tdsa_ddc_s : Lane {
  int D = 2, max_taps = 1, max_phases = kDdcBlock;
  size_t max_host = 0;
  float2* d_nco = nullptr;            // [kDdcNcoTable]
  float* d_taps = nullptr;            // [max_phases][D], zero beyond n_taps
  float2* d_hist[2] = {nullptr, nullptr};   // [max_phases * D] mixed inputs each, ping-pong
  int cur = 0;
  int n_taps = 0, phases = kDdcBlock;
  long long n_total = 0;              // inputs since the last reset
  uint32_t p_b = 0, step = 0;         // NCO: p[n] = p_b + (n - n_b) step (mod 2^32)
  long long n_b = 0;
  void* h_in = nullptr;               // pinned staging of a host block (up to 8 bytes per sample) ...
  void* d_in = nullptr;
  float2* d_out = nullptr;            // ... and of its outputs
  float2* h_out = nullptr;
  size_t out_cap = 0;
};

namespace {

int ddc_check_format(int fmt) {
  if (fmt == TDSA_IN_I8 || fmt == TDSA_IN_U8 || fmt == TDSA_IN_C64) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "in_format=%d: the down-converter takes complex IQ (TDSA_IN_I8 / _U8 / _C64)", fmt);
}

uint32_t ddc_phase_at(const tdsa_ddc d, long long n) {
  return d->p_b + uint32_t(uint64_t(n - d->n_b)) * d->step;
}

// zero history, input count and phase (the step is kept)
int ddc_clear(tdsa_ddc d) {
  TRY(d->own_stream());
  const size_t hb = size_t(d->max_phases) * d->D * sizeof(float2);
  HIPCHK(hipMemsetAsync(d->d_hist[0], 0, hb, d->stream));
  HIPCHK(hipMemsetAsync(d->d_hist[1], 0, hb, d->stream));
  TRY(d->done(d->stream));
  d->n_total = 0;
  d->n_b = 0;
  d->p_b = 0;
  return TDSA_OK;
}

// common checks of both process entry points (before any HIP call)
int ddc_check_call(tdsa_ddc d, int fmt, const void* in, size_t n_in, const void* out, size_t* n_out) {
  TRY(ddc_check_format(fmt));
  if (!d) return fail(TDSA_ERR_ARG, "null ddc");
  if (!n_out) return fail(TDSA_ERR_ARG, "null n_out");
  if (n_in > 0 && !in) return fail(TDSA_ERR_ARG, "null samples");
  const long long D = d->D;
  if (n_in > 0 && (d->n_total + (long long)n_in + D - 1) / D > (d->n_total + D - 1) / D && !out)
    return fail(TDSA_ERR_ARG, "null output");
  if (d->n_taps < 1) return fail(TDSA_ERR_STATE, "no taps: call tdsa_ddc_set_taps first");
  return TDSA_OK;
}

// enqueue one call on stream s: FIR of the outputs it completes, then the history for the next call
int ddc_run(tdsa_ddc d, hipStream_t s, int fmt, const void* in, size_t n_in, float2* out, size_t* n_out) {
  const long long D = d->D;
  const long long m_first = (d->n_total + D - 1) / D;
  const long long m_end = (d->n_total + (long long)n_in + D - 1) / D;
  *n_out = size_t(m_end - m_first);
  if (n_in == 0) return TDSA_OK;
  TRY(d->order(s));
  DdcLaunch a;
  a.in = in;
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
  a.hist = d->d_hist[d->cur];
  a.hist_out = d->d_hist[d->cur ^ 1];
  a.out = out;
  a.m_first = m_first;
  a.n_out = m_end - m_first;
  HIPCHK(launch_ddc(a, s));
  TRY(d->done(s));
  d->cur ^= 1;
  d->n_total += (long long)n_in;
  return TDSA_OK;
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
  d->out_cap = max_host_samples / size_t(decimation) + 1;
  const size_t hb = size_t(d->max_phases) * decimation * sizeof(float2);
  const size_t tb = size_t(d->max_phases) * decimation * sizeof(float);
  std::vector<float2> nco(kDdcNcoTable);
  for (int k = 0; k < kDdcNcoTable; ++k) {
    const double th = 2.0 * M_PI * double(k) / double(kDdcNcoTable);
    nco[k] = make_float2(float(std::cos(th)), float(-std::sin(th)));
  }
  hipError_t e = d->open(false);
  if (e == hipSuccess) e = hipMalloc(&d->d_nco, kDdcNcoTable * sizeof(float2));
  if (e == hipSuccess) e = hipMalloc(&d->d_taps, tb);
  if (e == hipSuccess) e = hipMalloc(&d->d_hist[0], hb);
  if (e == hipSuccess) e = hipMalloc(&d->d_hist[1], hb);
  if (e == hipSuccess) e = hipHostMalloc(&d->h_in, max_host_samples * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&d->d_in, max_host_samples * 8);
  if (e == hipSuccess) e = hipMalloc(&d->d_out, d->out_cap * sizeof(float2));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&d->h_out), d->out_cap * sizeof(float2), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemcpyAsync(d->d_nco, nco.data(), kDdcNcoTable * sizeof(float2), hipMemcpyHostToDevice, d->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d->d_taps, 0, tb, d->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
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
  free_all({d->d_nco, d->d_taps, d->d_hist[0], d->d_hist[1], d->d_in, d->d_out});
  if (d->h_in) (void)hipHostFree(d->h_in);
  if (d->h_out) (void)hipHostFree(d->h_out);
  d->close();
  delete d;
  return TDSA_OK;
}

int tdsa_ddc_set_taps(tdsa_ddc d, const float* taps_host, int n_taps) {
  if (!d) return fail(TDSA_ERR_ARG, "null ddc");
  if (!taps_host) return fail(TDSA_ERR_ARG, "null taps");
  if (n_taps < 1 || n_taps > d->max_taps)
    return fail(TDSA_ERR_ARG, "n_taps=%d: 1 .. %d (the handle's max_taps)", n_taps, d->max_taps);
  for (int k = 0; k < n_taps; ++k)
    if (!std::isfinite(taps_host[k])) return fail(TDSA_ERR_ARG, "tap %d is not finite", k);
  std::vector<float> pad(size_t(d->max_phases) * d->D, 0.0f);   // [phase][residue]: tap q D + r at q * D + r
  std::memcpy(pad.data(), taps_host, size_t(n_taps) * sizeof(float));
  TRY(d->own_stream());
  HIPCHK(hipMemcpyAsync(d->d_taps, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice, d->stream));
  d->n_taps = n_taps;
  d->phases = ddc_phases(n_taps, d->D);
  TRY(ddc_clear(d));
  HIPCHK(hipStreamSynchronize(d->stream));   // the host copy of the taps is released
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
  TRY(ddc_check_call(d, in_format, iq_host, n_in, out_host, n_out));
  if (n_in > d->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", n_in, d->max_host);
  *n_out = 0;
  if (n_in == 0) return TDSA_OK;
  HIPCHK(hipSetDevice(d->device));
  const size_t bytes = n_in * size_t(bytes_per_sample(in_format));
  std::memcpy(d->h_in, iq_host, bytes);   // the previous host call has waited: the staging is free
  HIPCHK(hipMemcpyAsync(d->d_in, d->h_in, bytes, hipMemcpyHostToDevice, d->stream));
  size_t n = 0;
  TRY(ddc_run(d, d->stream, in_format, d->d_in, n_in, d->d_out, &n));
  if (n) HIPCHK(hipMemcpyAsync(d->h_out, d->d_out, n * sizeof(float2), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  if (n) std::memcpy(out_host, d->h_out, n * sizeof(float2));
  *n_out = n;
  return TDSA_OK;
}

int tdsa_ddc_process_dev(tdsa_ddc d, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                         size_t* n_out) {
  TRY(ddc_check_call(d, in_format, iq_dev, n_in, out_dev, n_out));
  if (p && p->device != d->device) return fail(TDSA_ERR_ARG, "plan and down-converter live on different devices");
  if (out_dev && (reinterpret_cast<uintptr_t>(out_dev) % 8) != 0)
    return fail(TDSA_ERR_ARG, "output pointer must be aligned to one complex64 sample");
  *n_out = 0;
  if (n_in == 0) return TDSA_OK;
  hipStream_t s;
  TRY(d->producer_stream(p, &s));
  return ddc_run(d, s, in_format, iq_dev, n_in, static_cast<float2*>(out_dev), n_out);
}
