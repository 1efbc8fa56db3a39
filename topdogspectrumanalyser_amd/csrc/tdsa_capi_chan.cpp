// tdsa_capi_chan.cpp - tdsa_chan_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_chan.hpp"

using namespace tdsa;

// ---- polyphase channelizer (tdsa_chan.hip) -----------------------------------------------------------------------
struct tdsa_chan_s : Lane {
  int M = 4, log2M = 2, os = 1, max_taps = 1, max_rows = kChanBlock;
  size_t max_host = 0;
  float2* d_tw = nullptr;             // [M / 2]
  float* d_taps = nullptr;            // [max_rows][M], zero beyond n_taps
  float2* d_hist[2] = {nullptr, nullptr};   // [max_rows * M] unpacked inputs each, ping-pong
  int cur = 0;
  int n_taps = 0, P = 1;
  long long n_total = 0;              // inputs since the last reset
  void* h_in = nullptr;               // pinned staging of a host block (up to 8 bytes per sample) ...
  void* d_in = nullptr;
  float2* d_out = nullptr;            // ... and of its outputs, [M][n_out]
  float2* h_out = nullptr;
  size_t out_cap = 0;                 // outputs per channel one host block can complete
};

namespace {

int chan_check_format(int fmt) {
  if (fmt == TDSA_IN_I8 || fmt == TDSA_IN_U8 || fmt == TDSA_IN_C64) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "in_format=%d: the channelizer takes complex IQ (TDSA_IN_I8 / _U8 / _C64)", fmt);
}

// zero history and input count
int chan_clear(tdsa_chan c) {
  TRY(c->own_stream());
  const size_t hb = size_t(c->max_rows) * c->M * sizeof(float2);
  HIPCHK(hipMemsetAsync(c->d_hist[0], 0, hb, c->stream));
  HIPCHK(hipMemsetAsync(c->d_hist[1], 0, hb, c->stream));
  TRY(c->done(c->stream));
  c->n_total = 0;
  return TDSA_OK;
}

size_t chan_outputs(tdsa_chan c, size_t n_in) {
  const long long D = c->M / c->os;
  return size_t((c->n_total + (long long)n_in + D - 1) / D - (c->n_total + D - 1) / D);
}

// common checks of both process entry points (before any HIP call)
int chan_check_call(tdsa_chan c, int fmt, const void* in, size_t n_in, const void* out, size_t out_stride,
                    unsigned flags, size_t* n_out) {
  TRY(chan_check_format(fmt));
  if (!c) return fail(TDSA_ERR_ARG, "null channelizer");
  if (!n_out) return fail(TDSA_ERR_ARG, "null n_out");
  if (flags & ~unsigned(TDSA_CHAN_BRANCHES)) return fail(TDSA_ERR_ARG, "flags=%#x: TDSA_CHAN_BRANCHES or 0", flags);
  if (n_in > 0 && !in) return fail(TDSA_ERR_ARG, "null samples");
  const size_t n = chan_outputs(c, n_in);
  if (n > 0 && !out) return fail(TDSA_ERR_ARG, "null output");
  if (out_stride < n)
    return fail(TDSA_ERR_ARG, "out_stride=%zu: the call completes %zu outputs per channel", out_stride, n);
  if (c->n_taps < 1) return fail(TDSA_ERR_STATE, "no taps: call tdsa_chan_set_taps first");
  return TDSA_OK;
}

// enqueue one call on stream s: the bank over the outputs it completes, then the history for the next call
int chan_run(tdsa_chan c, hipStream_t s, int fmt, const void* in, size_t n_in, float2* out, size_t out_stride,
             unsigned flags, size_t* n_out) {
  const long long D = c->M / c->os;
  const long long m_first = (c->n_total + D - 1) / D;
  *n_out = chan_outputs(c, n_in);
  if (n_in == 0) return TDSA_OK;
  TRY(c->order(s));
  ChanLaunch a;
  a.in = in;
  a.fmt = fmt;
  a.n_in = (long long)n_in;
  a.n0 = c->n_total;
  a.taps = c->d_taps;
  a.tw = c->d_tw;
  a.M = c->M;
  a.log2M = c->log2M;
  a.os = c->os;
  a.P = c->P;
  a.hist = c->d_hist[c->cur];
  a.hist_out = c->d_hist[c->cur ^ 1];
  a.out = out;
  a.out_stride = (long long)out_stride;
  a.m_first = m_first;
  a.n_out = (long long)*n_out;
  a.branches = (flags & TDSA_CHAN_BRANCHES) ? 1 : 0;
  HIPCHK(launch_chan(a, s));
  TRY(c->done(s));
  c->cur ^= 1;
  c->n_total += (long long)n_in;
  return TDSA_OK;
}

}  // namespace

int tdsa_chan_create(int device_id, int channels, int oversample, int max_taps, size_t max_host_samples,
                     tdsa_chan* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (channels < kChanMinChannels || channels > kChanMaxChannels || (channels & (channels - 1)) != 0)
    return fail(TDSA_ERR_ARG, "channels=%d: a power of two, %d .. %d", channels, kChanMinChannels, kChanMaxChannels);
  if (oversample != 1 && oversample != 2) return fail(TDSA_ERR_ARG, "oversample=%d: 1 or 2", oversample);
  if (max_taps < 1 || max_taps > kChanMaxTapsPerBranch * channels)
    return fail(TDSA_ERR_ARG, "max_taps=%d: 1 .. %d (%d per branch at %d channels)", max_taps,
                kChanMaxTapsPerBranch * channels, kChanMaxTapsPerBranch, channels);
  if (max_host_samples < 1) return fail(TDSA_ERR_ARG, "max_host_samples=%zu", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_chan c = new (std::nothrow) tdsa_chan_s();
  if (!c) return fail(TDSA_ERR_NOMEM, "out of host memory");
  const int M = channels, D = channels / oversample;
  c->device = device_id;
  c->M = M;
  c->os = oversample;
  while ((1 << c->log2M) < M) ++c->log2M;
  c->max_taps = max_taps;
  c->max_rows = chan_tap_rows(max_taps, M);
  c->max_host = max_host_samples;
  c->out_cap = max_host_samples / size_t(D) + 1;
  const size_t hb = size_t(c->max_rows) * M * sizeof(float2);
  const size_t tb = size_t(c->max_rows) * M * sizeof(float);
  const size_t ob = c->out_cap * size_t(M) * sizeof(float2);
  std::vector<float2> tw(size_t(M / 2));   // exp(+2 pi j k / M): exact where the angle is a multiple of a quarter turn
  for (int k = 0; k < M / 2; ++k) {
    const double th = 2.0 * M_PI * double(k) / double(M);
    tw[k] = k == 0 ? make_float2(1.f, 0.f) : 4 * k == M ? make_float2(0.f, 1.f)
                                                        : make_float2(float(std::cos(th)), float(std::sin(th)));
  }
  hipError_t e = c->open(false);
  if (e == hipSuccess) e = hipMalloc(&c->d_tw, tw.size() * sizeof(float2));
  if (e == hipSuccess) e = hipMalloc(&c->d_taps, tb);
  if (e == hipSuccess) e = hipMalloc(&c->d_hist[0], hb);
  if (e == hipSuccess) e = hipMalloc(&c->d_hist[1], hb);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_in, max_host_samples * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&c->d_in, max_host_samples * 8);
  if (e == hipSuccess) e = hipMalloc(&c->d_out, ob);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->h_out), ob, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_taps, 0, tb, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the host copy of the twiddles is released
  if (e != hipSuccess) {
    (void)tdsa_chan_destroy(c);
    return fail(TDSA_ERR_HIP, "chan create: %s", hipGetErrorString(e));
  }
  const int rc = chan_clear(c);
  if (rc != TDSA_OK) {
    (void)tdsa_chan_destroy(c);
    return rc;
  }
  *out = c;
  return TDSA_OK;
}

int tdsa_chan_destroy(tdsa_chan c) {
  if (!c) return TDSA_OK;
  c->drain();
  free_all({c->d_tw, c->d_taps, c->d_hist[0], c->d_hist[1], c->d_in, c->d_out});
  if (c->h_in) (void)hipHostFree(c->h_in);
  if (c->h_out) (void)hipHostFree(c->h_out);
  c->close();
  delete c;
  return TDSA_OK;
}

int tdsa_chan_set_taps(tdsa_chan c, const float* taps_host, int n_taps) {
  if (!c) return fail(TDSA_ERR_ARG, "null channelizer");
  if (!taps_host) return fail(TDSA_ERR_ARG, "null taps");
  if (n_taps < 1 || n_taps > c->max_taps)
    return fail(TDSA_ERR_ARG, "n_taps=%d: 1 .. %d (the handle's max_taps)", n_taps, c->max_taps);
  for (int k = 0; k < n_taps; ++k)
    if (!std::isfinite(taps_host[k])) return fail(TDSA_ERR_ARG, "tap %d is not finite", k);
  std::vector<float> pad(size_t(c->max_rows) * c->M, 0.0f);   // [q][r]: tap q M + r at q * M + r
  std::memcpy(pad.data(), taps_host, size_t(n_taps) * sizeof(float));
  TRY(c->own_stream());
  HIPCHK(hipMemcpyAsync(c->d_taps, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  c->n_taps = n_taps;
  c->P = chan_branch_taps(n_taps, c->M);
  TRY(chan_clear(c));
  HIPCHK(hipStreamSynchronize(c->stream));   // the host copy of the taps is released
  return TDSA_OK;
}

int tdsa_chan_reset(tdsa_chan c) {
  if (!c) return fail(TDSA_ERR_ARG, "null channelizer");
  TRY(chan_clear(c));
  HIPCHK(hipStreamSynchronize(c->stream));   // every earlier call of the handle has finished too
  return TDSA_OK;
}

int tdsa_chan_process(tdsa_chan c, int in_format, const void* iq_host, size_t n_in, float* out_host,
                      size_t out_stride, unsigned flags, size_t* n_out) {
  TRY(chan_check_call(c, in_format, iq_host, n_in, out_host, out_stride, flags, n_out));
  if (n_in > c->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", n_in, c->max_host);
  *n_out = 0;
  if (n_in == 0) return TDSA_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = n_in * size_t(bytes_per_sample(in_format));
  std::memcpy(c->h_in, iq_host, bytes);   // the previous host call has waited: the staging is free
  HIPCHK(hipMemcpyAsync(c->d_in, c->h_in, bytes, hipMemcpyHostToDevice, c->stream));
  size_t n = 0;
  TRY(chan_run(c, c->stream, in_format, c->d_in, n_in, c->d_out, chan_outputs(c, n_in), flags, &n));
  const size_t row = n * sizeof(float2);
  if (n) HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, row * size_t(c->M), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int ch = 0; n && ch < c->M; ++ch)
    std::memcpy(out_host + 2 * size_t(ch) * out_stride, c->h_out + size_t(ch) * n, row);
  *n_out = n;
  return TDSA_OK;
}

int tdsa_chan_process_dev(tdsa_chan c, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                          size_t out_stride, unsigned flags, size_t* n_out) {
  if (out_dev && (reinterpret_cast<uintptr_t>(out_dev) % 8) != 0)
    return fail(TDSA_ERR_ARG, "output pointer must be aligned to one complex64 sample");
  TRY(chan_check_call(c, in_format, iq_dev, n_in, out_dev, out_stride, flags, n_out));
  if (p && p->device != c->device) return fail(TDSA_ERR_ARG, "plan and channelizer live on different devices");
  *n_out = 0;
  if (n_in == 0) return TDSA_OK;
  hipStream_t s;
  TRY(c->producer_stream(p, &s));
  return chan_run(c, s, in_format, iq_dev, n_in, static_cast<float2*>(out_dev), out_stride, flags, n_out);
}
