// tdsa_capi_chan.cpp - tdsa_chan_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_chan.hpp"

using namespace tdsa;

// ---- polyphase channelizer (tdsa_chan.hip) -----------------------------------------------------------------------
struct tdsa_chan_s : Feed {
  int M = 4, log2M = 2, os = 1, max_rows = kChanBlock, P = 1;
  Dev<float2> d_tw;                   // [M / 2]
  // the base's D = M / os; d_taps: [max_rows][M], tap q M + r at q * M + r; d_hist: [max_rows * M] unpacked inputs
  // (float2) each; the host staging of the outputs is [M][n_out]
};

namespace {

const FeedNames kChan = {"channelizer", "channelizer", "chan"};

// both process entry points: the bank over the outputs the call completes, then the history for the next call
int chan_process(tdsa_chan c, tdsa_plan p, bool host, int fmt, const void* in, size_t n_in, void* out,
                 size_t out_stride, unsigned flags, size_t* n_out) {
  if (flags & ~unsigned(TDSA_CHAN_BRANCHES)) return fail(TDSA_ERR_ARG, "flags=%#x: TDSA_CHAN_BRANCHES or 0", flags);
  FeedCall k;
  k.fmt = fmt;
  k.in = in;
  k.n_in = k.in_stride = n_in;
  k.in_unit = size_t(bytes_per_sample(fmt));
  k.out = out;
  k.out_stride = out_stride;
  k.out_rows = c ? size_t(c->M) : 1;
  k.out_align = host ? 0 : 8;
  k.n_out = n_out;
  const auto run = [&](hipStream_t s, const void* src, size_t, void* dst, size_t dst_stride, size_t* n) {
    return c->enqueue(s, n_in, n, [&](long long m_first, long long n_new) {
      ChanLaunch a;
      a.in = src;
      a.fmt = fmt;
      a.n_in = (long long)n_in;
      a.n0 = c->n_total;
      a.taps = c->d_taps;
      a.tw = c->d_tw;
      a.M = c->M;
      a.log2M = c->log2M;
      a.os = c->os;
      a.P = c->P;
      a.hist = c->d_hist[c->cur].as<float2>();
      a.hist_out = c->d_hist[c->cur ^ 1].as<float2>();
      a.out = static_cast<float2*>(dst);
      a.out_stride = (long long)dst_stride;
      a.m_first = m_first;
      a.n_out = n_new;
      a.branches = (flags & TDSA_CHAN_BRANCHES) ? 1 : 0;
      return launch_chan(a, s);
    });
  };
  return host ? Feed::host(c, kChan, k, run) : Feed::dev(c, kChan, p, k, run);
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
  c->D = D;
  c->M = M;
  c->os = oversample;
  while ((1 << c->log2M) < M) ++c->log2M;
  c->max_taps = max_taps;
  c->max_rows = chan_tap_rows(max_taps, M);
  c->max_host = max_host_samples;
  c->taps_len = size_t(c->max_rows) * M;
  c->hist_bytes = c->taps_len * sizeof(float2);
  std::vector<float2> tw(size_t(M / 2));   // exp(+2 pi j k / M): exact where the angle is a multiple of a quarter turn
  for (int k = 0; k < M / 2; ++k) {
    const double th = 2.0 * M_PI * double(k) / double(M);
    tw[k] = k == 0 ? make_float2(1.f, 0.f) : 4 * k == M ? make_float2(0.f, 1.f)
                                                        : make_float2(float(std::cos(th)), float(std::sin(th)));
  }
  hipError_t e = c->open(false);
  if (e == hipSuccess) e = c->d_tw.alloc(tw.size());
  if (e == hipSuccess) e = c->alloc(1, size_t(M), sizeof(float2));
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the host copy of the twiddles is released
  if (e != hipSuccess) {
    (void)tdsa_chan_destroy(c);
    return fail(TDSA_ERR_HIP, "chan create: %s", hipGetErrorString(e));
  }
  const int rc = c->clear();
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
  delete c;
  return TDSA_OK;
}

int tdsa_chan_set_taps(tdsa_chan c, const float* taps_host, int n_taps) {
  if (!c) return fail(TDSA_ERR_ARG, "null channelizer");
  TRY(c->set_taps(taps_host, n_taps));
  c->P = chan_branch_taps(n_taps, c->M);
  return TDSA_OK;
}

int tdsa_chan_reset(tdsa_chan c) {
  if (!c) return fail(TDSA_ERR_ARG, "null channelizer");
  TRY(c->clear());
  HIPCHK(hipStreamSynchronize(c->stream));   // every earlier call of the handle has finished too
  return TDSA_OK;
}

int tdsa_chan_process(tdsa_chan c, int in_format, const void* iq_host, size_t n_in, float* out_host,
                      size_t out_stride, unsigned flags, size_t* n_out) {
  return chan_process(c, nullptr, true, in_format, iq_host, n_in, out_host, out_stride, flags, n_out);
}

int tdsa_chan_process_dev(tdsa_chan c, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                          size_t out_stride, unsigned flags, size_t* n_out) {
  return chan_process(c, p, false, in_format, iq_dev, n_in, out_dev, out_stride, flags, n_out);
}
