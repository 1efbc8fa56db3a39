// tdsa_capi_demod.cpp - tdsa_demod_*.
#include <cstdint>
#include <limits>

#include "tdsa_capi_internal.hpp"
#include "tdsa_demod.hpp"

using namespace tdsa;

// ---- analog demodulator (tdsa_demod.hip) -------------------------------------------------------------------------
struct tdsa_demod_s : Feed {
  int mode = kDemodFM, C = 1, max_rows = kDemodBlock;
  // the base's D = R; d_taps: [max_rows][R], tap q R + r at q * R + r; d_hist: [C][hist_stride] discriminator values
  // (float) each; the host staging is [C][n_in] complex64 in, [C][n_out] float out
  long long hist_stride = 0;          // floats of history per channel: max phases * R
  Dev<float2> d_last[2];              // [C] the last raw sample, ping-pong with d_hist (the same `cur`)
  int pole_mode = kDemodPoleOff;
  float scale = 1.0f;
  Dev<float> d_pole;                  // [2][kDemodPoleBlock]: (1 - c) c^i, then c^(i + 1)
  Dev<float> d_pole_y;                // [C]
  Dev<float> d_pend;                  // [C][kDemodPoleBlock]
  Dev<char> d_meas;                   // [C] count, [C] sum, [C] sumsq, [C] max, [C] min

  long long* m_count() const { return d_meas.as<long long>(); }
  double* m_sum() const { return reinterpret_cast<double*>(m_count() + C); }
  double* m_sumsq() const { return m_sum() + C; }
  float* m_max() const { return reinterpret_cast<float*>(m_sumsq() + C); }
  float* m_min() const { return m_max() + C; }
  size_t meas_bytes() const { return size_t(C) * (8 + 8 + 8 + 4 + 4); }
};

namespace {

// count and sums to zero, max to -inf, min to +inf
int demod_clear_meas(tdsa_demod d) {
  TRY(d->own_stream());
  std::vector<unsigned char> init(d->meas_bytes(), 0);
  float* mx = reinterpret_cast<float*>(init.data() + size_t(d->C) * 24);
  for (int c = 0; c < d->C; ++c) {
    mx[c] = -std::numeric_limits<float>::infinity();
    mx[d->C + c] = std::numeric_limits<float>::infinity();
  }
  HIPCHK(hipMemcpyAsync(d->d_meas, init.data(), init.size(), hipMemcpyHostToDevice, d->stream));
  TRY(d->done(d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));   // the host copy is released; every earlier call has finished too
  return TDSA_OK;
}

const FeedNames kDemod = {"demodulator", "demodulator", "demod"};

// what the base's clear() leaves: last samples, pole state and measurements.  Waits for the stream.
int demod_clear_own(tdsa_demod d) {
  TRY(d->own_stream());
  for (int i = 0; i < 2; ++i) HIPCHK(hipMemsetAsync(d->d_last[i], 0, size_t(d->C) * sizeof(float2), d->stream));
  HIPCHK(hipMemsetAsync(d->d_pole_y, 0, size_t(d->C) * sizeof(float), d->stream));
  HIPCHK(hipMemsetAsync(d->d_pend, 0, size_t(d->C) * kDemodPoleBlock * sizeof(float), d->stream));
  TRY(d->done(d->stream));
  return demod_clear_meas(d);
}

// zero history, pole state, input count and measurements
int demod_clear(tdsa_demod d) {
  TRY(d->clear());
  return demod_clear_own(d);
}

// both process entry points: audio and post kernel over the outputs the call completes, then the history
int demod_process(tdsa_demod d, tdsa_plan p, bool host, const void* in, size_t n_in, size_t in_stride, void* out,
                  size_t out_stride, size_t* n_out) {
  FeedCall c;
  c.in = in;
  c.n_in = n_in;
  c.in_stride = in_stride;
  c.in_align = 8;
  c.out = out;
  c.out_stride = out_stride;
  c.out_unit = sizeof(float);
  c.out_align = 4;
  c.in_rows = c.out_rows = d ? size_t(d->C) : 1;
  c.n_out = n_out;
  const auto run = [&](hipStream_t s, const void* src, size_t src_stride, void* dst, size_t dst_stride, size_t* n) {
    return d->enqueue(s, n_in, n, [&](long long m_first, long long n_new) {
      DemodLaunch a;
      a.mode = d->mode;
      a.C = d->C;
      a.R = d->D;
      a.n_taps = d->n_taps;
      a.in = static_cast<const float2*>(src);
      a.in_stride = (long long)src_stride;
      a.n_in = (long long)n_in;
      a.n0 = d->n_total;
      a.taps = d->d_taps;
      a.hist = d->d_hist[d->cur].as<float>();
      a.hist_out = d->d_hist[d->cur ^ 1].as<float>();
      a.last = d->d_last[d->cur];
      a.last_out = d->d_last[d->cur ^ 1];
      a.hist_stride = d->hist_stride;
      a.out = static_cast<float*>(dst);
      a.out_stride = (long long)dst_stride;
      a.m_first = m_first;
      a.n_out = n_new;
      a.pole_mode = d->pole_mode;
      a.scale = d->scale;
      a.pole_w = d->d_pole;
      a.pole_cp = d->d_pole + kDemodPoleBlock;
      a.pole_y = d->d_pole_y;
      a.pole_pend = d->d_pend;
      a.m_count = d->m_count();
      a.m_max = d->m_max();
      a.m_min = d->m_min();
      a.m_sum = d->m_sum();
      a.m_sumsq = d->m_sumsq();
      return launch_demod(a, s);
    });
  };
  return host ? Feed::host(d, kDemod, c, run) : Feed::dev(d, kDemod, p, c, run);
}

int demod_upload_pole(tdsa_demod d, double c) {
  std::vector<float> t(2 * kDemodPoleBlock);
  double p = 1.0;                       // c^i in float64, every table entry rounded once
  for (int i = 0; i < kDemodPoleBlock; ++i) {
    t[i] = float((1.0 - c) * p);
    p *= c;
    t[kDemodPoleBlock + i] = float(p);
  }
  TRY(d->own_stream());
  HIPCHK(hipMemcpyAsync(d->d_pole, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, d->stream));
  TRY(d->done(d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));   // the host copy of the tables is released
  return TDSA_OK;
}

}  // namespace

int tdsa_demod_create(int device_id, int mode, int channels, int decimation, int max_taps, size_t max_host_samples,
                      tdsa_demod* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (mode != TDSA_DEMOD_FM && mode != TDSA_DEMOD_AM) return fail(TDSA_ERR_ARG, "mode=%d: TDSA_DEMOD_FM or _AM", mode);
  if (channels < 1 || channels > kDemodMaxChannels)
    return fail(TDSA_ERR_ARG, "channels=%d: 1 .. %d", channels, kDemodMaxChannels);
  if (decimation < 1 || decimation > kDemodMaxDecimation)
    return fail(TDSA_ERR_ARG, "decimation=%d: 1 .. %d", decimation, kDemodMaxDecimation);
  if (max_taps < 1 || max_taps > kDemodMaxTapsPerPhase * decimation)
    return fail(TDSA_ERR_ARG, "max_taps=%d: 1 .. %d (%d per phase at decimation %d)", max_taps,
                kDemodMaxTapsPerPhase * decimation, kDemodMaxTapsPerPhase, decimation);
  if (max_host_samples < size_t(channels))
    return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least one sample per channel", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_demod d = new (std::nothrow) tdsa_demod_s();
  if (!d) return fail(TDSA_ERR_NOMEM, "out of host memory");
  d->device = device_id;
  d->mode = mode;
  d->C = channels;
  d->D = decimation;
  d->max_taps = max_taps;
  d->max_rows = demod_tap_rows(max_taps, decimation);
  d->hist_stride = (long long)demod_phases(max_taps, decimation) * decimation;
  d->max_host = max_host_samples;
  d->taps_len = size_t(d->max_rows) * decimation;
  d->hist_bytes = size_t(channels) * size_t(d->hist_stride) * sizeof(float);
  hipError_t e = d->open(true);
  if (e == hipSuccess) e = d->alloc(size_t(channels), size_t(channels), sizeof(float));
  for (int i = 0; i < 2; ++i)
    if (e == hipSuccess) e = d->d_last[i].alloc(size_t(channels));
  if (e == hipSuccess) e = d->d_pole.alloc(2 * kDemodPoleBlock);
  if (e == hipSuccess) e = d->d_pole_y.alloc(size_t(channels));
  if (e == hipSuccess) e = d->d_pend.alloc(size_t(channels) * kDemodPoleBlock);
  if (e == hipSuccess) e = d->d_meas.alloc(d->meas_bytes());
  if (e != hipSuccess) {
    (void)tdsa_demod_destroy(d);
    return fail(TDSA_ERR_HIP, "demod create: %s", hipGetErrorString(e));
  }
  int rc = demod_upload_pole(d, 0.0);
  if (rc == TDSA_OK) rc = demod_clear(d);
  if (rc != TDSA_OK) {
    (void)tdsa_demod_destroy(d);
    return rc;
  }
  *out = d;
  return TDSA_OK;
}

int tdsa_demod_destroy(tdsa_demod d) {
  if (!d) return TDSA_OK;
  d->drain();
  delete d;
  return TDSA_OK;
}

int tdsa_demod_set_taps(tdsa_demod d, const float* taps_host, int n_taps) {
  if (!d) return fail(TDSA_ERR_ARG, "null demodulator");
  TRY(d->set_taps(taps_host, n_taps));
  return demod_clear_own(d);
}

int tdsa_demod_set_pole(tdsa_demod d, int pole_mode, double c, float scale) {
  if (!d) return fail(TDSA_ERR_ARG, "null demodulator");
  if (pole_mode != TDSA_DEMOD_POLE_OFF && pole_mode != TDSA_DEMOD_POLE_LOWPASS && pole_mode != TDSA_DEMOD_POLE_HIGHPASS)
    return fail(TDSA_ERR_ARG, "pole_mode=%d: TDSA_DEMOD_POLE_OFF, _LOWPASS or _HIGHPASS", pole_mode);
  if (!(c >= 0.0 && c < 1.0)) return fail(TDSA_ERR_ARG, "c=%g: 0 <= c < 1", c);
  if (!std::isfinite(scale)) return fail(TDSA_ERR_ARG, "scale is not finite");
  TRY(demod_upload_pole(d, c));
  d->pole_mode = pole_mode;
  d->scale = scale;
  return demod_clear(d);
}

int tdsa_demod_reset(tdsa_demod d) {
  if (!d) return fail(TDSA_ERR_ARG, "null demodulator");
  return demod_clear(d);
}

int tdsa_demod_process(tdsa_demod d, const void* in_host, size_t n_in, size_t in_stride, float* out_host,
                       size_t out_stride, size_t* n_out) {
  return demod_process(d, nullptr, true, in_host, n_in, in_stride, out_host, out_stride, n_out);
}

int tdsa_demod_process_dev(tdsa_demod d, tdsa_plan p, const void* in_dev, size_t n_in, size_t in_stride, void* out_dev,
                           size_t out_stride, size_t* n_out) {
  return demod_process(d, p, false, in_dev, n_in, in_stride, out_dev, out_stride, n_out);
}

int tdsa_demod_read_meas(tdsa_demod d, int64_t* count, float* max_f32, float* min_f32, double* sum_f64,
                         double* sumsq_f64) {
  if (!d) return fail(TDSA_ERR_ARG, "null demodulator");
  if (!count || !max_f32 || !min_f32 || !sum_f64 || !sumsq_f64) return fail(TDSA_ERR_ARG, "null result array");
  TRY(d->own_stream());
  std::vector<unsigned char> m(d->meas_bytes());
  HIPCHK(hipMemcpyAsync(m.data(), d->d_meas, m.size(), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  const size_t C = size_t(d->C);
  std::memcpy(count, m.data(), C * 8);
  std::memcpy(sum_f64, m.data() + C * 8, C * 8);
  std::memcpy(sumsq_f64, m.data() + C * 16, C * 8);
  std::memcpy(max_f32, m.data() + C * 24, C * 4);
  std::memcpy(min_f32, m.data() + C * 28, C * 4);
  return TDSA_OK;
}

int tdsa_demod_reset_meas(tdsa_demod d) {
  if (!d) return fail(TDSA_ERR_ARG, "null demodulator");
  return demod_clear_meas(d);
}

int tdsa_demod_timer_begin(tdsa_demod d) { return Lane::timer_begin(d, "demodulator"); }

int tdsa_demod_timer_end(tdsa_demod d, float* elapsed_ms) { return Lane::timer_end(d, "demodulator", elapsed_ms); }
