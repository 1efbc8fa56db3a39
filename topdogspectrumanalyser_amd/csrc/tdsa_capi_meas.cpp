// tdsa_capi_meas.cpp - tdsa_meas_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_meas.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_meas_row) == sizeof(MeasRow), "the public row record is the kernel's");
static_assert(sizeof(tdsa_meas_channel) == sizeof(MeasChannel), "the public channel record is the kernel's");
static_assert(TDSA_MEAS_EMPTY == kMeasFlagEmpty && TDSA_MEAS_INF == kMeasFlagInf && TDSA_MEAS_MASK_FAIL == kMeasFlagMaskFail,
              "the public flags are the kernel's");
static_assert(TDSA_MEAS_MAX_CHANNELS == kMeasMaxChannels, "the public channel count is the kernel's");

// ---- channel measurements (tdsa_meas.hip) ------------------------------------------------------------------------
struct tdsa_meas_s : RowAnalyser {   // the second records: sub_per_row channels per row
  Dev<float> d_limit;              // [n_bins] the limit line, when there is one
  bool has_limit = false;
  int relative = 0;
  uint64_t rows_failed = 0;
  int lo[kMeasMaxChannels] = {}, hi[kMeasMaxChannels] = {};
  int obw_lo = 0, obw_hi = 0;
  double fraction = 0.99;
  float xdb = 0.0f;

  hipError_t launch(hipStream_t s, const float* rows, size_t n_rows) {
    MeasLaunch a;
    a.rows = rows;
    a.n_rows = n_rows;
    a.n = n_bins;
    a.C = int(sub_per_row);
    for (int c = 0; c < a.C; ++c) {
      a.ch_lo[c] = int16_t(lo[c]);
      a.ch_hi[c] = int16_t(hi[c]);
    }
    a.obw_lo = obw_lo;
    a.obw_hi = obw_hi;
    a.f = fraction;
    a.xdb = xdb;
    a.limit = has_limit ? d_limit : nullptr;
    a.relative = relative;
    a.row_rec = d_row.as<MeasRow>();
    a.ch_rec = d_sub.as<MeasChannel>();
    return launch_meas(a, s);
  }
  void tally(const tdsa_meas_row* row_host, size_t n_rows) {
    for (size_t r = 0; r < n_rows; ++r) rows_failed += (row_host[r].flags & TDSA_MEAS_MASK_FAIL) != 0;
  }
};

namespace {
constexpr RowNames kNames = {"measurement handle", "meas", "channel"};
}

int tdsa_meas_create(int device_id, int n_bins, size_t max_host_rows, tdsa_meas* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (n_bins < 1 || n_bins > kMeasMaxBins) return fail(TDSA_ERR_ARG, "n_bins=%d: 1 .. %d", n_bins, kMeasMaxBins);
  if (max_host_rows < 1) return fail(TDSA_ERR_ARG, "max_host_rows=%zu: at least 1", max_host_rows);
  HIPCHK(hipSetDevice(device_id));
  {
    const hipError_t e = meas_prepare();
    if (e != hipSuccess)
      return fail(TDSA_ERR_HIP, "meas create: the device refuses %d bytes of LDS per workgroup: %s",
                  kMeasMaxLdsBytes - kMeasStaticLdsBytes, hipGetErrorString(e));
  }
  tdsa_meas h = new (std::nothrow) tdsa_meas_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->n_bins = n_bins;
  h->max_host = max_host_rows;
  h->row_unit = sizeof(MeasRow);
  h->sub_unit = sizeof(MeasChannel);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->alloc();
  if (e == hipSuccess) e = h->d_limit.alloc(size_t(n_bins));
  if (e != hipSuccess) {
    (void)tdsa_meas_destroy(h);
    return fail(TDSA_ERR_HIP, "meas create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_meas_destroy(tdsa_meas h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_meas_configure(tdsa_meas h, int n_channels, const int* lo, const int* hi, int obw_lo, int obw_hi, double fraction,
                        float xdb) {
  // what needs no handle first, then the handle, then what depends on its n_bins
  if (n_channels < 1 || n_channels > kMeasMaxChannels)
    return fail(TDSA_ERR_ARG, "n_channels=%d: 1 .. %d", n_channels, kMeasMaxChannels);
  if (!lo || !hi) return fail(TDSA_ERR_ARG, "channel bounds missing: lo and hi hold n_channels bins each");
  for (int c = 0; c < n_channels; ++c)
    if (lo[c] < 0 || hi[c] < lo[c] || hi[c] >= kMeasMaxBins)
      return fail(TDSA_ERR_ARG, "channel %d, bins %d .. %d: 0 <= lo <= hi < n_bins", c, lo[c], hi[c]);
  if (obw_lo < 0 || obw_hi < obw_lo || obw_hi >= kMeasMaxBins)
    return fail(TDSA_ERR_ARG, "obw bins %d .. %d: 0 <= obw_lo <= obw_hi < n_bins", obw_lo, obw_hi);
  if (!std::isfinite(fraction) || !(fraction > 0.0 && fraction < 1.0))
    return fail(TDSA_ERR_ARG, "fraction=%g: above 0 and below 1", fraction);
  if (!std::isfinite(xdb) || xdb < 0.0f) return fail(TDSA_ERR_ARG, "xdb=%g: finite and not negative", double(xdb));
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  for (int c = 0; c < n_channels; ++c)
    if (hi[c] >= h->n_bins)
      return fail(TDSA_ERR_ARG, "channel %d, hi=%d: below the handle's %d bins", c, hi[c], h->n_bins);
  if (obw_hi >= h->n_bins) return fail(TDSA_ERR_ARG, "obw_hi=%d: below the handle's %d bins", obw_hi, h->n_bins);
  h->sub_per_row = size_t(n_channels);
  for (int c = 0; c < n_channels; ++c) {
    h->lo[c] = lo[c];
    h->hi[c] = hi[c];
  }
  h->obw_lo = obw_lo;
  h->obw_hi = obw_hi;
  h->fraction = fraction;
  h->xdb = xdb;
  h->configured = true;
  return TDSA_OK;
}

int tdsa_meas_set_limit(tdsa_meas h, const float* limit_host, int n, int relative) {
  if (relative != 0 && relative != 1) return fail(TDSA_ERR_ARG, "relative=%d: 0 (absolute) or 1 (to channel 0's peak)", relative);
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  if (limit_host && n != h->n_bins)
    return fail(TDSA_ERR_ARG, "a limit of %d values: one per bin of the handle's %d", n, h->n_bins);
  if (!limit_host) {               // nothing is in flight: every process call returns with its launch finished
    h->has_limit = false;
    h->relative = 0;
    return TDSA_OK;
  }
  TRY(h->own_stream());            // behind the last launch, which may still read the previous line
  HIPCHK(hipMemcpyAsync(h->d_limit, limit_host, size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // limit_host is released on return
  h->has_limit = true;
  h->relative = relative;
  return TDSA_OK;
}

int tdsa_meas_process(tdsa_meas h, const float* rows_host, size_t n_rows, tdsa_meas_row* row_records_host,
                      tdsa_meas_channel* channel_records_host) {
  return RowAnalyser::host(h, kNames, rows_host, n_rows, row_records_host, channel_records_host);
}

int tdsa_meas_process_dev(tdsa_meas h, tdsa_plan p, const float* rows_dev, size_t n_rows, tdsa_meas_row* row_records_host,
                          tdsa_meas_channel* channel_records_host) {
  return RowAnalyser::dev(h, kNames, p, rows_dev, n_rows, row_records_host, channel_records_host);
}

int tdsa_meas_read_totals(tdsa_meas h, uint64_t* rows_seen, uint64_t* rows_failed) {
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  if (!rows_seen && !rows_failed) return fail(TDSA_ERR_ARG, "nothing to read into");
  if (rows_seen) *rows_seen = h->rows_seen;
  if (rows_failed) *rows_failed = h->rows_failed;
  return TDSA_OK;
}

int tdsa_meas_reset(tdsa_meas h) {
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  h->rows_seen = h->rows_failed = 0;
  return TDSA_OK;
}

int tdsa_meas_timer_begin(tdsa_meas h) { return Lane::timer_begin(h, kNames.handle); }

int tdsa_meas_timer_end(tdsa_meas h, float* elapsed_ms) { return Lane::timer_end(h, kNames.handle, elapsed_ms); }
