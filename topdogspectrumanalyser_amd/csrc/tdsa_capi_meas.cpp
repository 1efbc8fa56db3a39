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
struct tdsa_meas_s : Lane {
  int n_bins = 0;
  size_t max_host = 0;             // rows one host call stages
  void* h_in = nullptr;            // pinned staging of a host block ...
  float* d_in = nullptr;
  MeasRow* d_row = nullptr;        // ... and the records of either entry point, grown on demand
  MeasChannel* d_ch = nullptr;
  size_t row_cap = 0, ch_cap = 0;
  float* d_limit = nullptr;        // [n_bins] the limit line, when there is one
  bool has_limit = false;
  int relative = 0;
  uint64_t rows_seen = 0, rows_failed = 0;
  bool configured = false;
  int C = 1, lo[kMeasMaxChannels] = {}, hi[kMeasMaxChannels] = {};
  int obw_lo = 0, obw_hi = 0;
  double fraction = 0.99;
  float xdb = 0.0f;
};

namespace {

// the checks both entry points share, before any HIP call
int meas_check(const tdsa_meas_s* h, const void* rows, const void* row_rec, const void* ch_rec) {
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  if (!h->configured) return fail(TDSA_ERR_ARG, "not configured: call tdsa_meas_configure first");
  if (!rows) return fail(TDSA_ERR_ARG, "null rows");
  if (!row_rec) return fail(TDSA_ERR_ARG, "null row records");
  if (!ch_rec) return fail(TDSA_ERR_ARG, "null channel records");
  return TDSA_OK;
}

// one call on stream s over device rows; returns when the records are in the caller's memory
int meas_run(tdsa_meas_s* h, hipStream_t s, const float* rows, size_t n_rows, tdsa_meas_row* row_host,
             tdsa_meas_channel* ch_host) {
  TRY(grow_device(&h->d_row, &h->row_cap, n_rows, h->last, sizeof(MeasRow)));
  TRY(grow_device(&h->d_ch, &h->ch_cap, n_rows * size_t(h->C), h->last, sizeof(MeasChannel)));
  MeasLaunch a;
  a.rows = rows;
  a.n_rows = n_rows;
  a.n = h->n_bins;
  a.C = h->C;
  for (int c = 0; c < h->C; ++c) {
    a.ch_lo[c] = int16_t(h->lo[c]);
    a.ch_hi[c] = int16_t(h->hi[c]);
  }
  a.obw_lo = h->obw_lo;
  a.obw_hi = h->obw_hi;
  a.f = h->fraction;
  a.xdb = h->xdb;
  a.limit = h->has_limit ? h->d_limit : nullptr;
  a.relative = h->relative;
  a.row_rec = h->d_row;
  a.ch_rec = h->d_ch;
  HIPCHK(launch_meas(a, s));
  HIPCHK(hipMemcpyAsync(row_host, h->d_row, n_rows * sizeof(MeasRow), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ch_host, h->d_ch, n_rows * size_t(h->C) * sizeof(MeasChannel), hipMemcpyDeviceToHost, s));
  TRY(h->done(s));
  HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
  h->rows_seen += n_rows;
  for (size_t r = 0; r < n_rows; ++r) h->rows_failed += (row_host[r].flags & TDSA_MEAS_MASK_FAIL) != 0;
  return TDSA_OK;
}

}  // namespace

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
  const size_t in_bytes = max_host_rows * size_t(n_bins) * sizeof(float);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = hipHostMalloc(&h->h_in, in_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_in), in_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_limit), size_t(n_bins) * sizeof(float));
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
  free_all({h->d_in, h->d_row, h->d_ch, h->d_limit});
  if (h->h_in) (void)hipHostFree(h->h_in);
  h->close();
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
  h->C = n_channels;
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
  TRY(meas_check(h, rows_host, row_records_host, channel_records_host));
  if (n_rows > h->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu rows, the handle stages at most %zu (max_host_rows)", n_rows, h->max_host);
  if (n_rows == 0) return TDSA_OK;
  TRY(h->own_stream());
  const size_t bytes = n_rows * size_t(h->n_bins) * sizeof(float);
  std::memcpy(h->h_in, rows_host, bytes);   // the previous host call has waited: the staging is free
  HIPCHK(hipMemcpyAsync(h->d_in, h->h_in, bytes, hipMemcpyHostToDevice, h->stream));
  return meas_run(h, h->stream, h->d_in, n_rows, row_records_host, channel_records_host);
}

int tdsa_meas_process_dev(tdsa_meas h, tdsa_plan p, const float* rows_dev, size_t n_rows, tdsa_meas_row* row_records_host,
                          tdsa_meas_channel* channel_records_host) {
  TRY(meas_check(h, rows_dev, row_records_host, channel_records_host));
  if (reinterpret_cast<uintptr_t>(rows_dev) % 4 != 0)
    return fail(TDSA_ERR_ARG, "rows_dev must be aligned to one float32 (4 bytes)");
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and measurement handle live on different devices");
  if (n_rows == 0) return TDSA_OK;
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  TRY(h->order(s));
  return meas_run(h, s, rows_dev, n_rows, row_records_host, channel_records_host);
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

int tdsa_meas_timer_begin(tdsa_meas h) {
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  return h->timer_begin();
}

int tdsa_meas_timer_end(tdsa_meas h, float* elapsed_ms) {
  if (!h) return fail(TDSA_ERR_ARG, "null measurement handle");
  if (!elapsed_ms) return fail(TDSA_ERR_ARG, "null elapsed_ms");
  return h->timer_end(elapsed_ms);
}
