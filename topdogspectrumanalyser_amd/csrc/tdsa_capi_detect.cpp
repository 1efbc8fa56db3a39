// tdsa_capi_detect.cpp - tdsa_detect_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_detect.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_detect_row) == sizeof(DetRow), "the public row record is the kernel's");
static_assert(sizeof(tdsa_detect_signal) == sizeof(DetSignal), "the public signal record is the kernel's");

// ---- signal detection (tdsa_detect.hip) --------------------------------------------------------------------------
struct tdsa_detect_s : RowAnalyser {   // the second records: sub_per_row signals per row (max_signals)
  Dev<unsigned> d_occ;             // [n_bins] rows in which the bin was above the threshold
  uint64_t rows_flagged = 0;
  int lo = 0, hi = 0, rank = 0, min_width = 1, max_gap = 0;
  float margin = 0.0f, xdb = 0.0f;

  hipError_t launch(hipStream_t s, const float* rows, size_t n_rows) {
    DetLaunch a;
    a.rows = rows;
    a.n_rows = n_rows;
    a.n = n_bins;
    a.lo = lo;
    a.hi = hi;
    a.rank = rank;
    a.margin = margin;
    a.xdb = xdb;
    a.min_width = min_width;
    a.max_gap = max_gap;
    a.S = int(sub_per_row);
    a.row_rec = d_row.as<DetRow>();
    a.sig_rec = d_sub.as<DetSignal>();
    a.occ = d_occ;
    return launch_detect(a, s);
  }
  void tally(const tdsa_detect_row* row_host, size_t n_rows) {
    for (size_t r = 0; r < n_rows; ++r) rows_flagged += row_host[r].flags != 0;
  }
};

namespace {
constexpr RowNames kNames = {"detector", "detect", "signal"};
}

int tdsa_detect_create(int device_id, int n_bins, size_t max_host_rows, tdsa_detect* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (n_bins < 1 || n_bins > kDetMaxBins) return fail(TDSA_ERR_ARG, "n_bins=%d: 1 .. %d", n_bins, kDetMaxBins);
  if (max_host_rows < 1) return fail(TDSA_ERR_ARG, "max_host_rows=%zu: at least 1", max_host_rows);
  HIPCHK(hipSetDevice(device_id));
  {
    const hipError_t e = detect_prepare();
    if (e != hipSuccess)
      return fail(TDSA_ERR_HIP, "detect create: the device refuses %d bytes of LDS per workgroup: %s",
                  kDetMaxLdsBytes - kDetStaticLdsBytes, hipGetErrorString(e));
  }
  tdsa_detect h = new (std::nothrow) tdsa_detect_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->n_bins = n_bins;
  h->max_host = max_host_rows;
  h->row_unit = sizeof(DetRow);
  h->sub_unit = sizeof(DetSignal);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->alloc();
  if (e == hipSuccess) e = h->d_occ.alloc(size_t(n_bins));
  if (e == hipSuccess) e = hipMemsetAsync(h->d_occ, 0, size_t(n_bins) * sizeof(unsigned), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)tdsa_detect_destroy(h);
    return fail(TDSA_ERR_HIP, "detect create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_detect_destroy(tdsa_detect h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_detect_configure(tdsa_detect h, int bin_lo, int bin_hi, int rank, float margin_db, int min_width, int max_gap,
                          float xdb, int max_signals) {
  // what needs no handle first, then the handle, then what depends on its n_bins
  if (bin_lo < 0 || bin_hi < bin_lo || bin_hi >= kDetMaxBins)
    return fail(TDSA_ERR_ARG, "bins %d .. %d: 0 <= bin_lo <= bin_hi < n_bins", bin_lo, bin_hi);
  if (rank < 0 || rank > bin_hi - bin_lo)
    return fail(TDSA_ERR_ARG, "rank=%d: 0 .. %d, the range's bins less one", rank, bin_hi - bin_lo);
  if (!std::isfinite(margin_db)) return fail(TDSA_ERR_ARG, "margin_db is not finite");
  if (min_width < 1 || min_width > kDetMaxBins) return fail(TDSA_ERR_ARG, "min_width=%d: 1 .. n_bins", min_width);
  if (max_gap < 0 || max_gap > kDetMaxBins) return fail(TDSA_ERR_ARG, "max_gap=%d: 0 .. n_bins", max_gap);
  if (!std::isfinite(xdb) || xdb < 0.0f) return fail(TDSA_ERR_ARG, "xdb=%g: finite and not negative", double(xdb));
  if (max_signals < 1 || max_signals > kDetMaxSignals)
    return fail(TDSA_ERR_ARG, "max_signals=%d: 1 .. %d", max_signals, kDetMaxSignals);
  if (!h) return fail(TDSA_ERR_ARG, "null detector");
  if (bin_hi >= h->n_bins) return fail(TDSA_ERR_ARG, "bin_hi=%d: below the handle's %d bins", bin_hi, h->n_bins);
  if (min_width > h->n_bins) return fail(TDSA_ERR_ARG, "min_width=%d: 1 .. %d", min_width, h->n_bins);
  if (max_gap > h->n_bins) return fail(TDSA_ERR_ARG, "max_gap=%d: 0 .. %d", max_gap, h->n_bins);
  h->lo = bin_lo;
  h->hi = bin_hi;
  h->rank = rank;
  h->margin = margin_db;
  h->min_width = min_width;
  h->max_gap = max_gap;
  h->xdb = xdb;
  h->sub_per_row = size_t(max_signals);
  h->configured = true;
  return TDSA_OK;
}

int tdsa_detect_process(tdsa_detect h, const float* rows_host, size_t n_rows, tdsa_detect_row* row_records_host,
                        tdsa_detect_signal* signal_records_host) {
  return RowAnalyser::host(h, kNames, rows_host, n_rows, row_records_host, signal_records_host);
}

int tdsa_detect_process_dev(tdsa_detect h, tdsa_plan p, const float* rows_dev, size_t n_rows,
                            tdsa_detect_row* row_records_host, tdsa_detect_signal* signal_records_host) {
  return RowAnalyser::dev(h, kNames, p, rows_dev, n_rows, row_records_host, signal_records_host);
}

int tdsa_detect_read_occupancy(tdsa_detect h, uint32_t* counts_host, uint64_t* rows_seen, uint64_t* rows_flagged) {
  if (!h) return fail(TDSA_ERR_ARG, "null detector");
  if (!counts_host && !rows_seen && !rows_flagged) return fail(TDSA_ERR_ARG, "nothing to read into");
  if (counts_host) {
    TRY(h->own_stream());
    HIPCHK(hipMemcpyAsync(counts_host, h->d_occ, size_t(h->n_bins) * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    TRY(h->done(h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  if (rows_seen) *rows_seen = h->rows_seen;
  if (rows_flagged) *rows_flagged = h->rows_flagged;
  return TDSA_OK;
}

int tdsa_detect_reset(tdsa_detect h) {
  if (!h) return fail(TDSA_ERR_ARG, "null detector");
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_occ, 0, size_t(h->n_bins) * sizeof(unsigned), h->stream));
  TRY(h->done(h->stream));
  h->rows_seen = h->rows_flagged = 0;
  return TDSA_OK;
}

int tdsa_detect_timer_begin(tdsa_detect h) { return Lane::timer_begin(h, kNames.handle); }

int tdsa_detect_timer_end(tdsa_detect h, float* elapsed_ms) { return Lane::timer_end(h, kNames.handle, elapsed_ms); }
