// tdsa_capi_analytics.cpp - tdsa_rows_*, the per-frame scalars' setter / getter, tdsa_density_*, tdsa_waterfall_*.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

// ================================================================================================
// Trace analytics and display accumulators on device-resident dB rows
// ================================================================================================
namespace {

// scratch that grows on demand, owned by the plan (freed by tdsa_destroy; one plan = one thread at a time)
int plan_scratch(tdsa_plan p, size_t need) { return p->d_scratch.grow(need, p->stream); }

// Where the result arrays of a rows_* call are formed and how they reach the caller's (pageable) arrays: every copy
// into pageable memory costs ~10 us in the runtime's own staging, so the arrays of a call sit back to back in ONE
// region - the plan's pinned, device-visible buffer itself when they are a few KB (one displayed row per GUI tick:
// the kernel stores over the bus, the host only waits), else device scratch and one DMA into the pinned buffer -
// and leave it by memcpy.  Results too large for the bounce buffer go piece by piece as before.
constexpr size_t kResultsDirectMax = 4096;
struct RowsResults {
  char* base = nullptr;      // where the kernel writes (device-visible)
  const char* host = nullptr;   // where the host reads after fetch(): the pinned buffer, or null = piece by piece
  size_t total = 0;
};
int rows_results_begin(tdsa_plan p, size_t total, RowsResults* r) {
  r->total = total;
  if (total <= kPinnedBounceMax) {
    TRY(ensure_pins(p, 0, total));
    r->host = static_cast<const char*>(p->h_out_pin);
  }
  if (total <= kResultsDirectMax) {
    r->base = static_cast<char*>(p->h_out_pin);
    return TDSA_OK;
  }
  TRY(plan_scratch(p, total));
  r->base = static_cast<char*>(p->d_scratch);
  return TDSA_OK;
}
// after the launch: wait; afterwards piece(off) is readable on the host (r.host != null)
int rows_results_fetch(tdsa_plan p, const RowsResults& r) {
  if (r.host && r.base != r.host)
    HIPCHK(hipMemcpyAsync(p->h_out_pin, r.base, r.total, hipMemcpyDeviceToHost, p->stream));
  if (r.host) HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}
int rows_results_piece(tdsa_plan p, const RowsResults& r, void* dst_host, size_t off, size_t bytes) {
  if (!dst_host || bytes == 0) return TDSA_OK;
  if (r.host) std::memcpy(dst_host, r.host + off, bytes);
  else HIPCHK(hipMemcpyAsync(dst_host, r.base + off, bytes, hipMemcpyDeviceToHost, p->stream));
  return TDSA_OK;
}

}  // namespace

int tdsa_set_frame_stats(tdsa_plan p, int enable, int band_lo, int band_hi) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (enable && p->big) return fail(TDSA_ERR_STATE, "long-frame plans return one row per call: take tdsa_rows_stats of it");
  if (enable && band_lo <= band_hi && (band_lo < 0 || band_hi >= p->nfft))
    return fail(TDSA_ERR_ARG, "band [%d, %d] outside [0, %d)", band_lo, band_hi, p->nfft);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  p->fs_on = enable != 0;
  p->fs_lo = band_lo;
  p->fs_hi = band_hi;
  HIPCHK(hipStreamSynchronize(p->stream));                   // (joined: everything in flight is behind the main stream)
  for (auto& per_stream : p->fs)
    for (auto& sl : per_stream) sl.state = 0;
  for (auto& h : p->fs_hist) h = nullptr;
  p->fs_seq = 0;
  return TDSA_OK;
}

int tdsa_get_frame_stats(tdsa_plan p, int calls_back, int capacity, int* n_frames, float* peak_db_host,
                         int32_t* peak_bin_host, double* band_lin_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (!p->fs_on) return fail(TDSA_ERR_STATE, "tdsa_set_frame_stats has not enabled the per-frame scalars");
  if (calls_back < 0 || calls_back >= tdsa_plan_s::kFsKeep || (unsigned long long)calls_back >= p->fs_seq)
    return fail(TDSA_ERR_ARG, "calls_back=%d: the results of the last %d calls are kept, %llu made", calls_back,
                tdsa_plan_s::kFsKeep, p->fs_seq);
  tdsa_plan_s::FsSlot& sl = *p->fs_hist[(p->fs_seq - 1 - calls_back) % tdsa_plan_s::kFsKeep];
  if (sl.state == 2) return fail(TDSA_ERR_STATE, "that call wrote no dB rows and its plan / mode has no fused statistics");
  if (sl.state != 1) return fail(TDSA_ERR_STATE, "no statistics in that slot");
  if (n_frames) *n_frames = sl.n_frames;
  if (capacity < sl.n_frames && (peak_db_host || peak_bin_host || band_lin_host))
    return fail(TDSA_ERR_ARG, "capacity %d < %d frames", capacity, sl.n_frames);
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipStreamSynchronize(sl.stream));                   // the call's own stream (later calls on other streams stay in flight)
  if (!p->fs_stream) HIPCHK(hipStreamCreateWithFlags(&p->fs_stream, hipStreamNonBlocking));
  if (sl.pending) {
    HIPCHK(launch_frame_stats_finish(sl.d_part, sl.n_frames, sl.wpf, sl.cal_lin, sl.d_peak, sl.d_bin, sl.d_band,
                                     p->fs_stream));
    sl.pending = false;
  }
  const size_t nf = size_t(sl.n_frames);
  if (nf * 16 <= kPinnedBounceMax) {       // DMA into the pinned bounce buffer, one wait, memcpy out (pageable targets cost ~10 us each)
    TRY(ensure_pins(p, 0, nf * 16));
    char* pin = static_cast<char*>(p->h_out_pin);
    if (band_lin_host) HIPCHK(hipMemcpyAsync(pin, sl.d_band, nf * sizeof(double), hipMemcpyDeviceToHost, p->fs_stream));
    if (peak_db_host) HIPCHK(hipMemcpyAsync(pin + nf * 8, sl.d_peak, nf * sizeof(float), hipMemcpyDeviceToHost, p->fs_stream));
    if (peak_bin_host) HIPCHK(hipMemcpyAsync(pin + nf * 12, sl.d_bin, nf * sizeof(int), hipMemcpyDeviceToHost, p->fs_stream));
    HIPCHK(hipStreamSynchronize(p->fs_stream));
    if (band_lin_host) std::memcpy(band_lin_host, pin, nf * sizeof(double));
    if (peak_db_host) std::memcpy(peak_db_host, pin + nf * 8, nf * sizeof(float));
    if (peak_bin_host) std::memcpy(peak_bin_host, pin + nf * 12, nf * sizeof(int));
    return TDSA_OK;
  }
  if (peak_db_host) HIPCHK(hipMemcpyAsync(peak_db_host, sl.d_peak, nf * sizeof(float), hipMemcpyDeviceToHost, p->fs_stream));
  if (peak_bin_host) HIPCHK(hipMemcpyAsync(peak_bin_host, sl.d_bin, nf * sizeof(int), hipMemcpyDeviceToHost, p->fs_stream));
  if (band_lin_host) HIPCHK(hipMemcpyAsync(band_lin_host, sl.d_band, nf * sizeof(double), hipMemcpyDeviceToHost, p->fs_stream));
  HIPCHK(hipStreamSynchronize(p->fs_stream));
  return TDSA_OK;
}

int tdsa_rows_stats(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, int band_lo, int band_hi,
                    double bin_width, float* peak_db_host, int32_t* peak_bin_host, double* band_db_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_rows == 0) return TDSA_OK;
  if (!rows_dev || n_rows < 0 || n_bins < 1) return fail(TDSA_ERR_ARG, "bad rows (%p, %d x %d)", (const void*)rows_dev, n_rows, n_bins);
  if (band_db_host && (band_lo < 0 || band_hi >= n_bins) && band_lo <= band_hi)
    return fail(TDSA_ERR_ARG, "band [%d, %d] outside [0, %d)", band_lo, band_hi, n_bins);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const size_t nr = size_t(n_rows), o_peak = nr * sizeof(double), o_bin = o_peak + nr * sizeof(float);
  RowsResults res;
  TRY(rows_results_begin(p, o_bin + nr * sizeof(int), &res));
  double* d_band = reinterpret_cast<double*>(res.base);
  float* d_peak = reinterpret_cast<float*>(res.base + o_peak);
  int* d_bin = reinterpret_cast<int*>(res.base + o_bin);
  HIPCHK(launch_rows_stats(rows_dev, n_rows, n_bins, band_lo, band_hi, bin_width, d_peak, d_bin,
                           band_db_host ? d_band : nullptr, p->stream));
  TRY(rows_results_fetch(p, res));
  TRY(rows_results_piece(p, res, peak_db_host, o_peak, nr * sizeof(float)));
  TRY(rows_results_piece(p, res, peak_bin_host, o_bin, nr * sizeof(int)));
  TRY(rows_results_piece(p, res, band_db_host, 0, nr * sizeof(double)));
  if (!res.host) HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

int tdsa_rows_top_peaks(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, int n_peaks, int min_sep_bins,
                        float min_excursion_db, int32_t* peak_bins_host, float* peak_db_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_rows == 0) return TDSA_OK;
  if (!rows_dev || !peak_bins_host || n_rows < 0) return fail(TDSA_ERR_ARG, "null / negative argument");
  if (n_peaks < 1 || n_peaks > 8) return fail(TDSA_ERR_ARG, "n_peaks=%d outside [1, 8]", n_peaks);
  if (n_bins < 1 || n_bins > 16384) return fail(TDSA_ERR_ARG, "n_bins=%d outside [1, 16384] (row must fit the LDS)", n_bins);
  if (reinterpret_cast<uintptr_t>(rows_dev) % sizeof(float)) return fail(TDSA_ERR_ARG, "rows_dev %p is not aligned to a float", (const void*)rows_dev);
  if (min_excursion_db != min_excursion_db) return fail(TDSA_ERR_ARG, "NaN min_excursion_db");
  // no two bins of a row are n_bins apart: every separation from n_bins up means the same, and below 1 there is no rule
  min_sep_bins = min_sep_bins < 1 ? 1 : (min_sep_bins > n_bins ? n_bins : min_sep_bins);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const size_t cnt = size_t(n_rows) * n_peaks;
  RowsResults res;
  TRY(rows_results_begin(p, cnt * (sizeof(int) + sizeof(float)), &res));
  int* d_bins = reinterpret_cast<int*>(res.base);
  float* d_db = reinterpret_cast<float*>(res.base + cnt * sizeof(int));
  HIPCHK(launch_top_peaks(rows_dev, n_rows, n_bins, n_peaks, min_sep_bins, min_excursion_db, d_bins, d_db, p->stream));
  TRY(rows_results_fetch(p, res));
  TRY(rows_results_piece(p, res, peak_bins_host, 0, cnt * sizeof(int)));
  TRY(rows_results_piece(p, res, peak_db_host, cnt * sizeof(int), cnt * sizeof(float)));
  if (!res.host) HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

int tdsa_rows_marker_peaks(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, double height, double prominence,
                           int distance, int current_idx, int max_list, int32_t* n_peaks_host, int32_t* snap_bin_host,
                           int32_t* next_bin_host, int32_t* peak_bins_host, double* peak_prom_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_rows == 0) return TDSA_OK;
  if (!rows_dev || n_rows < 0) return fail(TDSA_ERR_ARG, "null / negative argument");
  if (n_bins < 1 || n_bins > 16384) return fail(TDSA_ERR_ARG, "n_bins=%d outside [1, 16384] (row must fit the LDS)", n_bins);
  if (distance < 1) return fail(TDSA_ERR_ARG, "distance=%d (scipy: `distance` must be greater or equal to 1)", distance);
  if (max_list < 0 || (max_list > 0 && !peak_bins_host)) return fail(TDSA_ERR_ARG, "max_list=%d without a list buffer", max_list);
  if (height != height || prominence != prominence) return fail(TDSA_ERR_ARG, "NaN height / prominence");
  if (reinterpret_cast<uintptr_t>(rows_dev) % sizeof(float)) return fail(TDSA_ERR_ARG, "rows_dev %p is not aligned to a float", (const void*)rows_dev);
  if (distance > n_bins) distance = n_bins;                  // (no two peaks are n_bins apart: the same rule, and no overflow in the reach)
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const size_t cnt = size_t(n_rows) * max_list, rb = size_t(n_rows) * sizeof(int);
  const size_t o_bins = cnt * sizeof(double), o_count = o_bins + cnt * sizeof(int), o_snap = o_count + rb, o_next = o_snap + rb;
  RowsResults res;
  TRY(rows_results_begin(p, o_next + rb, &res));
  double* d_prom = reinterpret_cast<double*>(res.base);
  int* d_bins = reinterpret_cast<int*>(res.base + o_bins);
  int* d_count = reinterpret_cast<int*>(res.base + o_count);
  int* d_snap = reinterpret_cast<int*>(res.base + o_snap);
  int* d_next = reinterpret_cast<int*>(res.base + o_next);
  HIPCHK(launch_marker_peaks(rows_dev, n_rows, n_bins, height, prominence, distance, current_idx, max_list, d_count, d_snap,
                             d_next, max_list > 0 ? d_bins : nullptr, max_list > 0 && peak_prom_host ? d_prom : nullptr,
                             p->stream));
  TRY(rows_results_fetch(p, res));
  TRY(rows_results_piece(p, res, n_peaks_host, o_count, rb));
  TRY(rows_results_piece(p, res, snap_bin_host, o_snap, rb));
  TRY(rows_results_piece(p, res, next_bin_host, o_next, rb));
  if (max_list > 0) {
    TRY(rows_results_piece(p, res, peak_bins_host, o_bins, cnt * sizeof(int)));
    TRY(rows_results_piece(p, res, peak_prom_host, 0, cnt * sizeof(double)));
  }
  if (!res.host) HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

// ---- density histogram --------------------------------------------------------------------------
struct tdsa_density_s : Lane {
  int n = 0;
  float decay = 0.96f;
  Dev<float> d_hist;           // [n][512]
  Dev<float> d_img;            // log1p image scratch
  Dev<unsigned char> d_u8;     // the image as bytes (+ 8 bytes: its min / max)
  Pinned<float> h_row[2];      // pinned, device-visible staging of host rows (the kernel reads them in place)
  hipEvent_t ev_row[2] = {nullptr, nullptr};   // ... free again when the update that read them has run
  unsigned tick = 0;
};

int tdsa_density_create(int device_id, int n_bins, float decay, tdsa_density* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  if (n_bins < 1) return fail(TDSA_ERR_ARG, "n_bins=%d", n_bins);
  HIPCHK(hipSetDevice(device_id));
  tdsa_density d = new (std::nothrow) tdsa_density_s();
  if (!d) return fail(TDSA_ERR_NOMEM, "out of host memory");
  d->device = device_id;
  d->n = n_bins;
  d->decay = decay;
  const size_t hb = size_t(n_bins) * 512 * sizeof(float);
  hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = d->d_hist.alloc(hb / sizeof(float));
  for (int k = 0; k < 2; ++k) {
    if (e == hipSuccess) e = d->h_row[k].alloc(size_t(n_bins), hipHostMallocPortable | hipHostMallocMapped);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_row[k], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipMemsetAsync(d->d_hist, 0, hb, d->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
  if (e != hipSuccess) {
    (void)tdsa_density_destroy(d);
    return fail(TDSA_ERR_HIP, "density create: %s", hipGetErrorString(e));
  }
  *out = d;
  return TDSA_OK;
}

int tdsa_density_destroy(tdsa_density d) {
  if (!d) return TDSA_OK;
  d->drain();
  for (hipEvent_t ev : d->ev_row)
    if (ev) (void)hipEventDestroy(ev);
  delete d;
  return TDSA_OK;
}

int tdsa_density_set_decay(tdsa_density d, float decay) {
  if (!d) return fail(TDSA_ERR_ARG, "null density");
  d->decay = decay;
  return TDSA_OK;
}

int tdsa_density_reset(tdsa_density d) {
  if (!d) return fail(TDSA_ERR_ARG, "null density");
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipMemsetAsync(d->d_hist, 0, size_t(d->n) * 512 * sizeof(float), d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return TDSA_OK;
}

// rows produced on plan p's stream (p may be NULL when the rows are otherwise known to be complete)
int tdsa_density_update_dev(tdsa_density d, tdsa_plan p, const float* rows_dev, int n_rows) {
  if (!d) return fail(TDSA_ERR_ARG, "null density");
  if (n_rows == 0) return TDSA_OK;
  if (!rows_dev || n_rows < 0) return fail(TDSA_ERR_ARG, "bad rows");
  if (p && (p->device != d->device)) return fail(TDSA_ERR_ARG, "plan and histogram live on different devices");
  HIPCHK(hipSetDevice(d->device));
  if (p) TRY(plan_order_before(p, d->stream));   // order after the producer
  HIPCHK(launch_density(rows_dev, n_rows, d->n, d->decay, d->d_hist, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return TDSA_OK;
}

int tdsa_density_update(tdsa_density d, const float* row_host, int n) {
  if (!d || !row_host) return fail(TDSA_ERR_ARG, "null argument");
  if (n != d->n) return fail(TDSA_ERR_ARG, "row of %d bins, histogram has %d (re-create it: _ensure_hist)", n, d->n);
  HIPCHK(hipSetDevice(d->device));
  // the per-tick call returns when the row is staged and its update queued (every other entry point is ordered behind
  // it on the histogram's stream; tdsa_density_read waits): two pinned rows the kernel reads in place, each free again
  // once the update that read it has run
  const unsigned k = d->tick++ & 1u;
  HIPCHK(hipEventSynchronize(d->ev_row[k]));
  std::memcpy(d->h_row[k], row_host, size_t(n) * sizeof(float));
  HIPCHK(launch_density(d->h_row[k], 1, d->n, d->decay, d->d_hist, d->stream));
  HIPCHK(hipEventRecord(d->ev_row[k], d->stream));
  return TDSA_OK;
}

int tdsa_density_read(tdsa_density d, float* hist_host, int as_log1p) {
  if (!d || !hist_host) return fail(TDSA_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(d->device));
  const size_t cnt = size_t(d->n) * 512;
  const float* src = d->d_hist;
  if (as_log1p) {
    if (!d->d_img) HIPCHK(d->d_img.alloc(cnt));
    HIPCHK(launch_log1p(d->d_hist, d->d_img, cnt, d->stream));
    src = d->d_img;
  }
  HIPCHK(hipMemcpyAsync(hist_host, src, cnt * sizeof(float), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return TDSA_OK;
}

int tdsa_density_read_u8(tdsa_density d, uint8_t* img_host, float* levels2) {
  if (!d || !img_host) return fail(TDSA_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(d->device));
  const size_t cnt = size_t(d->n) * 512;
  if (!d->d_img) HIPCHK(d->d_img.alloc(cnt));
  if (!d->d_u8) HIPCHK(d->d_u8.alloc(cnt + 16));
  unsigned* d_mm = reinterpret_cast<unsigned*>(d->d_u8 + ((cnt + 7) & ~size_t(7)));
  HIPCHK(launch_log1p(d->d_hist, d->d_img, cnt, d->stream));
  HIPCHK(launch_minmax_pos(d->d_img, cnt, d_mm, d->stream));
  float mm[2];
  HIPCHK(hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  if (levels2) { levels2[0] = mm[0]; levels2[1] = mm[1]; }
  if (mm[1] > mm[0]) {
    HIPCHK(launch_quantize_u8(d->d_img, d->d_u8, cnt, mm[0], mm[1], d->stream));
  } else {
    HIPCHK(hipMemsetAsync(d->d_u8, 0, cnt, d->stream));      // a flat image (an empty histogram): every pixel at the lower level
  }
  HIPCHK(hipMemcpyAsync(img_host, d->d_u8, cnt, hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return TDSA_OK;
}

// ---- waterfall ring -----------------------------------------------------------------------------
struct tdsa_waterfall_s : Lane {
  int n = 0, history = 0;
  int ptr = 0;
  bool have_last = false;
  Dev<float> d_ring;           // [history][n]: every line once, the view is two copies
  Dev<float> d_last;           // [n] Waterfall._last_row
  Dev<unsigned char> d_u8;     // [history][n] the view as bytes (tdsa_waterfall_view_u8)
  Pinned<float> h_row;         // pinned staging of a host row: small rows are read in place by the kernels,
  Dev<float> d_row;            // larger ones take one DMA into d_row first (the scatter reads every bin)
  Dev<int> d_flags;            // [2][cap() / 2] differs, destination line per pushed row
  Dev<int> d_info;             // {new rows, last new row} of the push in flight, for the scatter
  Pinned<int> h_info;          // the same two words, pinned: what the host waits for
};

int tdsa_waterfall_create(int device_id, int history_lines, int n_bins, float min_db, tdsa_waterfall* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  if (history_lines < 1 || n_bins < 1) return fail(TDSA_ERR_ARG, "history=%d n_bins=%d", history_lines, n_bins);
  HIPCHK(hipSetDevice(device_id));
  tdsa_waterfall w = new (std::nothrow) tdsa_waterfall_s();
  if (!w) return fail(TDSA_ERR_NOMEM, "out of host memory");
  w->device = device_id;
  w->n = n_bins;
  w->history = history_lines;
  const size_t cnt = size_t(history_lines) * n_bins;
  hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = w->d_ring.alloc(cnt);
  if (e == hipSuccess) e = w->d_info.alloc(2);
  if (e == hipSuccess) e = w->h_info.alloc(2, hipHostMallocDefault);
  if (e == hipSuccess) e = w->d_last.alloc(size_t(n_bins));
  if (e == hipSuccess)
    e = w->h_row.alloc(size_t(n_bins), hipHostMallocPortable | hipHostMallocMapped);
  if (e == hipSuccess) e = w->d_row.alloc(size_t(n_bins));
  if (e == hipSuccess) e = launch_fill(w->d_ring, cnt, min_db, w->stream);    // np.full((2H, W), wf_min_db)
  if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
  if (e != hipSuccess) {
    (void)tdsa_waterfall_destroy(w);
    return fail(TDSA_ERR_HIP, "waterfall create: %s", hipGetErrorString(e));
  }
  *out = w;
  return TDSA_OK;
}

int tdsa_waterfall_destroy(tdsa_waterfall w) {
  if (!w) return TDSA_OK;
  w->drain();
  delete w;
  return TDSA_OK;
}

static int waterfall_push_rows(tdsa_waterfall w, const float* rows_dev, int n_rows, int* n_new) {
  TRY(w->d_flags.grow(2 * size_t(n_rows), nullptr));   // (every push ends with a wait)
  // new-row flags, the pointer walk of _add_row as a scan over them, the scatter: three launches, one wait
  w->h_info[0] = 0;
  w->h_info[1] = -1;
  HIPCHK(launch_waterfall_push(rows_dev, n_rows, w->n, w->have_last ? 1 : 0, w->ptr, w->history, w->d_flags,
                               w->d_flags + w->d_flags.cap() / 2, w->d_info, w->h_info, w->d_ring, w->d_last, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  const int fresh = w->h_info[0];
  if (fresh > 0) {
    w->ptr = ((w->ptr - fresh % w->history) % w->history + w->history) % w->history;
    w->have_last = true;
  }
  if (n_new) *n_new = fresh;
  return TDSA_OK;
}

int tdsa_waterfall_push_dev(tdsa_waterfall w, tdsa_plan p, const float* rows_dev, int n_rows, int* n_new) {
  if (!w) return fail(TDSA_ERR_ARG, "null waterfall");
  if (n_new) *n_new = 0;
  if (n_rows == 0) return TDSA_OK;
  if (!rows_dev || n_rows < 0) return fail(TDSA_ERR_ARG, "bad rows");
  if (p && p->device != w->device) return fail(TDSA_ERR_ARG, "plan and waterfall live on different devices");
  HIPCHK(hipSetDevice(w->device));
  if (p) TRY(plan_order_before(p, w->stream));
  return waterfall_push_rows(w, rows_dev, n_rows, n_new);
}

int tdsa_waterfall_push(tdsa_waterfall w, const float* row_host, int n, int* is_new) {
  if (!w || !row_host) return fail(TDSA_ERR_ARG, "null argument");
  if (n != w->n) return fail(TDSA_ERR_ARG, "row of %d bins, ring has %d", n, w->n);
  HIPCHK(hipSetDevice(w->device));
  std::memcpy(w->h_row, row_host, size_t(n) * sizeof(float));     // (every push ends with a wait: the row is free)
  if (n <= 4096) return waterfall_push_rows(w, w->h_row, 1, is_new);
  HIPCHK(hipMemcpyAsync(w->d_row, w->h_row, size_t(n) * sizeof(float), hipMemcpyHostToDevice, w->stream));
  return waterfall_push_rows(w, w->d_row, 1, is_new);
}

int tdsa_waterfall_view(tdsa_waterfall w, float* view_host, int* ptr) {
  if (!w) return fail(TDSA_ERR_ARG, "null waterfall");
  HIPCHK(hipSetDevice(w->device));
  if (view_host) {   // _display_view: buf[ptr : ptr + H], newest row first
    const size_t head = size_t(w->history - w->ptr) * w->n;      // lines ptr ... H-1, then 0 ... ptr-1
    HIPCHK(hipMemcpyAsync(view_host, w->d_ring + size_t(w->ptr) * w->n, head * sizeof(float), hipMemcpyDeviceToHost,
                          w->stream));
    if (w->ptr > 0)
      HIPCHK(hipMemcpyAsync(view_host + head, w->d_ring, size_t(w->ptr) * w->n * sizeof(float), hipMemcpyDeviceToHost,
                            w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
  }
  if (ptr) *ptr = w->ptr;
  return TDSA_OK;
}

int tdsa_waterfall_view_u8(tdsa_waterfall w, float min_db, float max_db, uint8_t* view_host) {
  if (!w || !view_host) return fail(TDSA_ERR_ARG, "null argument");
  if (!(max_db > min_db)) return fail(TDSA_ERR_ARG, "levels (%g, %g): need max > min", double(min_db), double(max_db));
  HIPCHK(hipSetDevice(w->device));
  const size_t cnt = size_t(w->history) * w->n;
  if (!w->d_u8) HIPCHK(w->d_u8.alloc(cnt));
  const size_t head = size_t(w->history - w->ptr) * w->n;
  HIPCHK(launch_quantize_u8(w->d_ring + size_t(w->ptr) * w->n, w->d_u8, head, min_db, max_db, w->stream));
  HIPCHK(launch_quantize_u8(w->d_ring, w->d_u8 + head, cnt - head, min_db, max_db, w->stream));
  HIPCHK(hipMemcpyAsync(view_host, w->d_u8, cnt, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return TDSA_OK;
}
