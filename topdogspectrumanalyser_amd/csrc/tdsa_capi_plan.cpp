// tdsa_capi_plan.cpp - the plan object: create / destroy, window, mode, state; the error text and the other
// library-wide entry points.  Plain C types only; every entry point returns a status and never throws.
#include "tdsa_capi_internal.hpp"

#include <cstdarg>

using namespace tdsa;

namespace tdsa {

static thread_local char g_err[512] = "ok";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int join_streams(tdsa_plan p) {
  if (p->aux_busy) {
    for (int i = 0; i < p->n_overlap - 1; ++i) {
      HIPCHK(hipEventRecord(p->ev_aux[i], p->aux[i]));
      HIPCHK(hipStreamWaitEvent(p->stream, p->ev_aux[i], 0));
    }
    p->aux_busy = false;
  }
  p->state_dirty = true;
  return TDSA_OK;
}

int plan_order_before(tdsa_plan p, hipStream_t consumer) {
  JOIN(p);
  HIPCHK(hipEventRecord(p->ev_state, p->stream));
  HIPCHK(hipStreamWaitEvent(consumer, p->ev_state, 0));
  return TDSA_OK;
}

std::vector<float2> unit_circle(int n) {
  std::vector<float2> tw(n);
  for (int m = 0; m < n; ++m) {
    const double ang = -2.0 * M_PI * double(m) / double(n);
    tw[m] = float2{float(std::cos(ang)), float(std::sin(ang))};
  }
  return tw;
}

// W_N^(n2 k1), k1 = a + 8 b: per column n2 the factors W_N^(n2 a), a = 1 .. NA-1, and W_N^(n2 8 b), b = 1 .. NB-1 -
// exponent reduced mod N in integers, angle and sin / cos in double, rounded once
std::vector<float2> seed_table(int n, int log2n) {
  const int nrow = 1 << kMaxLog2N, n1 = n >> kMaxLog2N, na = n1 < 8 ? n1 : 8;
  const int rows = big_seed_rows(log2n);
  std::vector<float2> seed(size_t(rows > 0 ? rows : 1) * nrow);
  for (int r = 0; r < rows; ++r) {
    const long long mult = r < na - 1 ? (r + 1) : 8ll * (r - (na - 1) + 1);
    for (int n2 = 0; n2 < nrow; ++n2) {
      const long long e = (mult * n2) % n;
      const double ang = -2.0 * M_PI * double(e) / double(n);
      seed[size_t(r) * nrow + n2] = float2{float(std::cos(ang)), float(std::sin(ang))};
    }
  }
  return seed;
}

}  // namespace tdsa

static int ilog2i(int x) {
  int l = 0;
  while ((1 << l) < x) ++l;
  return l;
}

static int reset_hold(tdsa_plan p, bool mx, bool mn) {
  if (mx) {
    HIPCHK(launch_fill(p->d_hold_max, p->nfft, -INFINITY, p->stream));
    p->held_max = 0;
  }
  if (mn) {
    HIPCHK(launch_fill(p->d_hold_min, p->nfft, INFINITY, p->stream));
    p->held_min = 0;
  }
  return TDSA_OK;
}

extern "C" {

const char* tdsa_last_error_string(void) { return g_err; }
int tdsa_version(void) { return TDSA_VERSION; }

int tdsa_device_count(int* count) {
  if (!count) return fail(TDSA_ERR_ARG, "count is null");
  HIPCHK(hipGetDeviceCount(count));
  return TDSA_OK;
}

static int plan_init(tdsa_plan p);

int tdsa_create(int device_id, int nfft, int max_frames, tdsa_plan* out) {
  if (!out) return fail(TDSA_ERR_ARG, "out is null");
  *out = nullptr;
  const bool native = nfft >= (1 << kMinLog2N) && nfft <= (1 << kBigMaxLog2N) && (nfft & (nfft - 1)) == 0;
  const bool chirp = !native && nfft >= 2 && nfft <= kChirpMaxN;
  if (!native && !chirp)
    return fail(TDSA_ERR_ARG, "nfft=%d: need a power of two in [%d, %d] or any size in [2, %d]", nfft, 1 << kMinLog2N,
                1 << kBigMaxLog2N, kChirpMaxN);
  const bool big = native && nfft > (1 << kMaxLog2N);
  if (max_frames < 1) return fail(TDSA_ERR_ARG, "max_frames=%d must be >= 1", max_frames);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(TDSA_ERR_ARG, "device %d of %d", device_id, ndev);
  HIPCHK(hipSetDevice(device_id));
  tdsa_plan p = new (std::nothrow) tdsa_plan_s();
  if (!p) return fail(TDSA_ERR_NOMEM, "host allocation failed");
  p->device = device_id;
  p->nfft = nfft;
  p->log2n = ilog2i(nfft);
  p->max_frames = max_frames;
  p->big = big;
  p->chirp = chirp;
  if (chirp) {
    int m = 1 << kMinLog2N;
    if (nfft > (1 << 19)) {                  // 2^21 would be needed: split into half-length sub-convolutions of 2^20
      p->chirp_split = (nfft + 1) / 2;
      m = 1 << kBigMaxLog2N;
    } else {
      while (m < 2 * nfft - 1) m <<= 1;
    }
    p->m_fft = m;
    p->log2m = ilog2i(m);
    p->chirp_big = p->log2m > kMaxLog2N;
    p->log2n = p->chirp_big ? kMaxLog2N : p->log2m;      // what the frame kernel of this plan transforms
  }
  const int rc_init = plan_init(p);          // a failure half way leaves nothing behind
  if (rc_init != TDSA_OK) {
    (void)tdsa_destroy(p);
    return rc_init;
  }
  *out = p;
  return TDSA_OK;
}

static int plan_init(tdsa_plan p) {
  const int device_id = p->device, nfft = p->nfft, max_frames = p->max_frames;
  const bool big = p->big;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  p->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // one thread per bin walking the frames beats the three launches of the chunked scan up to ~48 frames at N <= 4096
  // (N = 1024, 128 frames: 24.5 against 13.9 us) and up to ~128 at the larger sizes (N = 16384: 33.7 against 35.0 us)
  p->avg_wg_min = nfft <= 4096 ? 48 : 128;
  HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&p->ev0));
  HIPCHK(hipEventCreate(&p->ev1));
  HIPCHK(hipEventCreateWithFlags(&p->ev_state, hipEventDisableTiming));
  for (int f = 0; f < 3; ++f) HIPCHK(p->d_window[f].alloc(size_t(nfft)));
  if (!p->big && !p->chirp && p->log2n >= 11)     // only the 3-pass sizes read the permuted table (Cfg::WIN_LDS below)
    for (int f = 0; f < 3; ++f) HIPCHK(p->d_window_perm[f].alloc(size_t(nfft)));
  const int tw_n = p->chirp ? (p->chirp_big ? (1 << kMaxLog2N) : p->m_fft) : nfft;       // the size the frame kernel transforms
  HIPCHK(p->d_hold_max.alloc(size_t(nfft)));
  HIPCHK(p->d_hold_min.alloc(size_t(nfft)));
  HIPCHK(p->d_avg.alloc(size_t(nfft)));
  HIPCHK(p->d_dc_state.alloc(1));
  HIPCHK(p->d_sums.alloc(size_t(max_frames) + 8));   // (+ 7: block sums of overlapping frames)
  HIPCHK(p->d_dc_sub.alloc(size_t(max_frames)));
  HIPCHK(p->d_tare_base.alloc(size_t(nfft)));
  HIPCHK(p->d_tare_acc.alloc(size_t(nfft)));
  HIPCHK(p->d_trace_in.alloc(size_t(nfft)));
  HIPCHK(p->d_trace_live.alloc(size_t(nfft)));
  HIPCHK(hipMemsetAsync(p->d_dc_state, 0, sizeof(float2), p->stream));
  HIPCHK(hipMemsetAsync(p->d_avg, 0, size_t(nfft) * sizeof(double), p->stream));
  TRY(upload(unit_circle(tw_n), p->d_tw));      // twiddle table exp(-2 pi i m / N)
  if (p->chirp) TRY(chirp_plan_init(p));
  if (big) {
    HIPCHK(p->d_sum.alloc(size_t(nfft)));
    HIPCHK(p->d_lin64.alloc(size_t(nfft)));
    {   // per-workgroup partial power sums of the row pass: [N1 * split][16384], split = workgroups per k1 row
      const int n1 = nfft >> 14;
      int split = p->num_cu / n1 > 1 ? p->num_cu / n1 : 1;
      const int gmax = p->max_frames < p->big_group ? p->max_frames : p->big_group;
      if (split > gmax) split = gmax;
      HIPCHK(p->d_acc.alloc(size_t(n1) * split * (size_t(1) << 14)));
    }
    const int nrow = 1 << kMaxLog2N;
    TRY(upload(seed_table(nfft, p->log2n), p->d_tw_seed));
    TRY(upload(unit_circle(nrow), p->d_tw_row));
    TRY(upload(std::vector<float>(nrow, 1.0f), p->d_ones));
  }
  TRY(reset_hold(p, true, true));
  // defaults = HackRF plain branch (hackrf_samples.py:382-383)
  p->mode.db_mode = TDSA_DB_MAG;
  p->mode.power_scale = 1.0f;
  p->mode.log_floor = 1e-12f;
  p->mode.avg_mode = TDSA_AVG_OFF;
  p->mode.avg_n = 1;
  p->mode.dc_alpha = 1.0f;
  p->mode.cal_offset_db = 0.0f;
  p->mode.hold_flags = 0;
  HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

int tdsa_destroy(tdsa_plan p) {
  if (!p) return TDSA_OK;
  (void)hipSetDevice(p->device);
  for (hipStream_t a : p->aux)
    if (a) (void)hipStreamSynchronize(a);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->fs_stream) { (void)hipStreamSynchronize(p->fs_stream); (void)hipStreamDestroy(p->fs_stream); }
  for (hipEvent_t e : p->prof_events) (void)hipEventDestroy(e);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  if (p->ev_state) (void)hipEventDestroy(p->ev_state);
  for (hipEvent_t e : p->ev_aux)
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t a : p->aux)
    if (a) (void)hipStreamDestroy(a);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
  return TDSA_OK;
}

int tdsa_get_info(tdsa_plan p, tdsa_info* out) {
  if (!p || !out) return fail(TDSA_ERR_ARG, "null argument");
  LaunchGeom g = p->big ? spectrum_geometry(kMaxLog2N, (p->nfft >> kMaxLog2N) * (p->max_frames < p->big_group ? p->max_frames : p->big_group), p->num_cu)
                        : spectrum_geometry(p->log2n, p->max_frames, p->num_cu);
  out->nfft = p->nfft;
  out->max_frames = p->max_frames;
  out->device_id = p->device;
  out->grid = g.grid;
  out->block = g.block;
  out->frames_per_block = g.fpw;
  out->lds_bytes = int(g.lds_bytes);
  out->num_cu = p->num_cu;
  out->frames_held_max = p->held_max;
  out->frames_held_min = p->held_min;
  out->avg_count = p->avg_count;
  out->version = TDSA_VERSION;
  return TDSA_OK;
}

// Long frames: the column pass fetches the window sample by sample (one 4-byte load each).  A window that is ONE value
// throughout - np.ones, rtl_samples.py:203-204 - travels as that value instead (BigWindow::flat); every other table
// is read.  (The cosine-sum windows the reference builds were also evaluated in the kernel in round 5 - two FMAs per
// sample from three scalar row constants: slower than the loads, see tdsa_big.hip; not kept.)
static void big_window_model(tdsa_plan p, const float* w, const float scale[3]) {
  bool flat = true;
  for (int i = 1; i < p->nfft && flat; ++i) flat = w[i] == w[0];
  for (int f = 0; f < 3; ++f) {
    p->big_win[f] = BigWindow{flat ? 2 : 0, p->d_window[f], w[0] * scale[f]};
  }
}

int tdsa_set_window(tdsa_plan p, const float* w_host, int n) {
  if (!p || !w_host) return fail(TDSA_ERR_ARG, "null argument");
  if (n != p->nfft) return fail(TDSA_ERR_ARG, "window length %d != nfft %d", n, p->nfft);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  float scale[3];                      // per input format, as d_window is
  for (int f = 0; f < 3; ++f) scale[f] = in_format_consts(f).scale;
  std::vector<float> tmp(n);
  HIPCHK(hipStreamSynchronize(p->stream));
  for (int f = 0; f < 3; ++f) {
    for (int i = 0; i < n; ++i) tmp[i] = w_host[i] * scale[f];
    HIPCHK(hipMemcpy(p->d_window[f], tmp.data(), size_t(n) * sizeof(float), hipMemcpyHostToDevice));
    if (p->d_window_perm[f]) HIPCHK(launch_window_perm(p->log2n, p->d_window[f], p->d_window_perm[f], p->stream));
  }
  if (p->big) big_window_model(p, w_host, scale);
  if (p->chirp && p->log2m >= 10) {
    // window x input scale x chirp a[n] = exp(-i pi n^2 / N) (phase from n^2 mod 2N in integers), product in double,
    // rounded once: the first transform multiplies the unpacked samples by it on load
    std::vector<float2> aw(n);
    std::vector<double> ca(n), sa(n);
    for (int i = 0; i < n; ++i) {
      const long long q = ((long long)i * i) % (2ll * n);
      const double ang = -M_PI * double(q) / double(n);
      ca[i] = std::cos(ang);
      sa[i] = std::sin(ang);
    }
    for (int f = 0; f < 3; ++f) {
      for (int i = 0; i < n; ++i) {
        const double wv = double(w_host[i]) * double(scale[f]);
        aw[i] = float2{float(wv * ca[i]), float(wv * sa[i])};
      }
      if (!p->d_chirp_aw[f]) HIPCHK(p->d_chirp_aw[f].alloc(aw.size()));
      HIPCHK(hipMemcpy(p->d_chirp_aw[f], aw.data(), aw.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
  }
  p->window_set = true;
  return TDSA_OK;
}

int tdsa_set_mode(tdsa_plan p, const tdsa_mode* m) {
  if (!p || !m) return fail(TDSA_ERR_ARG, "null argument");
  if (m->db_mode != TDSA_DB_MAG && m->db_mode != TDSA_DB_POW) return fail(TDSA_ERR_ARG, "db_mode %d", m->db_mode);
  if (m->avg_mode < TDSA_AVG_OFF || m->avg_mode > TDSA_AVG_LIN) return fail(TDSA_ERR_ARG, "avg_mode %d", m->avg_mode);
  if (m->dc_alpha > 1.0f) return fail(TDSA_ERR_ARG, "dc_alpha %g > 1", double(m->dc_alpha));
  if (!(m->log_floor >= 0.0f)) return fail(TDSA_ERR_ARG, "log_floor must be >= 0");
  tdsa_mode nm = *m;
  if (nm.avg_n < 1) nm.avg_n = 1;   // TraceAverager.set_mode: n = max(1, n)
  const bool avg_changed = nm.avg_mode != p->mode.avg_mode || nm.avg_n != p->mode.avg_n;
  p->mode = nm;
  if (avg_changed) p->avg_count = 0;   // set_mode() resets the buffer (signal_processing.py:26-28)
  return TDSA_OK;
}

int tdsa_set_overlap(tdsa_plan p, int n_streams) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_streams < 1 || n_streams > tdsa_plan_s::kMaxOverlap)
    return fail(TDSA_ERR_ARG, "n_streams=%d outside [1, %d]", n_streams, tdsa_plan_s::kMaxOverlap);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  for (int i = 0; i < n_streams - 1; ++i) {
    if (!p->aux[i]) {
      HIPCHK(hipStreamCreateWithFlags(&p->aux[i], hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&p->ev_aux[i], hipEventDisableTiming));
    }
  }
  p->n_overlap = n_streams;
  p->rr = 0;
  return TDSA_OK;
}

int tdsa_reset_state(tdsa_plan p, uint32_t what) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (what & TDSA_RESET_AVG) p->avg_count = 0;
  TRY(reset_hold(p, (what & TDSA_RESET_HOLD_MAX) != 0, (what & TDSA_RESET_HOLD_MIN) != 0));
  if ((what & TDSA_RESET_HOLD_MAX) && (what & TDSA_RESET_HOLD_MIN)) p->frames_seen = 0;
  if (what & TDSA_RESET_DC) HIPCHK(hipMemsetAsync(p->d_dc_state, 0, sizeof(float2), p->stream));
  if (what & TDSA_RESET_TARE) {
    p->tare_active = false;
    p->tare_count = 0;
  }
  return TDSA_OK;
}

int tdsa_set_tare_baseline(tdsa_plan p, const float* baseline_db_host, int n) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (!baseline_db_host) {
    p->tare_active = false;
    return TDSA_OK;
  }
  if (n != p->nfft) return fail(TDSA_ERR_ARG, "baseline length %d != nfft %d", n, p->nfft);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  HIPCHK(hipMemcpy(p->d_tare_base, baseline_db_host, size_t(n) * sizeof(float), hipMemcpyHostToDevice));
  p->tare_active = true;
  return TDSA_OK;
}

int tdsa_get_hold(tdsa_plan p, float* max_host, float* min_host, int64_t* frames_held) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  const size_t nb = size_t(p->nfft) * sizeof(float);
  if (max_host && p->held_max > 0) HIPCHK(hipMemcpy(max_host, p->d_hold_max, nb, hipMemcpyDeviceToHost));
  if (min_host && p->held_min > 0) HIPCHK(hipMemcpy(min_host, p->d_hold_min, nb, hipMemcpyDeviceToHost));
  if (frames_held) *frames_held = p->held_max > p->held_min ? p->held_max : p->held_min;
  return TDSA_OK;
}

int tdsa_get_avg(tdsa_plan p, double* avg_linear_host, int* count) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (p->big) TRY(big_materialize_mean(p));
  HIPCHK(hipStreamSynchronize(p->stream));
  if (avg_linear_host && p->avg_count > 0)
    HIPCHK(hipMemcpy(avg_linear_host, p->d_avg, size_t(p->nfft) * sizeof(double), hipMemcpyDeviceToHost));
  if (count) *count = p->avg_count;
  return TDSA_OK;
}

int tdsa_host_register(void* host, size_t bytes) {
  if (!host || bytes == 0) return fail(TDSA_ERR_ARG, "null / empty host range");
  HIPCHK(hipHostRegister(host, bytes, hipHostRegisterPortable));
  return TDSA_OK;
}

int tdsa_host_unregister(void* host) {
  if (!host) return fail(TDSA_ERR_ARG, "null host pointer");
  HIPCHK(hipHostUnregister(host));
  return TDSA_OK;
}

int tdsa_get_dc(tdsa_plan p, float* re, float* im) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  float2 dc;
  HIPCHK(hipMemcpy(&dc, p->d_dc_state, sizeof(dc), hipMemcpyDeviceToHost));
  if (re) *re = dc.x;
  if (im) *im = dc.y;
  return TDSA_OK;
}

int tdsa_set_dc(tdsa_plan p, float re, float im) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  const float2 dc{re, im};
  HIPCHK(hipMemcpy(p->d_dc_state, &dc, sizeof(dc), hipMemcpyHostToDevice));
  return TDSA_OK;
}

int tdsa_synchronize(tdsa_plan p) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

int tdsa_dev_alloc(int device_id, size_t bytes, void** out_dev) {
  if (!out_dev) return fail(TDSA_ERR_ARG, "out is null");
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipMalloc(out_dev, bytes));
  return TDSA_OK;
}
int tdsa_dev_free(int device_id, void* dev) {
  HIPCHK(hipSetDevice(device_id));
  if (dev) HIPCHK(hipFree(dev));
  return TDSA_OK;
}
int tdsa_memcpy_h2d(int device_id, void* dst_dev, const void* src_host, size_t bytes) {
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
  return TDSA_OK;
}
int tdsa_memcpy_d2h(int device_id, void* dst_host, const void* src_dev, size_t bytes) {
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return TDSA_OK;
}

int tdsa_plan_copy(tdsa_plan p, void* dst, const void* src, size_t bytes, int wait) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (bytes > 0 && (!dst || !src)) return fail(TDSA_ERR_ARG, "null pointer");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (bytes > 0) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, p->stream));
  if (wait) HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

}  // extern "C"
