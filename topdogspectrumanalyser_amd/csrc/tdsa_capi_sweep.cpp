// tdsa_capi_sweep.cpp - tdsa_sweep_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_sweep.hpp"

// the host evaluates bin frequencies with the kernels' expression: one multiply, one add, never fused
#pragma clang fp contract(off)

using namespace tdsa;

// ---- stepped sweeps: step detector and stitch (tdsa_sweep.hip) -----------------------------------------------------
struct tdsa_sweep_s : Lane {           // its stream: _read, _get_steps, the timer, and updates without a plan
  int nfft = 0, S = 0, n_grid = 0;
  hipEvent_t ev_tab = nullptr;        // the last upload of the step table has left its pinned staging
  bool geometry = false;
  std::vector<double> centres;
  double bin_hz = 0.0, h = 0.0;
  int k0 = 0, k1 = 0;
  std::vector<unsigned char> valid;   // per step: 1 = present
  bool tab_dirty = true;
  int n_present = 0;
  Dev<float> d_T;                     // [S][K]
  Dev<double> d_grid;                 // [n_grid]
  Dev<double> d_out;                  // [n_grid] of a _read without a device pointer
  Dev<double2> d_tab;                 // [S] (frequency of the first kept bin, centre) of the steps present
  Dev<int> d_step_of;                 // [S] their step numbers
  Pinned<char> h_tab;                 // pinned: S double2 then S int
  Dev<float> d_rows;                  // _run_dev: dB rows of one chunk of steps
  size_t chunk_bytes = kSweepChunkBytes;
};

namespace {

double sweep_x(const tdsa_sweep w, int s, int k) { return w->centres[s] + double(k - w->nfft / 2) * w->bin_hz; }

int sweep_check_detector(int det) {
  if (det >= TDSA_SWEEP_DET_SAMPLE && det <= TDSA_SWEEP_DET_AVG) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "detector=%d: TDSA_SWEEP_DET_SAMPLE / _MAX / _MIN / _AVG", det);
}

// common checks of both update entry points (before any HIP call)
int sweep_check_update(tdsa_sweep w, tdsa_plan p, int first_step, int n_steps, const void* src, int frames, int det) {
  TRY(sweep_check_detector(det));
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  if (!w->geometry) return fail(TDSA_ERR_STATE, "no geometry: call tdsa_sweep_set_geometry first");
  if (first_step < 0 || n_steps < 0 || first_step + (long long)n_steps > w->S)
    return fail(TDSA_ERR_ARG, "steps [%d, %d + %d) outside the handle's %d", first_step, first_step, n_steps, w->S);
  if (frames < 1) return fail(TDSA_ERR_ARG, "frames_per_step=%d: at least 1", frames);
  if (n_steps > 0 && !src) return fail(TDSA_ERR_ARG, "null input");
  if (p && p->device != w->device) return fail(TDSA_ERR_ARG, "plan and sweep assembler live on different devices");
  return TDSA_OK;
}

// the detector over rows of n_steps steps on stream s; those steps become present
int sweep_detect(tdsa_sweep w, hipStream_t s, int first_step, int n_steps, const float* rows, int frames,
                 size_t step_stride, int det) {
  TRY(w->order(s));
  SweepDetLaunch a;
  a.rows = rows;
  a.step_stride = (long long)step_stride;
  a.n_steps = n_steps;
  a.frames = frames;
  a.nfft = w->nfft;
  a.k0 = w->k0;
  a.k1 = w->k1;
  a.detector = det;
  a.T = w->d_T + size_t(first_step) * size_t(w->k1 - w->k0);
  HIPCHK(launch_sweep_detector(a, s));
  TRY(w->done(s));
  for (int i = 0; i < n_steps; ++i) {
    if (!w->valid[first_step + i]) w->tab_dirty = true;
    w->valid[first_step + i] = 1;
  }
  return TDSA_OK;
}

// the table of the steps present, through pinned staging, on the handle's stream
int sweep_upload_table(tdsa_sweep w) {
  if (!w->tab_dirty) return TDSA_OK;
  HIPCHK(hipEventSynchronize(w->ev_tab));
  double2* tab = w->h_tab.as<double2>();
  int* step_of = reinterpret_cast<int*>(tab + w->S);
  int n = 0;
  for (int s = 0; s < w->S; ++s) {
    if (!w->valid[s]) continue;
    tab[n] = make_double2(sweep_x(w, s, w->k0), w->centres[s]);
    step_of[n++] = s;
  }
  w->n_present = n;
  if (n) {
    HIPCHK(hipMemcpyAsync(w->d_tab, tab, size_t(n) * sizeof(double2), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(w->d_step_of, step_of, size_t(n) * sizeof(int), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipEventRecord(w->ev_tab, w->stream));
  }
  w->tab_dirty = false;
  return TDSA_OK;
}

}  // namespace

int tdsa_sweep_create(int device_id, int nfft, int n_steps, int n_grid, tdsa_sweep* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (nfft < 2 || nfft > kSweepMaxNfft) return fail(TDSA_ERR_ARG, "nfft=%d: 2 .. %d", nfft, kSweepMaxNfft);
  if (n_steps < 1 || n_steps > kSweepMaxSteps) return fail(TDSA_ERR_ARG, "n_steps=%d: 1 .. %d", n_steps, kSweepMaxSteps);
  if (n_grid < 2 || n_grid > kSweepMaxGrid) return fail(TDSA_ERR_ARG, "n_grid=%d: 2 .. %d", n_grid, kSweepMaxGrid);
  HIPCHK(hipSetDevice(device_id));
  tdsa_sweep w = new (std::nothrow) tdsa_sweep_s();
  if (!w) return fail(TDSA_ERR_NOMEM, "out of host memory");
  w->device = device_id;
  w->nfft = nfft;
  w->S = n_steps;
  w->n_grid = n_grid;
  w->valid.assign(size_t(n_steps), 0);
  const size_t S = size_t(n_steps);
  hipError_t e = w->open(true);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ev_tab, hipEventDisableTiming);
  if (e == hipSuccess) e = w->d_grid.alloc(size_t(n_grid));
  if (e == hipSuccess) e = w->d_out.alloc(size_t(n_grid));
  if (e == hipSuccess) e = w->d_tab.alloc(S);
  if (e == hipSuccess) e = w->d_step_of.alloc(S);
  if (e == hipSuccess) e = w->h_tab.alloc(S * (sizeof(double2) + sizeof(int)), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)tdsa_sweep_destroy(w);
    return fail(TDSA_ERR_HIP, "sweep create: %s", hipGetErrorString(e));
  }
  *out = w;
  return TDSA_OK;
}

int tdsa_sweep_destroy(tdsa_sweep w) {
  if (!w) return TDSA_OK;
  w->drain();
  if (w->ev_tab) (void)hipEventDestroy(w->ev_tab);
  delete w;
  return TDSA_OK;
}

int tdsa_sweep_set_geometry(tdsa_sweep w, const double* centres_hz, double bin_hz, int k0, int k1,
                            const double* grid_hz_host) {
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  if (!centres_hz) return fail(TDSA_ERR_ARG, "null centres");
  if (!grid_hz_host) return fail(TDSA_ERR_ARG, "null grid");
  if (!(bin_hz > 0.0) || !std::isfinite(bin_hz)) return fail(TDSA_ERR_ARG, "bin_hz=%g: positive and finite", bin_hz);
  if (k0 < 0 || k1 <= k0 || k1 > w->nfft)
    return fail(TDSA_ERR_ARG, "kept range [%d, %d): 0 <= k0 < k1 <= nfft = %d", k0, k1, w->nfft);
  for (int s = 0; s < w->S; ++s)
    if (!std::isfinite(centres_hz[s])) return fail(TDSA_ERR_ARG, "centre %d is not finite", s);
  for (int i = 0; i < w->n_grid; ++i)
    if (!std::isfinite(grid_hz_host[i])) return fail(TDSA_ERR_ARG, "grid point %d is not finite", i);
  const double lo = double(k0 - w->nfft / 2) * bin_hz, hi = double(k1 - 1 - w->nfft / 2) * bin_hz;
  for (int s = 0; s + 1 < w->S; ++s)
    if (!(centres_hz[s] + hi < centres_hz[s + 1] + lo))
      return fail(TDSA_ERR_ARG, "steps %d and %d: the last kept bin of one (%.17g Hz) is not below the first of the next "
                  "(%.17g Hz) - centres must ascend and kept ranges must not overlap", s, s + 1, centres_hz[s] + hi,
                  centres_hz[s + 1] + lo);
  HIPCHK(hipSetDevice(w->device));
  HIPCHK(hipEventSynchronize(w->ev_done));   // nothing in flight reads the old T or grid
  HIPCHK(hipStreamSynchronize(w->stream));
  TRY(w->d_T.grow(size_t(w->S) * size_t(k1 - k0), nullptr));
  HIPCHK(hipMemset(w->d_T, 0, size_t(w->S) * size_t(k1 - k0) * sizeof(float)));   // steps not yet present read as 0
  HIPCHK(hipMemcpy(w->d_grid, grid_hz_host, size_t(w->n_grid) * sizeof(double), hipMemcpyHostToDevice));
  w->centres.assign(centres_hz, centres_hz + w->S);
  w->bin_hz = bin_hz;
  w->k0 = k0;
  w->k1 = k1;
  w->h = grid_hz_host[1] - grid_hz_host[0];
  w->geometry = true;
  return tdsa_sweep_reset(w);
}

int tdsa_sweep_reset(tdsa_sweep w) {
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  w->valid.assign(size_t(w->S), 0);
  w->tab_dirty = true;
  return TDSA_OK;
}

int tdsa_sweep_set_chunk_bytes(tdsa_sweep w, size_t bytes) {
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  if (bytes < 1) return fail(TDSA_ERR_ARG, "bytes=%zu", bytes);
  w->chunk_bytes = bytes;
  return TDSA_OK;
}

int tdsa_sweep_update_dev(tdsa_sweep w, tdsa_plan p, int first_step, int n_steps, const float* rows_dev,
                          int frames_per_step, size_t step_stride_floats, int detector) {
  TRY(sweep_check_update(w, p, first_step, n_steps, rows_dev, frames_per_step, detector));
  if ((reinterpret_cast<uintptr_t>(rows_dev) % 4) != 0) return fail(TDSA_ERR_ARG, "rows pointer must be aligned to one float");
  if (n_steps == 0) return TDSA_OK;
  if (step_stride_floats == 0) step_stride_floats = size_t(frames_per_step) * size_t(w->nfft);
  hipStream_t s;
  TRY(w->producer_stream(p, &s));
  return sweep_detect(w, s, first_step, n_steps, rows_dev, frames_per_step, step_stride_floats, detector);
}

int tdsa_sweep_run_dev(tdsa_sweep w, tdsa_plan p, int in_format, const void* iq_dev, size_t step_stride_bytes,
                       int first_step, int n_steps, size_t n_samples_per_step, int hop, int frames_per_step,
                       int detector) {
  TRY(sweep_check_update(w, p, first_step, n_steps, iq_dev, frames_per_step, detector));
  if (!p) return fail(TDSA_ERR_ARG, "null plan: the rows come from one");
  if (p->nfft != w->nfft || p->big)
    return fail(TDSA_ERR_ARG, "the plan's frames (%d points%s) are not the assembler's rows of %d", p->nfft,
                p->big ? ", one row per call" : "", w->nfft);
  if (in_format < TDSA_IN_I8 || in_format > TDSA_IN_C64) return fail(TDSA_ERR_ARG, "in_format %d", in_format);
  if (n_steps == 0) return TDSA_OK;
  HIPCHK(hipSetDevice(w->device));
  const size_t step_floats = size_t(frames_per_step) * size_t(w->nfft);
  size_t per_chunk = w->chunk_bytes / (step_floats * sizeof(float));
  if (per_chunk < 1) per_chunk = 1;
  if (per_chunk > size_t(n_steps)) per_chunk = size_t(n_steps);
  JOIN(p);
  TRY(w->d_rows.grow(per_chunk * step_floats, p->stream));
  for (int done = 0; done < n_steps; done += int(per_chunk)) {
    const int n = n_steps - done < int(per_chunk) ? n_steps - done : int(per_chunk);
    TRY(tdsa_process_dev_batch(p, in_format, static_cast<const unsigned char*>(iq_dev) + size_t(done) * step_stride_bytes,
                               step_stride_bytes, n, n_samples_per_step, hop, frames_per_step, w->d_rows, 0));
    JOIN(p);   // the next chunk's frames, on whichever stream they go, start after this detector
    TRY(sweep_detect(w, p->stream, first_step + done, n, w->d_rows, frames_per_step, step_floats, detector));
  }
  return TDSA_OK;
}

int tdsa_sweep_read(tdsa_sweep w, int mode, double* out_f64_host, double* out_f64_dev) {
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  if (mode != TDSA_SWEEP_INTERP && mode != TDSA_SWEEP_PEAK)
    return fail(TDSA_ERR_ARG, "mode=%d: TDSA_SWEEP_INTERP / _PEAK", mode);
  if (!w->geometry) return fail(TDSA_ERR_STATE, "no geometry: call tdsa_sweep_set_geometry first");
  if (mode == TDSA_SWEEP_PEAK && !(w->h > 0.0))
    return fail(TDSA_ERR_ARG, "peak mode needs an ascending grid (grid[1] - grid[0] = %g)", w->h);
  if (out_f64_dev && (reinterpret_cast<uintptr_t>(out_f64_dev) % 8) != 0)
    return fail(TDSA_ERR_ARG, "output pointer must be aligned to one float64");
  TRY(w->own_stream());
  TRY(sweep_upload_table(w));
  SweepStitchLaunch a;
  a.tab = w->d_tab;
  a.step_of = w->d_step_of;
  a.n_present = w->n_present;
  a.K = w->k1 - w->k0;
  a.koff = w->k0 - w->nfft / 2;
  a.bin_hz = w->bin_hz;
  a.T = w->d_T;
  a.grid = w->d_grid;
  a.n_grid = w->n_grid;
  a.h = w->h;
  a.mode = mode;
  a.out = out_f64_dev ? out_f64_dev : w->d_out;
  HIPCHK(launch_sweep_stitch(a, w->stream));
  TRY(w->done(w->stream));
  if (out_f64_host) {
    HIPCHK(hipMemcpyAsync(out_f64_host, a.out, size_t(w->n_grid) * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
  }
  return TDSA_OK;
}

int tdsa_sweep_get_steps(tdsa_sweep w, float* T_host, unsigned char* valid_host) {
  if (!w) return fail(TDSA_ERR_ARG, "null sweep");
  if (!w->geometry) return fail(TDSA_ERR_STATE, "no geometry: call tdsa_sweep_set_geometry first");
  TRY(w->own_stream());
  if (T_host)
    HIPCHK(hipMemcpyAsync(T_host, w->d_T, size_t(w->S) * size_t(w->k1 - w->k0) * sizeof(float), hipMemcpyDeviceToHost,
                          w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  if (valid_host) std::memcpy(valid_host, w->valid.data(), size_t(w->S));
  return TDSA_OK;
}

int tdsa_sweep_timer_begin(tdsa_sweep w) { return Lane::timer_begin(w, "sweep"); }

int tdsa_sweep_timer_end(tdsa_sweep w, float* elapsed_ms) { return Lane::timer_end(w, "sweep", elapsed_ms); }
