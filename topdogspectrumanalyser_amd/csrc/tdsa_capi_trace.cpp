// tdsa_capi_trace.cpp - tdsa_trace_*: hold / tare / averager state of one displayed trace (tdsa_trace.hip).
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

struct tdsa_trace_s : Lane {
  int n = 0;
  Dev<float> d_in;
  Dev<float> d_live;
  Dev<float> d_hold_max;
  Dev<float> d_hold_min;
  Dev<float> d_tare_base;
  Dev<float> d_tare_acc;
  Dev<double> d_avg;
  Dev<double> d_avg_in;
  Pinned<float> h_pin;          // pinned, device-visible: [4][n] row in, live / max / min out (one GUI tick, zero-copy)
  Pinned<double> h_pin_avg;     // pinned: [2][n] linear row in, averager state out (tdsa_trace_avg_process)
  long long held_max = 0, held_min = 0;
  bool tare_active = false;
  int tare_count = 0;
  int avg_mode = TDSA_AVG_OFF, avg_n = 1, avg_count = 0;
};

extern "C" {

int tdsa_trace_create(int device_id, int n, tdsa_trace* out) {
  if (!out) return fail(TDSA_ERR_ARG, "out is null");
  *out = nullptr;
  if (n < 1) return fail(TDSA_ERR_ARG, "n=%d must be >= 1", n);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(TDSA_ERR_ARG, "device %d of %d", device_id, ndev);
  HIPCHK(hipSetDevice(device_id));
  tdsa_trace t = new (std::nothrow) tdsa_trace_s();
  if (!t) return fail(TDSA_ERR_NOMEM, "host allocation failed");
  t->device = device_id;
  t->n = n;
  hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
  for (Dev<float>* b : {&t->d_in, &t->d_live, &t->d_hold_max, &t->d_hold_min, &t->d_tare_base, &t->d_tare_acc})
    if (e == hipSuccess) e = b->alloc(size_t(n));
  if (e == hipSuccess) e = t->d_avg.alloc(size_t(n));
  if (e == hipSuccess) e = t->d_avg_in.alloc(size_t(n));
  if (e != hipSuccess) {                     // a failure half way leaves nothing behind
    (void)tdsa_trace_destroy(t);
    return fail(TDSA_ERR_HIP, "trace create: %s", hipGetErrorString(e));
  }
  *out = t;
  return TDSA_OK;
}

int tdsa_trace_destroy(tdsa_trace t) {
  if (!t) return TDSA_OK;
  t->drain();
  delete t;
  return TDSA_OK;
}

int tdsa_trace_reset(tdsa_trace t, uint32_t what) {
  if (!t) return fail(TDSA_ERR_ARG, "null trace");
  if (what & TDSA_RESET_AVG) t->avg_count = 0;
  if (what & TDSA_RESET_HOLD_MAX) t->held_max = 0;
  if (what & TDSA_RESET_HOLD_MIN) t->held_min = 0;
  if (what & TDSA_RESET_TARE) {
    t->tare_active = false;
    t->tare_count = 0;
  }
  return TDSA_OK;
}

int tdsa_trace_update(tdsa_trace t, const float* db_in_host, int n, float cal_offset_db, int tare_collect,
                      int tare_total, int tare_subtract, uint32_t hold_flags, float* live_out, float* max_out,
                      float* min_out, int* tare_done) {
  if (!t || !db_in_host) return fail(TDSA_ERR_ARG, "null argument");
  if (n != t->n) return fail(TDSA_ERR_ARG, "row length %d != trace length %d", n, t->n);
  if (tare_collect && tare_total < 1) return fail(TDSA_ERR_ARG, "tare_total=%d", tare_total);
  HIPCHK(hipSetDevice(t->device));
  const size_t nb = size_t(n) * sizeof(float);
  // one displayed frame: the kernel reads the row from and writes its results to pinned, device-visible memory of the
  // trace object - no DMA operation on the way in or out (each costs ~10 us from / to pageable memory)
  if (!t->h_pin) HIPCHK(t->h_pin.alloc(4 * size_t(n), hipHostMallocPortable | hipHostMallocMapped));
  float* const h_in = t->h_pin;
  float* const h_live = t->h_pin + n;
  float* const h_max = t->h_pin + 2 * size_t(n);
  float* const h_min = t->h_pin + 3 * size_t(n);
  std::memcpy(h_in, db_in_host, nb);
  TraceParams tp{};
  tp.db_in = h_in;
  tp.n = n;
  tp.cal_db = cal_offset_db;
  tp.tare_acc = t->d_tare_acc;
  tp.tare_base = t->d_tare_base;
  bool finish = false;
  if (tare_collect) {
    tp.tare_collect = 1;
    tp.tare_first = t->tare_count == 0;
    t->tare_count += 1;
    tp.tare_count = t->tare_count;
    finish = t->tare_count >= tare_total;
    tp.tare_finish = finish;
  }
  tp.tare_active = ((tare_subtract && t->tare_active) || finish) ? 1 : 0;
  tp.live = live_out ? h_live : nullptr;
  tp.state_max = (hold_flags & TDSA_HOLD_MAX) ? t->d_hold_max : nullptr;
  tp.state_min = (hold_flags & TDSA_HOLD_MIN) ? t->d_hold_min : nullptr;
  tp.max_copy = (max_out && tp.state_max) ? h_max : nullptr;
  tp.min_copy = (min_out && tp.state_min) ? h_min : nullptr;
  tp.max_first = t->held_max == 0;
  tp.min_first = t->held_min == 0;
  HIPCHK(launch_trace_update(tp, t->stream));
  if (finish) {
    t->tare_active = true;
    t->tare_count = 0;
  }
  if (tare_done) *tare_done = finish ? 1 : 0;
  if (hold_flags & TDSA_HOLD_MAX) t->held_max += 1;
  if (hold_flags & TDSA_HOLD_MIN) t->held_min += 1;
  HIPCHK(hipStreamSynchronize(t->stream));
  if (live_out) std::memcpy(live_out, h_live, nb);
  if (tp.max_copy) std::memcpy(max_out, h_max, nb);
  if (tp.min_copy) std::memcpy(min_out, h_min, nb);
  return TDSA_OK;
}

int tdsa_trace_get_tare_baseline(tdsa_trace t, float* baseline_db_host, int* active) {
  if (!t) return fail(TDSA_ERR_ARG, "null trace");
  HIPCHK(hipSetDevice(t->device));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (baseline_db_host && t->tare_active)
    HIPCHK(hipMemcpy(baseline_db_host, t->d_tare_base, size_t(t->n) * sizeof(float), hipMemcpyDeviceToHost));
  if (active) *active = t->tare_active ? 1 : 0;
  return TDSA_OK;
}

int tdsa_trace_set_tare_baseline(tdsa_trace t, const float* baseline_db_host, int n) {
  if (!t) return fail(TDSA_ERR_ARG, "null trace");
  if (!baseline_db_host) {
    t->tare_active = false;
    return TDSA_OK;
  }
  if (n != t->n) return fail(TDSA_ERR_ARG, "baseline length %d != trace length %d", n, t->n);
  HIPCHK(hipSetDevice(t->device));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipMemcpy(t->d_tare_base, baseline_db_host, size_t(n) * sizeof(float), hipMemcpyHostToDevice));
  t->tare_active = true;
  return TDSA_OK;
}

int tdsa_trace_avg_set_mode(tdsa_trace t, int avg_mode, int avg_n) {
  if (!t) return fail(TDSA_ERR_ARG, "null trace");
  if (avg_mode < TDSA_AVG_OFF || avg_mode > TDSA_AVG_LIN) return fail(TDSA_ERR_ARG, "avg_mode %d", avg_mode);
  t->avg_mode = avg_mode;
  t->avg_n = avg_n < 1 ? 1 : avg_n;   // TraceAverager.set_mode: n = max(1, n), then reset()
  t->avg_count = 0;
  return TDSA_OK;
}

int tdsa_trace_avg_process(tdsa_trace t, const double* linear_in_host, int n, double* avg_out_host,
                           int* count_out) {
  if (!t || !linear_in_host) return fail(TDSA_ERR_ARG, "null argument");
  if (n != t->n) return fail(TDSA_ERR_ARG, "row length %d != trace length %d", n, t->n);
  if (t->avg_mode == TDSA_AVG_OFF || t->avg_n <= 1)
    return fail(TDSA_ERR_STATE, "averaging is off (pass-through is the caller's job)");
  HIPCHK(hipSetDevice(t->device));
  const size_t nb = size_t(n) * sizeof(double);
  // one row per call: in through pinned, device-visible memory the kernel reads in place, the state back through a
  // DMA copy into pinned memory (the float64 state itself stays on the device)
  if (!t->h_pin_avg)
    HIPCHK(t->h_pin_avg.alloc(2 * size_t(n), hipHostMallocPortable | hipHostMallocMapped));
  double* const h_in = t->h_pin_avg;
  double* const h_out = t->h_pin_avg + n;
  std::memcpy(h_in, linear_in_host, nb);
  HIPCHK(launch_avg_host_frame(h_in, n, t->d_avg, t->avg_count, t->avg_mode, t->avg_n, t->stream));
  if (t->avg_count == 0) t->avg_count = 1;
  else if (t->avg_mode == TDSA_AVG_LIN && t->avg_count < t->avg_n) t->avg_count += 1;
  if (avg_out_host) HIPCHK(hipMemcpyAsync(h_out, t->d_avg, nb, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (avg_out_host) std::memcpy(avg_out_host, h_out, nb);
  if (count_out) *count_out = t->avg_count;
  return TDSA_OK;
}

}  // extern "C"
