// tdsa_capi_pipe.cpp - tdsa_pipe_*.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

// ================================================================================================
// tdsa_pipe: pinned host ring + asynchronous H2D / frame kernel / D2H legs on separate streams.
// Counterpart of the reader-thread -> queue.Queue(4) -> get_power_levels() front end of
// HackrfSamplesDataSource (datasources/hackrf_samples.py:191-305) for batch users: the producer writes
// IQ bytes straight into a pinned slot, the copy of slot k+1 and the read-back of slot k-1 overlap
// the frame kernel of slot k.
// ================================================================================================
struct tdsa_pipe_s {
  tdsa_plan plan = nullptr;
  int fmt = TDSA_IN_I8;
  size_t slot_samples = 0;
  bool rows = false;        // dB rows are produced (kept per slot on the device)
  bool rows_host = false;   // ... and read back into pinned host memory
  bool rows_u8 = false;     // ... as bytes under the display's levels (1 B per bin over PCIe instead of 4)
  float lo_db = -120.0f, hi_db = 0.0f;
  struct Slot {
    Pinned<char> h_in;
    Dev<char> d_in;
    Pinned<float> h_out;
    Dev<float> d_out;
    Pinned<unsigned char> h_u8;
    Dev<unsigned char> d_u8;
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_d2h = nullptr;
    int n_frames = 0;
    bool acquired = false, in_flight = false;
  };
  std::vector<Slot> slots;
  hipStream_t s_in = nullptr, s_out = nullptr;
  size_t head = 0, tail = 0;   // next slot to acquire / to collect
  int pending = 0;
};

int tdsa_pipe_create(tdsa_plan p, int in_format, size_t slot_samples, int n_slots, int want_rows, tdsa_pipe* out) {
  if (!p || !out) return fail(TDSA_ERR_ARG, "null argument");
  if (in_format < TDSA_IN_I8 || in_format > TDSA_IN_C64) return fail(TDSA_ERR_ARG, "in_format %d", in_format);
  if (n_slots < 1 || n_slots > 16) return fail(TDSA_ERR_ARG, "n_slots=%d outside [1, 16]", n_slots);
  if (slot_samples < size_t(p->nfft)) return fail(TDSA_ERR_ARG, "slot_samples=%zu < nfft", slot_samples);
  if (want_rows < 0 || want_rows > 3)
    return fail(TDSA_ERR_ARG, "want_rows=%d (0 none, 1 host, 2 device, 3 host as uint8 levels)", want_rows);
  HIPCHK(hipSetDevice(p->device));
  tdsa_pipe q = new (std::nothrow) tdsa_pipe_s();
  if (!q) return fail(TDSA_ERR_NOMEM, "out of host memory");
  q->plan = p;
  q->fmt = in_format;
  q->slot_samples = slot_samples;
  q->rows = want_rows != 0;
  q->rows_host = want_rows == 1;
  q->rows_u8 = want_rows == 3;
  q->slots = std::vector<tdsa_pipe_s::Slot>(size_t(n_slots));   // (a Slot owns its buffers: it cannot move)
  const size_t in_bytes = slot_samples * size_t(bytes_per_sample(in_format));
  const size_t out_rows = p->big ? 1 : size_t(p->max_frames);
  const size_t out_bytes = out_rows * size_t(p->nfft) * sizeof(float);
  auto bail = [&](hipError_t e, const char* what) {
    (void)tdsa_pipe_destroy(q);
    return fail(TDSA_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&q->s_in, hipStreamNonBlocking)) != hipSuccess) return bail(e, "stream");
  if ((e = hipStreamCreateWithFlags(&q->s_out, hipStreamNonBlocking)) != hipSuccess) return bail(e, "stream");
  for (auto& sl : q->slots) {
    if ((e = sl.h_in.alloc(in_bytes, hipHostMallocDefault)) != hipSuccess) return bail(e, "pinned input slot");
    if ((e = sl.d_in.alloc(in_bytes)) != hipSuccess) return bail(e, "device input slot");
    if (q->rows) {
      if (q->rows_host && (e = sl.h_out.alloc(out_bytes / sizeof(float), hipHostMallocDefault)) != hipSuccess)
        return bail(e, "pinned output slot");
      if ((e = sl.d_out.alloc(out_bytes / sizeof(float))) != hipSuccess) return bail(e, "device output slot");
      if (q->rows_u8) {
        if ((e = sl.d_u8.alloc(out_bytes / 4)) != hipSuccess) return bail(e, "device byte rows");
        if ((e = sl.h_u8.alloc(out_bytes / 4, hipHostMallocDefault)) != hipSuccess)
          return bail(e, "pinned byte rows");
      }
    }
    if ((e = hipEventCreateWithFlags(&sl.ev_h2d, hipEventDisableTiming)) != hipSuccess) return bail(e, "event");
    if ((e = hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming)) != hipSuccess) return bail(e, "event");
    if ((e = hipEventCreateWithFlags(&sl.ev_d2h, hipEventDisableTiming)) != hipSuccess) return bail(e, "event");
  }
  *out = q;
  return TDSA_OK;
}

int tdsa_pipe_destroy(tdsa_pipe q) {
  if (!q) return TDSA_OK;
  if (q->plan) (void)hipSetDevice(q->plan->device);
  if (q->s_in) (void)hipStreamSynchronize(q->s_in);
  if (q->plan) (void)tdsa_synchronize(q->plan);
  if (q->s_out) (void)hipStreamSynchronize(q->s_out);
  for (auto& sl : q->slots) {
    if (sl.ev_h2d) (void)hipEventDestroy(sl.ev_h2d);
    if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    if (sl.ev_d2h) (void)hipEventDestroy(sl.ev_d2h);
  }
  if (q->s_in) (void)hipStreamDestroy(q->s_in);
  if (q->s_out) (void)hipStreamDestroy(q->s_out);
  delete q;
  return TDSA_OK;
}

int tdsa_pipe_acquire(tdsa_pipe q, void** host_slot) {
  if (!q || !host_slot) return fail(TDSA_ERR_ARG, "null argument");
  auto& sl = q->slots[q->head % q->slots.size()];
  if (sl.acquired) return fail(TDSA_ERR_STATE, "slot already acquired: submit it first");
  if (sl.in_flight) return fail(TDSA_ERR_STATE, "all %zu slots in flight: collect one first", q->slots.size());
  sl.acquired = true;
  *host_slot = sl.h_in;
  return TDSA_OK;
}

int tdsa_pipe_submit(tdsa_pipe q, size_t n_samples, int hop, int n_frames) {
  if (!q) return fail(TDSA_ERR_ARG, "null pipe");
  auto& sl = q->slots[q->head % q->slots.size()];
  if (!sl.acquired) return fail(TDSA_ERR_STATE, "no acquired slot");
  if (n_samples > q->slot_samples) return fail(TDSA_ERR_ARG, "n_samples=%zu exceeds the slot (%zu)", n_samples, q->slot_samples);
  if (n_frames < 1) return fail(TDSA_ERR_ARG, "n_frames=%d", n_frames);
  tdsa_plan p = q->plan;
  HIPCHK(hipSetDevice(p->device));
  const size_t in_bytes = n_samples * size_t(bytes_per_sample(q->fmt));
  HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, in_bytes, hipMemcpyHostToDevice, q->s_in));
  HIPCHK(hipEventRecord(sl.ev_h2d, q->s_in));
  const int rc = process_dev_impl(p, q->fmt, sl.d_in, n_samples, hop, n_frames, q->rows ? sl.d_out : nullptr,
                                  sl.ev_h2d, sl.ev_done);
  if (rc != TDSA_OK) {
    sl.acquired = false;
    return rc;
  }
  sl.n_frames = p->big ? 1 : n_frames;
  if (q->rows_host) {
    HIPCHK(hipStreamWaitEvent(q->s_out, sl.ev_done, 0));
    HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, size_t(sl.n_frames) * p->nfft * sizeof(float), hipMemcpyDeviceToHost,
                          q->s_out));
    HIPCHK(hipEventRecord(sl.ev_d2h, q->s_out));
  }
  if (q->rows_u8) {   // the read-back leg carries what setImage(img, levels) makes of the rows: a quarter of the bytes
    const size_t cnt = size_t(sl.n_frames) * p->nfft;
    HIPCHK(hipStreamWaitEvent(q->s_out, sl.ev_done, 0));
    HIPCHK(launch_quantize_u8(sl.d_out, sl.d_u8, cnt, q->lo_db, q->hi_db, q->s_out));
    HIPCHK(hipMemcpyAsync(sl.h_u8, sl.d_u8, cnt, hipMemcpyDeviceToHost, q->s_out));
    HIPCHK(hipEventRecord(sl.ev_d2h, q->s_out));
  }
  sl.acquired = false;
  sl.in_flight = true;
  ++q->head;
  ++q->pending;
  return TDSA_OK;
}

static int pipe_collect(tdsa_pipe q, const float** rows_host, const float** rows_dev, int* n_frames,
                        const uint8_t** rows_u8 = nullptr) {
  if (!q) return fail(TDSA_ERR_ARG, "null pipe");
  if (q->pending == 0) return fail(TDSA_ERR_STATE, "nothing submitted");
  auto& sl = q->slots[q->tail % q->slots.size()];
  HIPCHK(hipSetDevice(q->plan->device));
  HIPCHK(hipEventSynchronize(q->rows_host || q->rows_u8 ? sl.ev_d2h : sl.ev_done));
  sl.in_flight = false;
  if (rows_u8) *rows_u8 = sl.h_u8;
  if (rows_host) *rows_host = q->rows_host ? sl.h_out : nullptr;
  if (rows_dev) *rows_dev = q->rows ? sl.d_out : nullptr;
  if (n_frames) *n_frames = sl.n_frames;
  ++q->tail;
  --q->pending;
  return TDSA_OK;
}

int tdsa_pipe_collect(tdsa_pipe q, const float** rows_host, int* n_frames) {
  return pipe_collect(q, rows_host, nullptr, n_frames);
}

int tdsa_pipe_collect_dev(tdsa_pipe q, const float** rows_dev, int* n_frames) {
  if (q && !q->rows) return fail(TDSA_ERR_STATE, "this pipe keeps no dB rows (want_rows = 0)");
  return pipe_collect(q, nullptr, rows_dev, n_frames);
}

int tdsa_pipe_collect_u8(tdsa_pipe q, const uint8_t** rows_host, int* n_frames) {
  if (q && !q->rows_u8) return fail(TDSA_ERR_STATE, "this pipe reads no byte rows back (want_rows != 3)");
  return pipe_collect(q, nullptr, nullptr, n_frames, rows_host);
}

int tdsa_pipe_set_levels(tdsa_pipe q, float min_db, float max_db) {
  if (!q) return fail(TDSA_ERR_ARG, "null pipe");
  if (!(max_db > min_db)) return fail(TDSA_ERR_ARG, "levels (%g, %g): need max > min", double(min_db), double(max_db));
  q->lo_db = min_db;      // slots submitted from now on
  q->hi_db = max_db;
  return TDSA_OK;
}

int tdsa_pipe_pending(tdsa_pipe q, int* pending) {
  if (!q || !pending) return fail(TDSA_ERR_ARG, "null argument");
  *pending = q->pending;
  return TDSA_OK;
}
