// tdsa_capi_fsk.cpp - tdsa_fsk_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_fsk.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_fsk_record) == sizeof(FskRecord), "the public record is the kernel's");
static_assert(TDSA_FSK_IQ == kFskIq && TDSA_FSK_FREQ == kFskFreq, "the input kinds are the kernel's");

// ---- FSK analysis (tdsa_fsk.hip) ---------------------------------------------------------------------------------
struct tdsa_fsk_s : SegAnalyser {
  static constexpr SegNames who = {"FSK analyser", "fsk", "FSK", "levels"};
  // levels are float32, their indices bytes
  static constexpr size_t out_unit = sizeof(float), aux_unit = 1, rec_unit = sizeof(FskRecord);
  int levels = 2, kind = kFskIq, boxcar = 1, lag = 1;

  size_t in_unit() const { return kind == kFskIq ? sizeof(float2) : sizeof(float); }
  long long symbols(size_t seg_len) const { return fsk_symbols_per_segment(step, seg_len, kind, boxcar); }
  int aligned(const void* in, const void* out, const void*, const void* rec) const {
    if (reinterpret_cast<uintptr_t>(in) % in_unit() != 0)
      return fail(TDSA_ERR_ARG, "input pointer must be aligned to one %s (%zu bytes)",
                  kind == kFskIq ? "complex64 sample" : "float32", in_unit());
    if (reinterpret_cast<uintptr_t>(out) % 4 != 0) return fail(TDSA_ERR_ARG, "output pointer must be aligned to one float32 (4 bytes)");
    if (reinterpret_cast<uintptr_t>(rec) % 8 != 0) return fail(TDSA_ERR_ARG, "records must be aligned to 8 bytes");
    return TDSA_OK;
  }
  hipError_t launch(hipStream_t s, const void* in, size_t seg_len, size_t hop, int n_seg, void* out, size_t out_stride,
                    void* idx, int K) {
    FskLaunch a;
    a.in = in;
    a.seg_len = (long long)seg_len;
    a.hop = (long long)hop;
    a.n_seg = n_seg;
    a.kind = kind;
    a.step = step;
    a.nu = nu;
    a.levels = levels;
    a.boxcar = boxcar;
    a.lag = lag;
    a.fixed = fixed;
    a.delta_fx = delta_fx;
    a.K = K;
    a.nco = d_nco;
    a.out = static_cast<float*>(out);
    a.idx = static_cast<uint8_t*>(idx);
    a.out_stride = (long long)out_stride;
    a.rec = d_rec.as<FskRecord>();
    return launch_fsk(a, s);
  }
};

namespace {

int fsk_check_kind(int kind) {
  if (kind != TDSA_FSK_IQ && kind != TDSA_FSK_FREQ)
    return fail(TDSA_ERR_ARG, "input_kind=%d: TDSA_FSK_IQ or _FREQ", kind);
  return TDSA_OK;
}
int fsk_check_boxcar(int boxcar) {
  if (boxcar < 1 || boxcar > kFskMaxBoxcar) return fail(TDSA_ERR_ARG, "boxcar=%d: 1 .. %d samples", boxcar, kFskMaxBoxcar);
  return TDSA_OK;
}

}  // namespace

int tdsa_fsk_symbols_per_segment(uint64_t step, size_t seg_len, int input_kind, int boxcar, int* K) {
  if (!K) return fail(TDSA_ERR_ARG, "null K");
  TRY(SegAnalyser::check_step(step));
  TRY(fsk_check_kind(input_kind));
  TRY(fsk_check_boxcar(boxcar));
  *K = SegAnalyser::clamp_k(fsk_symbols_per_segment(step, seg_len, input_kind, boxcar));
  return TDSA_OK;
}

int tdsa_fsk_create(int device_id, size_t max_host_samples, tdsa_fsk* out) {
  return SegAnalyser::create(device_id, max_host_samples, out, [] { return TDSA_OK; });
}

int tdsa_fsk_destroy(tdsa_fsk h) { return SegAnalyser::destroy(h); }

int tdsa_fsk_configure(tdsa_fsk h, uint64_t step, uint32_t nu, int levels, int input_kind, int boxcar, int lag,
                       int timing_mode, uint64_t delta_fx) {
  TRY(SegAnalyser::check_rate(step, nu));
  if (levels != 2 && levels != 4 && levels != 8) return fail(TDSA_ERR_ARG, "levels=%d: 2, 4 or 8", levels);
  TRY(fsk_check_kind(input_kind));
  TRY(fsk_check_boxcar(boxcar));
  if (lag < 1 || lag > kFskMaxLag) return fail(TDSA_ERR_ARG, "lag=%d: 1 .. %d samples", lag, kFskMaxLag);
  TRY(SegAnalyser::check_timing(tdsa_fsk_s::who, step, timing_mode, delta_fx));
  TRY(SegAnalyser::set_clock(h, tdsa_fsk_s::who, step, nu, timing_mode, delta_fx));
  h->levels = levels;
  h->kind = input_kind;
  h->boxcar = boxcar;
  h->lag = lag;
  return TDSA_OK;
}

int tdsa_fsk_process(tdsa_fsk h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                     float* out_host, size_t out_stride, uint8_t* idx_host, tdsa_fsk_record* records_host) {
  return SegAnalyser::host(h, in_host, n_samples, seg_len, hop, n_seg, out_host, out_stride, idx_host, records_host);
}

int tdsa_fsk_process_dev(tdsa_fsk h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                         void* out_dev, size_t out_stride, void* idx_dev, tdsa_fsk_record* records_host) {
  return SegAnalyser::dev(h, p, in_dev, seg_len, hop, n_seg, out_dev, out_stride, idx_dev, records_host);
}

int tdsa_fsk_timer_begin(tdsa_fsk h) { return Lane::timer_begin(h, tdsa_fsk_s::who.handle); }

int tdsa_fsk_timer_end(tdsa_fsk h, float* elapsed_ms) { return Lane::timer_end(h, tdsa_fsk_s::who.handle, elapsed_ms); }
