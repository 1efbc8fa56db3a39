// tdsa_capi_symsync.cpp - tdsa_symsync_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_symsync.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_symsync_record) == sizeof(SymRecord), "the public record is the kernel's");

// ---- symbol recovery (tdsa_symsync.hip) --------------------------------------------------------------------------
struct tdsa_symsync_s : SegAnalyser {
  static constexpr SegNames who = {"symbol synchroniser", "symsync", "SYMSYNC", "symbols"};
  // symbols and raw symbols are complex64 as the samples are
  static constexpr size_t out_unit = sizeof(float2), aux_unit = sizeof(float2), rec_unit = sizeof(SymRecord);
  int carrier = 0;   // the order M, 0 = off
  float ref = 0.0f;

  size_t in_unit() const { return sizeof(float2); }
  long long symbols(size_t seg_len) const { return sym_symbols_per_segment(step, seg_len); }
  int aligned(const void* in, const void* sym, const void* raw, const void* rec) const {
    for (const void* p : {in, sym, raw, rec})
      if (reinterpret_cast<uintptr_t>(p) % 8 != 0) return fail(TDSA_ERR_ARG, "pointers must be aligned to 8 bytes");
    return TDSA_OK;
  }
  hipError_t launch(hipStream_t s, const void* in, size_t seg_len, size_t hop, int n_seg, void* sym, size_t out_stride,
                    void* raw, int K) {
    SymLaunch a;
    a.in = static_cast<const float2*>(in);
    a.seg_len = (long long)seg_len;
    a.hop = (long long)hop;
    a.n_seg = n_seg;
    a.step = step;
    a.nu = nu;
    a.order = carrier;
    a.ref = ref;
    a.fixed = fixed;
    a.delta_fx = delta_fx;
    a.K = K;
    a.log2G = sym_log2_grid(K);
    a.nco = d_nco;
    a.sym = static_cast<float2*>(sym);
    a.raw = static_cast<float2*>(raw);
    a.out_stride = (long long)out_stride;
    a.rec = d_rec.as<SymRecord>();
    return launch_symsync(a, s);
  }
};

int tdsa_symsync_symbols_per_segment(uint64_t step, size_t seg_len, int* K) {
  if (!K) return fail(TDSA_ERR_ARG, "null K");
  TRY(SegAnalyser::check_step(step));
  *K = SegAnalyser::clamp_k(sym_symbols_per_segment(step, seg_len));
  return TDSA_OK;
}

int tdsa_symsync_create(int device_id, size_t max_host_samples, tdsa_symsync* out) {
  return SegAnalyser::create(device_id, max_host_samples, out, [] {
    const hipError_t e = symsync_prepare();
    return e == hipSuccess ? TDSA_OK
                           : fail(TDSA_ERR_HIP, "symsync create: the device refuses %d bytes of LDS per workgroup: %s",
                                  kSymMaxLdsBytes - kSymStaticLdsBytes, hipGetErrorString(e));
  });
}

int tdsa_symsync_destroy(tdsa_symsync h) { return SegAnalyser::destroy(h); }

int tdsa_symsync_configure(tdsa_symsync h, uint64_t step, uint32_t nu, int order, double ref_arg, int timing_mode,
                           uint64_t delta_fx) {
  TRY(SegAnalyser::check_rate(step, nu));
  if (order != 0 && order != 2 && order != 4 && order != 8) return fail(TDSA_ERR_ARG, "order=%d: 0, 2, 4 or 8", order);
  if (!std::isfinite(ref_arg)) return fail(TDSA_ERR_ARG, "ref_arg is not finite");
  TRY(SegAnalyser::check_timing(tdsa_symsync_s::who, step, timing_mode, delta_fx));
  TRY(SegAnalyser::set_clock(h, tdsa_symsync_s::who, step, nu, timing_mode, delta_fx));
  h->carrier = order;
  h->ref = float(ref_arg / 3.14159265358979323846);
  return TDSA_OK;
}

int tdsa_symsync_process(tdsa_symsync h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                         void* sym_host, size_t out_stride, void* raw_host, tdsa_symsync_record* records_host) {
  return SegAnalyser::host(h, in_host, n_samples, seg_len, hop, n_seg, sym_host, out_stride, raw_host, records_host);
}

int tdsa_symsync_process_dev(tdsa_symsync h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                             void* sym_dev, size_t out_stride, void* raw_dev, tdsa_symsync_record* records_host) {
  return SegAnalyser::dev(h, p, in_dev, seg_len, hop, n_seg, sym_dev, out_stride, raw_dev, records_host);
}

int tdsa_symsync_timer_begin(tdsa_symsync h) { return Lane::timer_begin(h, tdsa_symsync_s::who.handle); }

int tdsa_symsync_timer_end(tdsa_symsync h, float* elapsed_ms) { return Lane::timer_end(h, tdsa_symsync_s::who.handle, elapsed_ms); }
