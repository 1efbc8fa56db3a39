// tdsa_capi_symsync.cpp - tdsa_symsync_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_symsync.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_symsync_record) == sizeof(SymRecord), "the public record is the kernel's");

// ---- symbol recovery (tdsa_symsync.hip) --------------------------------------------------------------------------
struct tdsa_symsync_s : Lane {
  size_t max_host = 0;            // samples one host call stages
  float2* d_nco = nullptr;        // [kSymNcoTable]
  void* h_in = nullptr;           // pinned staging of a host block ...
  float2* d_in = nullptr;
  float2* d_sym = nullptr;        // ... of its symbols and raw symbols, [2][max_host / 4] ...
  void* h_sym = nullptr;
  SymRecord* d_rec = nullptr;     // ... and of the records of either entry point, grown on demand
  size_t rec_cap = 0;
  bool configured = false;
  uint64_t step = 0, delta_fx = 0;
  uint32_t nu = 0;
  int carrier = 0, fixed = 0;   // carrier: the order M, 0 = off
  float ref = 0.0f;

  size_t sym_cap() const { return max_host / 4 + 1; }   // K n_seg < seg_len n_seg / 4
};

namespace {

// the checks both entry points share, before any HIP call; *K_out = symbols per segment
int sym_check(const tdsa_symsync_s* h, const void* in, size_t seg_len, size_t hop, int n_seg, const void* sym,
              size_t out_stride, const void* raw, const void* rec, int* K_out) {
  if (!h) return fail(TDSA_ERR_ARG, "null symbol synchroniser");
  if (!h->configured) return fail(TDSA_ERR_STATE, "not configured: call tdsa_symsync_configure first");
  if (!in) return fail(TDSA_ERR_ARG, "null samples");
  if (!sym) return fail(TDSA_ERR_ARG, "null symbols");
  if (!rec) return fail(TDSA_ERR_ARG, "null records");
  for (const void* p : {in, sym, raw, rec})
    if (reinterpret_cast<uintptr_t>(p) % 8 != 0) return fail(TDSA_ERR_ARG, "pointers must be aligned to 8 bytes");
  if (n_seg < 1) return fail(TDSA_ERR_ARG, "n_seg=%d: at least one segment", n_seg);
  if (hop < 1) return fail(TDSA_ERR_ARG, "hop=%zu: at least one sample", hop);
  const long long K = sym_symbols_per_segment(h->step, seg_len);
  if (K < 2 || K > kSymMaxSymbols)
    return fail(TDSA_ERR_ARG, "seg_len=%zu gives %lld symbols per segment: 2 .. %d", seg_len, K, kSymMaxSymbols);
  if (out_stride < size_t(K)) return fail(TDSA_ERR_ARG, "out_stride=%zu: a segment gives %lld symbols", out_stride, K);
  *K_out = int(K);
  return TDSA_OK;
}

int sym_launch(tdsa_symsync_s* h, hipStream_t s, const void* in, size_t seg_len, size_t hop, int n_seg, void* sym,
               size_t out_stride, void* raw, int K) {
  SymLaunch a;
  a.in = static_cast<const float2*>(in);
  a.seg_len = (long long)seg_len;
  a.hop = (long long)hop;
  a.n_seg = n_seg;
  a.step = h->step;
  a.nu = h->nu;
  a.order = h->carrier;
  a.ref = h->ref;
  a.fixed = h->fixed;
  a.delta_fx = h->delta_fx;
  a.K = K;
  a.log2G = sym_log2_grid(K);
  a.nco = h->d_nco;
  a.sym = static_cast<float2*>(sym);
  a.raw = static_cast<float2*>(raw);
  a.out_stride = (long long)out_stride;
  a.rec = h->d_rec;
  HIPCHK(launch_symsync(a, s));
  return TDSA_OK;
}

}  // namespace

int tdsa_symsync_symbols_per_segment(uint64_t step, size_t seg_len, int* K) {
  if (!K) return fail(TDSA_ERR_ARG, "null K");
  if (step < kSymMinStep || step > kSymMaxStep)
    return fail(TDSA_ERR_ARG, "step=%llu: 4 .. 64 samples per symbol in 32.32 fixed point", (unsigned long long)step);
  const long long k = sym_symbols_per_segment(step, seg_len);
  *K = k < 0 ? 0 : k > 0x7fffffff ? 0x7fffffff : int(k);
  return TDSA_OK;
}

int tdsa_symsync_create(int device_id, size_t max_host_samples, tdsa_symsync* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (max_host_samples < 16) return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least 16", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  {
    const hipError_t e = symsync_prepare();
    if (e != hipSuccess)
      return fail(TDSA_ERR_HIP, "symsync create: the device refuses %d bytes of LDS per workgroup: %s",
                  kSymMaxLdsBytes - kSymStaticLdsBytes, hipGetErrorString(e));
  }
  tdsa_symsync h = new (std::nothrow) tdsa_symsync_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->max_host = max_host_samples;
  // (cos, -sin) of 2 pi k / 4096 from the first quarter turn, so that whole quarter turns are exact
  std::vector<float2> nco(kSymNcoTable);
  const int q = kSymNcoTable / 4;
  for (int k = 0; k < kSymNcoTable; ++k) {
    const double th = 2.0 * 3.14159265358979323846 * double(k % q) / double(kSymNcoTable);
    const float c = k % q ? float(std::cos(th)) : 1.0f, s = k % q ? float(std::sin(th)) : 0.0f;
    const float cs[4] = {c, -s, -c, s}, sn[4] = {s, c, -s, -c};   // cos, sin of th + quarter turns
    nco[k] = make_float2(cs[k / q], -sn[k / q]);
  }
  const size_t sym_bytes = 2 * h->sym_cap() * sizeof(float2);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_nco), kSymNcoTable * sizeof(float2));
  if (e == hipSuccess) e = hipHostMalloc(&h->h_in, max_host_samples * sizeof(float2), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_in), max_host_samples * sizeof(float2));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_sym), sym_bytes);
  if (e == hipSuccess) e = hipHostMalloc(&h->h_sym, sym_bytes, hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->d_nco, nco.data(), kSymNcoTable * sizeof(float2), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the host copy of the table is released
  if (e != hipSuccess) {
    (void)tdsa_symsync_destroy(h);
    return fail(TDSA_ERR_HIP, "symsync create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_symsync_destroy(tdsa_symsync h) {
  if (!h) return TDSA_OK;
  h->drain();
  free_all({h->d_nco, h->d_in, h->d_sym, h->d_rec});
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_sym) (void)hipHostFree(h->h_sym);
  h->close();
  delete h;
  return TDSA_OK;
}

int tdsa_symsync_configure(tdsa_symsync h, uint64_t step, uint32_t nu, int order, double ref_arg, int timing_mode,
                           uint64_t delta_fx) {
  if (step < kSymMinStep || step > kSymMaxStep)
    return fail(TDSA_ERR_ARG, "step=%llu: 4 .. 64 samples per symbol in 32.32 fixed point", (unsigned long long)step);
  const unsigned __int128 turn = (unsigned __int128)1 << 64;
  const uint64_t want = uint64_t((turn + step / 2) / step);   // round(2^32 / sps)
  if (uint64_t(nu) + 1 < want || uint64_t(nu) > want + 1)
    return fail(TDSA_ERR_ARG, "nu=%u: the phase step of this symbol rate is %llu", nu, (unsigned long long)want);
  if (order != 0 && order != 2 && order != 4 && order != 8) return fail(TDSA_ERR_ARG, "order=%d: 0, 2, 4 or 8", order);
  if (!std::isfinite(ref_arg)) return fail(TDSA_ERR_ARG, "ref_arg is not finite");
  if (timing_mode != TDSA_SYMSYNC_AUTO && timing_mode != TDSA_SYMSYNC_FIXED)
    return fail(TDSA_ERR_ARG, "timing_mode=%d: TDSA_SYMSYNC_AUTO or _FIXED", timing_mode);
  if (timing_mode == TDSA_SYMSYNC_FIXED && (delta_fx < kSymOne || delta_fx >= step + kSymOne))
    return fail(TDSA_ERR_ARG, "delta_fx=%llu: 2^32 <= delta_fx < step + 2^32", (unsigned long long)delta_fx);
  if (!h) return fail(TDSA_ERR_ARG, "null symbol synchroniser");
  h->step = step;
  h->nu = nu;
  h->carrier = order;
  h->ref = float(ref_arg / 3.14159265358979323846);
  h->fixed = timing_mode == TDSA_SYMSYNC_FIXED;
  h->delta_fx = h->fixed ? delta_fx : 0;
  h->configured = true;
  return TDSA_OK;
}

int tdsa_symsync_process(tdsa_symsync h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                         void* sym_host, size_t out_stride, void* raw_host, tdsa_symsync_record* records_host) {
  int K = 0;
  TRY(sym_check(h, in_host, seg_len, hop, n_seg, sym_host, out_stride, raw_host, records_host, &K));
  if ((size_t(n_seg) - 1) * hop + seg_len > n_samples)
    return fail(TDSA_ERR_ARG, "%d segments of %zu samples every %zu need %zu samples, the block has %zu", n_seg, seg_len,
                hop, (size_t(n_seg) - 1) * hop + seg_len, n_samples);
  if (n_samples > h->max_host || size_t(n_seg) * seg_len > h->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples in %d segments of %zu, the handle stages at most %zu "
                "(max_host_samples)", n_samples, n_seg, seg_len, h->max_host);
  TRY(h->own_stream());
  TRY(grow_device(&h->d_rec, &h->rec_cap, size_t(n_seg), h->stream, sizeof(SymRecord)));
  std::memcpy(h->h_in, in_host, n_samples * sizeof(float2));   // the previous host call has waited: the staging is free
  HIPCHK(hipMemcpyAsync(h->d_in, h->h_in, n_samples * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  // staged rows are K wide, back to back
  const size_t rows = size_t(n_seg) * size_t(K);
  float2* d_raw = raw_host ? h->d_sym + h->sym_cap() : nullptr;
  TRY(sym_launch(h, h->stream, h->d_in, seg_len, hop, n_seg, h->d_sym, size_t(K), d_raw, K));
  TRY(h->done(h->stream));
  char* hs = static_cast<char*>(h->h_sym);
  HIPCHK(hipMemcpyAsync(hs, h->d_sym, rows * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  if (raw_host)
    HIPCHK(hipMemcpyAsync(hs + h->sym_cap() * sizeof(float2), d_raw, rows * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(SymRecord), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t s = 0; s < size_t(n_seg); ++s) {
    std::memcpy(static_cast<float2*>(sym_host) + s * out_stride, hs + s * K * sizeof(float2), size_t(K) * sizeof(float2));
    if (raw_host)
      std::memcpy(static_cast<float2*>(raw_host) + s * out_stride, hs + (h->sym_cap() + s * K) * sizeof(float2),
                  size_t(K) * sizeof(float2));
  }
  return TDSA_OK;
}

int tdsa_symsync_process_dev(tdsa_symsync h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                             void* sym_dev, size_t out_stride, void* raw_dev, tdsa_symsync_record* records_host) {
  int K = 0;
  TRY(sym_check(h, in_dev, seg_len, hop, n_seg, sym_dev, out_stride, raw_dev, records_host, &K));
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and symbol synchroniser live on different devices");
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  TRY(h->order(s));
  TRY(grow_device(&h->d_rec, &h->rec_cap, size_t(n_seg), h->last, sizeof(SymRecord)));
  TRY(sym_launch(h, s, in_dev, seg_len, hop, n_seg, sym_dev, out_stride, raw_dev, K));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(SymRecord), hipMemcpyDeviceToHost, s));
  TRY(h->done(s));
  HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
  return TDSA_OK;
}

int tdsa_symsync_timer_begin(tdsa_symsync h) { return Lane::timer_begin(h, "symbol synchroniser"); }

int tdsa_symsync_timer_end(tdsa_symsync h, float* elapsed_ms) { return Lane::timer_end(h, "symbol synchroniser", elapsed_ms); }
