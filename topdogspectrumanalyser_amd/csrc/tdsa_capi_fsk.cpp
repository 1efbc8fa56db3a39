// tdsa_capi_fsk.cpp - tdsa_fsk_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_fsk.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_fsk_record) == sizeof(FskRecord), "the public record is the kernel's");
static_assert(TDSA_FSK_IQ == kFskIq && TDSA_FSK_FREQ == kFskFreq, "the input kinds are the kernel's");

// ---- FSK analysis (tdsa_fsk.hip) ---------------------------------------------------------------------------------
struct tdsa_fsk_s : Lane {
  size_t max_host = 0;            // samples one host call stages
  float2* d_nco = nullptr;        // [kFskNcoTable]
  Staging in;                     // of a host block, 8 bytes a sample whichever the kind ...
  float* d_out = nullptr;         // ... of its levels, [max_host / 4 + 1], and their indices behind them ...
  void* h_out = nullptr;
  FskRecord* d_rec = nullptr;     // ... and of the records of either entry point, grown on demand
  size_t rec_cap = 0;
  bool configured = false;
  uint64_t step = 0, delta_fx = 0;
  uint32_t nu = 0;
  int levels = 2, kind = kFskIq, boxcar = 1, lag = 1, fixed = 0;

  size_t out_cap() const { return max_host / 4 + 1; }   // K n_seg < seg_len n_seg / 4
  size_t unit() const { return kind == kFskIq ? sizeof(float2) : sizeof(float); }
};

namespace {

int fsk_check_kind(int kind) {
  if (kind != TDSA_FSK_IQ && kind != TDSA_FSK_FREQ)
    return fail(TDSA_ERR_ARG, "input_kind=%d: TDSA_FSK_IQ or _FREQ", kind);
  return TDSA_OK;
}
int fsk_check_step(uint64_t step) {
  if (step < kFskMinStep || step > kFskMaxStep)
    return fail(TDSA_ERR_ARG, "step=%llu: 4 .. 64 samples per symbol in 32.32 fixed point", (unsigned long long)step);
  return TDSA_OK;
}
int fsk_check_boxcar(int boxcar) {
  if (boxcar < 1 || boxcar > kFskMaxBoxcar) return fail(TDSA_ERR_ARG, "boxcar=%d: 1 .. %d samples", boxcar, kFskMaxBoxcar);
  return TDSA_OK;
}

// the checks both entry points share, before any HIP call; *K_out = symbols per segment
int fsk_check(const tdsa_fsk_s* h, const void* in, size_t seg_len, size_t hop, int n_seg, const void* out,
              size_t out_stride, const void* rec, int* K_out) {
  if (!h) return fail(TDSA_ERR_ARG, "null FSK analyser");
  if (!h->configured) return fail(TDSA_ERR_STATE, "not configured: call tdsa_fsk_configure first");
  if (!in) return fail(TDSA_ERR_ARG, "null samples");
  if (!out) return fail(TDSA_ERR_ARG, "null levels");
  if (!rec) return fail(TDSA_ERR_ARG, "null records");
  if (reinterpret_cast<uintptr_t>(in) % h->unit() != 0)
    return fail(TDSA_ERR_ARG, "input pointer must be aligned to one %s (%zu bytes)",
                h->kind == kFskIq ? "complex64 sample" : "float32", h->unit());
  if (reinterpret_cast<uintptr_t>(out) % 4 != 0) return fail(TDSA_ERR_ARG, "output pointer must be aligned to one float32 (4 bytes)");
  if (reinterpret_cast<uintptr_t>(rec) % 8 != 0) return fail(TDSA_ERR_ARG, "records must be aligned to 8 bytes");
  if (n_seg < 1) return fail(TDSA_ERR_ARG, "n_seg=%d: at least one segment", n_seg);
  if (hop < 1) return fail(TDSA_ERR_ARG, "hop=%zu: at least one sample", hop);
  const long long K = fsk_symbols_per_segment(h->step, seg_len, h->kind, h->boxcar);
  if (K < 2 || K > kFskMaxSymbols)
    return fail(TDSA_ERR_ARG, "seg_len=%zu gives %lld symbols per segment: 2 .. %d", seg_len, K, kFskMaxSymbols);
  if (out_stride < size_t(K)) return fail(TDSA_ERR_ARG, "out_stride=%zu: a segment gives %lld symbols", out_stride, K);
  *K_out = int(K);
  return TDSA_OK;
}

int fsk_launch(tdsa_fsk_s* h, hipStream_t s, const void* in, size_t seg_len, size_t hop, int n_seg, void* out,
               size_t out_stride, void* idx, int K) {
  FskLaunch a;
  a.in = in;
  a.seg_len = (long long)seg_len;
  a.hop = (long long)hop;
  a.n_seg = n_seg;
  a.kind = h->kind;
  a.step = h->step;
  a.nu = h->nu;
  a.levels = h->levels;
  a.boxcar = h->boxcar;
  a.lag = h->lag;
  a.fixed = h->fixed;
  a.delta_fx = h->delta_fx;
  a.K = K;
  a.nco = h->d_nco;
  a.out = static_cast<float*>(out);
  a.idx = static_cast<uint8_t*>(idx);
  a.out_stride = (long long)out_stride;
  a.rec = h->d_rec;
  HIPCHK(launch_fsk(a, s));
  return TDSA_OK;
}

}  // namespace

int tdsa_fsk_symbols_per_segment(uint64_t step, size_t seg_len, int input_kind, int boxcar, int* K) {
  if (!K) return fail(TDSA_ERR_ARG, "null K");
  TRY(fsk_check_step(step));
  TRY(fsk_check_kind(input_kind));
  TRY(fsk_check_boxcar(boxcar));
  const long long k = fsk_symbols_per_segment(step, seg_len, input_kind, boxcar);
  *K = k < 0 ? 0 : k > 0x7fffffff ? 0x7fffffff : int(k);
  return TDSA_OK;
}

int tdsa_fsk_create(int device_id, size_t max_host_samples, tdsa_fsk* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (max_host_samples < 16) return fail(TDSA_ERR_ARG, "max_host_samples=%zu: at least 16", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_fsk h = new (std::nothrow) tdsa_fsk_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->max_host = max_host_samples;
  // (cos, -sin) of 2 pi k / 4096 from the first quarter turn, so that whole quarter turns are exact: the symbol
  // recovery's table
  std::vector<float2> nco(kFskNcoTable);
  const int q = kFskNcoTable / 4;
  for (int k = 0; k < kFskNcoTable; ++k) {
    const double th = 2.0 * 3.14159265358979323846 * double(k % q) / double(kFskNcoTable);
    const float c = k % q ? float(std::cos(th)) : 1.0f, s = k % q ? float(std::sin(th)) : 0.0f;
    const float cs[4] = {c, -s, -c, s}, sn[4] = {s, c, -s, -c};   // cos, sin of th + quarter turns
    nco[k] = make_float2(cs[k / q], -sn[k / q]);
  }
  const size_t out_bytes = h->out_cap() * (sizeof(float) + 1);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_nco), kFskNcoTable * sizeof(float2));
  if (e == hipSuccess) e = h->in.alloc(max_host_samples * sizeof(float2));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_out), out_bytes);
  if (e == hipSuccess) e = hipHostMalloc(&h->h_out, out_bytes, hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->d_nco, nco.data(), kFskNcoTable * sizeof(float2), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the host copy of the table is released
  if (e != hipSuccess) {
    (void)tdsa_fsk_destroy(h);
    return fail(TDSA_ERR_HIP, "fsk create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_fsk_destroy(tdsa_fsk h) {
  if (!h) return TDSA_OK;
  h->drain();
  free_all({h->d_nco, h->d_out, h->d_rec});
  h->in.release();
  if (h->h_out) (void)hipHostFree(h->h_out);
  h->close();
  delete h;
  return TDSA_OK;
}

int tdsa_fsk_configure(tdsa_fsk h, uint64_t step, uint32_t nu, int levels, int input_kind, int boxcar, int lag,
                       int timing_mode, uint64_t delta_fx) {
  TRY(fsk_check_step(step));
  const unsigned __int128 turn = (unsigned __int128)1 << 64;
  const uint64_t want = uint64_t((turn + step / 2) / step);   // round(2^32 / sps)
  if (uint64_t(nu) + 1 < want || uint64_t(nu) > want + 1)
    return fail(TDSA_ERR_ARG, "nu=%u: the phase step of this symbol rate is %llu", nu, (unsigned long long)want);
  if (levels != 2 && levels != 4 && levels != 8) return fail(TDSA_ERR_ARG, "levels=%d: 2, 4 or 8", levels);
  TRY(fsk_check_kind(input_kind));
  TRY(fsk_check_boxcar(boxcar));
  if (lag < 1 || lag > kFskMaxLag) return fail(TDSA_ERR_ARG, "lag=%d: 1 .. %d samples", lag, kFskMaxLag);
  if (timing_mode != TDSA_FSK_AUTO && timing_mode != TDSA_FSK_FIXED)
    return fail(TDSA_ERR_ARG, "timing_mode=%d: TDSA_FSK_AUTO or _FIXED", timing_mode);
  if (timing_mode == TDSA_FSK_FIXED && (delta_fx < kFskOne || delta_fx >= step + kFskOne))
    return fail(TDSA_ERR_ARG, "delta_fx=%llu: 2^32 <= delta_fx < step + 2^32", (unsigned long long)delta_fx);
  if (!h) return fail(TDSA_ERR_ARG, "null FSK analyser");
  h->step = step;
  h->nu = nu;
  h->levels = levels;
  h->kind = input_kind;
  h->boxcar = boxcar;
  h->lag = lag;
  h->fixed = timing_mode == TDSA_FSK_FIXED;
  h->delta_fx = h->fixed ? delta_fx : 0;
  h->configured = true;
  return TDSA_OK;
}

int tdsa_fsk_process(tdsa_fsk h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                     float* out_host, size_t out_stride, uint8_t* idx_host, tdsa_fsk_record* records_host) {
  int K = 0;
  TRY(fsk_check(h, in_host, seg_len, hop, n_seg, out_host, out_stride, records_host, &K));
  // hop first, so that the product below cannot wrap
  if (seg_len > n_samples || (n_seg > 1 && hop > (n_samples - seg_len) / (size_t(n_seg) - 1)))
    return fail(TDSA_ERR_ARG, "%d segments of %zu samples every %zu need %zu samples, the block has %zu", n_seg, seg_len,
                hop, (size_t(n_seg) - 1) * hop + seg_len, n_samples);
  if (n_samples > h->max_host || size_t(n_seg) * seg_len > h->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples in %d segments of %zu, the handle stages at most %zu "
                "(max_host_samples)", n_samples, n_seg, seg_len, h->max_host);
  TRY(h->own_stream());
  TRY(grow_device(&h->d_rec, &h->rec_cap, size_t(n_seg), h->stream, sizeof(FskRecord)));
  // the previous host call has waited: the staging is free
  TRY(h->in.fill(h->stream, in_host, 1, n_samples, n_samples, h->unit()));
  // staged rows are K wide, back to back; the indices lie behind the levels' room
  const size_t rows = size_t(n_seg) * size_t(K);
  uint8_t* d_idx = idx_host ? reinterpret_cast<uint8_t*>(h->d_out + h->out_cap()) : nullptr;
  TRY(fsk_launch(h, h->stream, h->in.d_in, seg_len, hop, n_seg, h->d_out, size_t(K), d_idx, K));
  TRY(h->done(h->stream));
  char* ho = static_cast<char*>(h->h_out);
  char* hi = ho + h->out_cap() * sizeof(float);
  HIPCHK(hipMemcpyAsync(ho, h->d_out, rows * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (idx_host) HIPCHK(hipMemcpyAsync(hi, d_idx, rows, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(FskRecord), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t s = 0; s < size_t(n_seg); ++s) {
    std::memcpy(out_host + s * out_stride, ho + s * K * sizeof(float), size_t(K) * sizeof(float));
    if (idx_host) std::memcpy(idx_host + s * out_stride, hi + s * K, size_t(K));
  }
  return TDSA_OK;
}

int tdsa_fsk_process_dev(tdsa_fsk h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                         void* out_dev, size_t out_stride, void* idx_dev, tdsa_fsk_record* records_host) {
  int K = 0;
  TRY(fsk_check(h, in_dev, seg_len, hop, n_seg, out_dev, out_stride, records_host, &K));
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and FSK analyser live on different devices");
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  TRY(h->order(s));
  TRY(grow_device(&h->d_rec, &h->rec_cap, size_t(n_seg), h->last, sizeof(FskRecord)));
  TRY(fsk_launch(h, s, in_dev, seg_len, hop, n_seg, out_dev, out_stride, idx_dev, K));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(FskRecord), hipMemcpyDeviceToHost, s));
  TRY(h->done(s));
  HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
  return TDSA_OK;
}

int tdsa_fsk_timer_begin(tdsa_fsk h) { return Lane::timer_begin(h, "FSK analyser"); }

int tdsa_fsk_timer_end(tdsa_fsk h, float* elapsed_ms) { return Lane::timer_end(h, "FSK analyser", elapsed_ms); }
