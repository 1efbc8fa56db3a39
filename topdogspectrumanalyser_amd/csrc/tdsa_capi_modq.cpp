// tdsa_capi_modq.cpp - tdsa_modq_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_modq.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_modq_record) == sizeof(ModqRecord), "the public record is the kernel's");
static_assert(TDSA_MODQ_MAX_POINTS == kModqMaxPoints && TDSA_MODQ_MAX_SYMBOLS == kModqMaxSymbols, "the public limits are the kernel's");
static_assert(TDSA_MODQ_NONFINITE == kModqFlagNonFinite && TDSA_MODQ_DEGENERATE == kModqFlagDegenerate &&
                  TDSA_MODQ_ONE_POINT == kModqFlagOnePoint, "the flags are the kernel's");

// ---- modulation quality (tdsa_modq.hip) ---------------------------------------------------------------------------
// The handle holds the table on the device, the staging of a host block, the outputs of a host call (the error vectors,
// then the indices, K wide back to back, grown on demand) and the records of either entry point.  There is no symbol
// clock: the segments are rows of symbols already.
struct tdsa_modq_s : Lane {
  size_t max_host = 0;             // symbols one host call stages
  Staging in;
  Dev<ModqTable> d_tab;
  bool has_points = false;
  Dev<char> d_rec;
  Dev<char> d_out;
  Pinned<char> h_out;

  hipError_t launch(hipStream_t s, const void* in, int K, size_t in_stride, int n_seg, void* idx, size_t out_stride, void* err) {
    ModqLaunch a;
    a.in = static_cast<const float2*>(in);
    a.in_stride = (long long)in_stride;
    a.n_seg = n_seg;
    a.K = K;
    a.table = d_tab;
    a.idx = static_cast<uint8_t*>(idx);
    a.err = static_cast<float2*>(err);
    a.out_stride = (long long)out_stride;
    a.rec = d_rec.as<ModqRecord>();
    return launch_modq(a, s);
  }
};

namespace {

constexpr const char* kWho = "modulation quality handle";

// The checks both entry points share, in one order: K, in_stride, n_seg, out_stride, which need no handle; then null
// handle, no table, the null pointers, alignment.  None of them makes a HIP call.
int modq_check(const tdsa_modq_s* h, const void* in, int K, size_t in_stride, int n_seg, const void* idx, size_t out_stride,
               const void* err, const void* rec, bool dev) {
  if (K < kModqMinSymbols || K > kModqMaxSymbols)
    return fail(TDSA_ERR_ARG, "K=%d: %d .. %d symbols per segment", K, kModqMinSymbols, kModqMaxSymbols);
  if (in_stride < 1) return fail(TDSA_ERR_ARG, "in_stride=%zu: at least one symbol", in_stride);
  if (n_seg < 1) return fail(TDSA_ERR_ARG, "n_seg=%d: at least one segment", n_seg);
  if (out_stride < size_t(K)) return fail(TDSA_ERR_ARG, "out_stride=%zu: a segment gives %d symbols", out_stride, K);
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  if (!h->has_points) return fail(TDSA_ERR_ARG, "no reference points: call tdsa_modq_set_points first");
  if (!in) return fail(TDSA_ERR_ARG, "null symbols");
  if (!idx) return fail(TDSA_ERR_ARG, "null indices");
  if (!rec) return fail(TDSA_ERR_ARG, "null records");
  if (dev && reinterpret_cast<uintptr_t>(in) % 8 != 0)
    return fail(TDSA_ERR_ARG, "symbols pointer must be aligned to one complex64 symbol (8 bytes)");
  if (dev && reinterpret_cast<uintptr_t>(err) % 8 != 0)
    return fail(TDSA_ERR_ARG, "errors pointer must be aligned to one complex64 error vector (8 bytes)");
  if (reinterpret_cast<uintptr_t>(rec) % 8 != 0) return fail(TDSA_ERR_ARG, "records must be aligned to 8 bytes");
  return TDSA_OK;
}

}  // namespace

int tdsa_modq_create(int device_id, size_t max_host_symbols, tdsa_modq* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (max_host_symbols < 2) return fail(TDSA_ERR_ARG, "max_host_symbols=%zu: at least 2", max_host_symbols);
  HIPCHK(hipSetDevice(device_id));
  tdsa_modq h = new (std::nothrow) tdsa_modq_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->max_host = max_host_symbols;
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = h->in.alloc(max_host_symbols * sizeof(float2));
  if (e == hipSuccess) e = h->d_tab.alloc(1);
  if (e != hipSuccess) {
    (void)tdsa_modq_destroy(h);
    return fail(TDSA_ERR_HIP, "modq create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_modq_destroy(tdsa_modq h) {
  if (!h) return TDSA_OK;
  h->drain();
  delete h;
  return TDSA_OK;
}

int tdsa_modq_set_points(tdsa_modq h, const float* points, int n_points) {
  if (n_points < 1 || n_points > kModqMaxPoints)
    return fail(TDSA_ERR_ARG, "n_points=%d: 1 .. %d reference points", n_points, kModqMaxPoints);
  if (!points) return fail(TDSA_ERR_ARG, "null points");
  double power = 0.0;
  for (int i = 0; i < n_points; ++i) {
    if (!std::isfinite(points[2 * i]) || !std::isfinite(points[2 * i + 1])) return fail(TDSA_ERR_ARG, "point %d is not finite", i);
    power += double(points[2 * i]) * double(points[2 * i]) + double(points[2 * i + 1]) * double(points[2 * i + 1]);
  }
  if (!(power > 0.0)) return fail(TDSA_ERR_ARG, "every reference point is zero");
  if (!h) return fail(TDSA_ERR_ARG, "null %s", kWho);
  ModqTable t = {};
  for (int i = 0; i < n_points; ++i) {
    t.r[i] = make_float2(points[2 * i], points[2 * i + 1]);
    t.r_abs[i] = modq_abs32(ModqC32{points[2 * i], points[2 * i + 1]});
  }
  t.inv_rho = float(1.0 / std::sqrt(power / double(n_points)));
  t.T = n_points;
  TRY(h->own_stream());            // behind the last launch, which reads the table it was launched with
  HIPCHK(hipMemcpyAsync(h->d_tab, &t, sizeof(ModqTable), hipMemcpyHostToDevice, h->stream));
  TRY(h->done(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // t is released
  h->has_points = true;
  return TDSA_OK;
}

int tdsa_modq_process(tdsa_modq h, const void* in_host, size_t n_symbols, int K, size_t in_stride, int n_seg,
                      uint8_t* idx_host, size_t out_stride, void* err_host, tdsa_modq_record* records_host) {
  TRY(modq_check(h, in_host, K, in_stride, n_seg, idx_host, out_stride, err_host, records_host, false));
  // in_stride first, so that the product below cannot wrap
  if (size_t(K) > n_symbols || (n_seg > 1 && in_stride > (n_symbols - size_t(K)) / (size_t(n_seg) - 1)))
    return fail(TDSA_ERR_ARG, "%d segments of %d symbols every %zu need %zu symbols, the block has %zu", n_seg, K, in_stride,
                (size_t(n_seg) - 1) * in_stride + size_t(K), n_symbols);
  if (n_symbols > h->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu symbols, the handle stages at most %zu (max_host_symbols)", n_symbols, h->max_host);
  TRY(h->own_stream());
  const size_t rows = size_t(n_seg) * size_t(K), idx_at = err_host ? rows * sizeof(float2) : 0, bytes = idx_at + rows;
  TRY(h->d_rec.grow(size_t(n_seg) * sizeof(ModqRecord), h->stream));
  TRY(h->d_out.grow(bytes, h->stream));
  TRY(h->h_out.grow(bytes, h->stream));
  // the previous host call has waited: the staging is free
  TRY(h->in.fill(h->stream, in_host, 1, n_symbols, n_symbols, sizeof(float2)));
  HIPCHK(h->launch(h->stream, h->in.d_in, K, in_stride, n_seg, h->d_out + idx_at, size_t(K), err_host ? h->d_out : nullptr));
  TRY(h->done(h->stream));
  HIPCHK(hipMemcpyAsync(h->h_out, h->d_out, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(ModqRecord), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const char* ho = static_cast<const char*>(h->h_out);
  for (size_t s = 0; s < size_t(n_seg); ++s) {
    std::memcpy(idx_host + s * out_stride, ho + idx_at + s * size_t(K), size_t(K));
    if (err_host)
      std::memcpy(static_cast<char*>(err_host) + s * out_stride * sizeof(float2), ho + s * size_t(K) * sizeof(float2),
                  size_t(K) * sizeof(float2));
  }
  return TDSA_OK;
}

int tdsa_modq_process_dev(tdsa_modq h, tdsa_plan p, const void* in_dev, int K, size_t in_stride, int n_seg, void* idx_dev,
                          size_t out_stride, void* err_dev, tdsa_modq_record* records_host) {
  TRY(modq_check(h, in_dev, K, in_stride, n_seg, idx_dev, out_stride, err_dev, records_host, true));
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and %s live on different devices", kWho);
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  TRY(h->order(s));
  TRY(h->d_rec.grow(size_t(n_seg) * sizeof(ModqRecord), h->last));
  HIPCHK(h->launch(s, in_dev, K, in_stride, n_seg, idx_dev, out_stride, err_dev));
  HIPCHK(hipMemcpyAsync(records_host, h->d_rec, size_t(n_seg) * sizeof(ModqRecord), hipMemcpyDeviceToHost, s));
  TRY(h->done(s));
  HIPCHK(hipStreamSynchronize(s));   // the records are the call's result: they are in the caller's memory on return
  return TDSA_OK;
}

int tdsa_modq_timer_begin(tdsa_modq h) { return Lane::timer_begin(h, kWho); }

int tdsa_modq_timer_end(tdsa_modq h, float* elapsed_ms) { return Lane::timer_end(h, kWho, elapsed_ms); }
