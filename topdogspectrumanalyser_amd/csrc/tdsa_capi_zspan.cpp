// tdsa_capi_zspan.cpp - tdsa_zspan_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_zerospan.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_zspan_info) == 64, "tdsa_zspan_info is part of the ABI");

// ---- zero span: detector ring, trigger search, trace view (tdsa_zerospan.hip) ---------------------------------------
struct tdsa_zspan_s : Lane {           // its stream: host pushes, views, the timer
  long long cap = 0;
  size_t max_host = 0;
  hipEvent_t ev_in = nullptr;         // the last host chunk has left its pinned staging
  int detector = TDSA_ZS_DET_REAL;
  float log_floor = 0.f, offset_db = 0.f;
  long long total = 0;                // samples pushed since the last reset
  Dev<float> d_ring;                  // [cap]; absolute sample t lives at t % cap
  Pinned<char> h_in;                  // pinned staging of one host chunk (up to 8 bytes per sample) ...
  Dev<char> d_in;                     // ... and where it lands
  Dev<unsigned char> d_res;           // ZsCtrl, kZsMaxBlocks ZsPart, then the trace of a view without a device pointer
  Pinned<char> h_res;                 // pinned: what one view reads back
};

namespace {

constexpr size_t kZsBounceMax = size_t(8) << 20;   // traces up to 8 MiB come back through the pinned block, larger ones directly

int zspan_check_format(int fmt) {
  if (fmt >= TDSA_IN_I8 && fmt <= TDSA_IN_F32R) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "in_format=%d: TDSA_IN_I8 / _U8 / _C64 / _F32R", fmt);
}

int zspan_check_detector(int det) {
  if (det >= TDSA_ZS_DET_REAL && det <= TDSA_ZS_DET_DB) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "detector=%d: TDSA_ZS_DET_REAL / _MAG / _DB", det);
}

// common checks of both push entry points (before any HIP call)
int zspan_check_push(tdsa_zspan z, int fmt, const void* src, size_t n) {
  TRY(zspan_check_format(fmt));
  if (!z) return fail(TDSA_ERR_ARG, "null zero span");
  if (n > 0 && !src) return fail(TDSA_ERR_ARG, "null samples");
  return TDSA_OK;
}

// enqueue the detector over n samples at `dev` on stream s: the last `cap` of them, in up to two contiguous pieces
int zspan_run(tdsa_zspan z, hipStream_t s, int fmt, const void* dev, size_t n) {
  TRY(z->order(s));
  const long long skip = (long long)n > z->cap ? (long long)n - z->cap : 0;
  long long left = (long long)n - skip;
  long long t = z->total + skip;
  const unsigned char* src = static_cast<const unsigned char*>(dev) + size_t(skip) * bytes_per_sample(fmt);
  while (left > 0) {
    const long long pos = t % z->cap;
    const long long piece = left < z->cap - pos ? left : z->cap - pos;
    ZsPush a;
    a.in = src;
    a.out = z->d_ring + pos;
    a.n = piece;
    a.fmt = fmt;
    a.detector = z->detector;
    a.log_floor = z->log_floor;
    a.offset_db = z->offset_db;
    HIPCHK(launch_zspan_push(a, s));
    src += size_t(piece) * bytes_per_sample(fmt);
    t += piece;
    left -= piece;
  }
  TRY(z->done(s));
  z->total += (long long)n;
  return TDSA_OK;
}

}  // namespace

int tdsa_zspan_create(int device_id, size_t capacity, size_t max_host_samples, tdsa_zspan* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (capacity < size_t(kZsMinCapacity) || capacity > size_t(kZsMaxCapacity))
    return fail(TDSA_ERR_ARG, "capacity=%zu: %lld .. %lld", capacity, kZsMinCapacity, kZsMaxCapacity);
  if (max_host_samples < 1) return fail(TDSA_ERR_ARG, "max_host_samples=%zu", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_zspan z = new (std::nothrow) tdsa_zspan_s();
  if (!z) return fail(TDSA_ERR_NOMEM, "out of host memory");
  z->device = device_id;
  z->cap = (long long)capacity;
  z->max_host = max_host_samples;
  hipError_t e = z->open(true);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&z->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = z->d_ring.alloc(capacity);
  if (e == hipSuccess) e = z->h_in.alloc(max_host_samples * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = z->d_in.alloc(max_host_samples * 8);
  if (e != hipSuccess) {
    (void)tdsa_zspan_destroy(z);
    return fail(TDSA_ERR_HIP, "zero span create: %s", hipGetErrorString(e));
  }
  *out = z;
  return TDSA_OK;
}

int tdsa_zspan_destroy(tdsa_zspan z) {
  if (!z) return TDSA_OK;
  z->drain();
  if (z->ev_in) (void)hipEventDestroy(z->ev_in);
  delete z;
  return TDSA_OK;
}

int tdsa_zspan_set_detector(tdsa_zspan z, int detector, float log_floor, float offset_db) {
  TRY(zspan_check_detector(detector));
  if (!z) return fail(TDSA_ERR_ARG, "null zero span");
  if (detector == TDSA_ZS_DET_DB && (!(log_floor >= 0.f) || !std::isfinite(log_floor) || !std::isfinite(offset_db)))
    return fail(TDSA_ERR_ARG, "log_floor=%g (finite, >= 0), offset_db=%g (finite)", log_floor, offset_db);
  z->detector = detector;
  z->log_floor = log_floor;
  z->offset_db = offset_db;
  return tdsa_zspan_reset(z);
}

int tdsa_zspan_reset(tdsa_zspan z) {
  if (!z) return fail(TDSA_ERR_ARG, "null zero span");
  z->total = 0;   // launches in flight keep their own positions; later ones are ordered behind them
  return TDSA_OK;
}

int tdsa_zspan_push(tdsa_zspan z, int in_format, const void* samples_host, size_t n) {
  TRY(zspan_check_push(z, in_format, samples_host, n));
  if (n == 0) return TDSA_OK;
  TRY(z->own_stream());
  const size_t bps = size_t(bytes_per_sample(in_format));
  const unsigned char* src = static_cast<const unsigned char*>(samples_host);
  if (n > size_t(z->cap)) {   // only the last `capacity` samples can be seen again
    const size_t skip = n - size_t(z->cap);
    src += skip * bps;
    z->total += (long long)skip;
    n -= skip;
  }
  for (size_t done = 0; done < n; done += z->max_host) {
    const size_t k = n - done < z->max_host ? n - done : z->max_host;
    HIPCHK(hipEventSynchronize(z->ev_in));   // the previous chunk has left the staging
    std::memcpy(z->h_in, src + done * bps, k * bps);
    HIPCHK(hipMemcpyAsync(z->d_in, z->h_in, k * bps, hipMemcpyHostToDevice, z->stream));
    HIPCHK(hipEventRecord(z->ev_in, z->stream));
    TRY(zspan_run(z, z->stream, in_format, z->d_in, k));
  }
  return TDSA_OK;
}

int tdsa_zspan_push_dev(tdsa_zspan z, tdsa_plan p, int in_format, const void* samples_dev, size_t n) {
  TRY(zspan_check_push(z, in_format, samples_dev, n));
  if (p && p->device != z->device) return fail(TDSA_ERR_ARG, "plan and zero span live on different devices");
  if ((reinterpret_cast<uintptr_t>(samples_dev) % uintptr_t(bytes_per_sample(in_format))) != 0)
    return fail(TDSA_ERR_ARG, "samples pointer must be aligned to one sample (%d bytes)", bytes_per_sample(in_format));
  if (n == 0) return TDSA_OK;
  hipStream_t s;
  TRY(z->producer_stream(p, &s));
  return zspan_run(z, s, in_format, samples_dev, n);
}

int tdsa_zspan_view(tdsa_zspan z, int mode, double level, size_t n_display, int n_points, int col_detector,
                    tdsa_zspan_info* info, float* out_host, float* out_dev) {
  if (mode < TDSA_ZS_FREE_RUN || mode > TDSA_ZS_FALL) return fail(TDSA_ERR_ARG, "mode=%d: TDSA_ZS_FREE_RUN / _RISE / _FALL", mode);
  if (n_points < 0 || n_points > kZsMaxPoints) return fail(TDSA_ERR_ARG, "n_points=%d: 0 .. %d", n_points, kZsMaxPoints);
  if (col_detector < TDSA_ZS_COL_MINMAX || col_detector > TDSA_ZS_COL_MEAN)
    return fail(TDSA_ERR_ARG, "col_detector=%d: TDSA_ZS_COL_MINMAX / _SAMPLE / _MEAN", col_detector);
  if (n_display < 1 || n_display > size_t(kZsMaxCapacity))
    return fail(TDSA_ERR_ARG, "n_display=%zu: 1 .. %lld", n_display, kZsMaxCapacity);
  if (!z) return fail(TDSA_ERR_ARG, "null zero span");
  if (!info) return fail(TDSA_ERR_ARG, "null info");
  if (out_dev && (reinterpret_cast<uintptr_t>(out_dev) % 4) != 0) return fail(TDSA_ERR_ARG, "output pointer must be aligned to one float");
  // the host half of the contract
  const long long total = z->total, held = total < z->cap ? total : z->cap, base = total - held;
  const long long nd = (long long)n_display;
  const int length = int(held < nd ? held : nd);
  const int P = n_points == 0 ? 0 : (n_points < length ? n_points : length);
  std::memset(info, 0, sizeof(*info));
  info->total = total;
  info->length = length;
  info->n_columns = P;
  info->start = held < nd ? base : total - nd;
  info->min = info->max = NAN;
  info->mean = NAN;
  if (length == 0) return TDSA_OK;
  const float level32 = float(level);
  long long ss = 0, n_pairs = 0;
  if (held >= nd && mode != TDSA_ZS_FREE_RUN) {
    const long long se = held - nd;
    ss = se - 8 * nd > 0 ? se - 8 * nd : 0;
    n_pairs = se - 1 - ss > 0 ? se - 1 - ss : 0;   // i = ss .. se - 2
  }
  const size_t out_floats = P == 0 ? size_t(length) : size_t(P) * (col_detector == TDSA_ZS_COL_MINMAX ? 2 : 1);
  TRY(z->own_stream());
  TRY(z->d_res.grow(kZsOutOffset + (out_dev ? 0 : out_floats) * sizeof(float), z->stream));
  ZsCtrl* ctrl = z->d_res.as<ZsCtrl>();
  float* d_out = out_dev ? out_dev : reinterpret_cast<float*>(z->d_res + kZsOutOffset);
  HIPCHK(hipMemsetAsync(z->d_res, 0, kZsCtrlZeroed, z->stream));
  if (n_pairs > 0) {
    ZsTrigger t;
    t.ring = z->d_ring;
    t.cap = z->cap;
    t.first = base + ss;
    t.ss = ss;
    t.n_pairs = n_pairs;
    t.level = level32;
    t.fall = mode == TDSA_ZS_FALL;
    t.ctrl = ctrl;
    HIPCHK(launch_zspan_trigger(t, z->stream));
  }
  ZsView v;
  v.ring = z->d_ring;
  v.cap = z->cap;
  v.base = base;
  v.free_start = info->start;
  v.use_trig = n_pairs > 0;
  v.length = length;
  v.level = level32;
  v.columns = P;
  v.col_detector = col_detector;
  v.ctrl = ctrl;
  v.part = reinterpret_cast<ZsPart*>(z->d_res + sizeof(ZsCtrl));
  v.out = d_out;
  v.blocks = zs_view_blocks(v);
  HIPCHK(launch_zspan_view(v, z->stream));
  TRY(z->done(z->stream));
  // one read-back: the control block, the partials and - when it is ours and small - the trace behind them
  const size_t head_bytes = sizeof(ZsCtrl) + size_t(v.blocks) * sizeof(ZsPart);
  const bool bounce = out_host && !out_dev && out_floats * sizeof(float) <= kZsBounceMax;
  const size_t back = bounce ? kZsOutOffset + out_floats * sizeof(float) : head_bytes;
  TRY(z->h_res.grow(back, nullptr));
  HIPCHK(hipMemcpyAsync(z->h_res, z->d_res, back, hipMemcpyDeviceToHost, z->stream));
  if (out_host && !bounce)
    HIPCHK(hipMemcpyAsync(out_host, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, z->stream));
  HIPCHK(hipStreamSynchronize(z->stream));
  const unsigned char* h = z->h_res.as<const unsigned char>();
  if (bounce) std::memcpy(out_host, h + kZsOutOffset, out_floats * sizeof(float));
  ZsCtrl c;
  std::memcpy(&c, h, sizeof(c));
  const ZsPart* part = reinterpret_cast<const ZsPart*>(h + sizeof(ZsCtrl));
  float mn = part[0].mn, mx = part[0].mx;
  double sum = part[0].sum;
  bool nan = std::isnan(mn);
  for (int b = 1; b < v.blocks; ++b) {   // block order
    nan = nan || std::isnan(part[b].mn);
    mn = std::fmin(mn, part[b].mn);
    mx = std::fmax(mx, part[b].mx);
    sum += part[b].sum;
  }
  info->start = c.start;
  info->triggered = c.triggered;
  info->min = nan ? NAN : mn;
  info->max = nan ? NAN : mx;
  info->mean = sum / double(length);
  info->n_at_or_above = (long long)c.n_ge;
  info->n_rise = c.n_rise;
  info->n_fall = c.n_fall;
  return TDSA_OK;
}

int tdsa_zspan_timer_begin(tdsa_zspan z) { return Lane::timer_begin(z, "zero span"); }

int tdsa_zspan_timer_end(tdsa_zspan z, float* elapsed_ms) { return Lane::timer_end(z, "zero span", elapsed_ms); }
