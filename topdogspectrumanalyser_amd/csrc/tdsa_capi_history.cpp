// tdsa_capi_history.cpp - tdsa_history_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_history.hpp"

using namespace tdsa;

static_assert(sizeof(tdsa_history_info) == 48, "tdsa_history_info is part of the ABI");
static_assert(sizeof(tdsa_history_out) == 64, "tdsa_history_out is part of the ABI");

// ---- 3-D history views: trace ring, hold row, ribbon / line-stack / surface passes (tdsa_history.hip) ----------------
struct tdsa_history_s : Lane {         // its stream: host pushes, views, the timer
  int depth = 0, n = 0, kind = TDSA_HIST_HEIGHTS;
  double ref_level = 0.0, range_db = 100.0;
  long long pushed = 0;               // rows since the last reset
  int head = 0;                       // slot of the next row
  int has_min = 0;                    // the newest push brought a min trace
  hipEvent_t ev_in = nullptr;         // the last host rows have left their pinned staging
  Dev<float> d_ring;                  // [depth][n]
  Dev<float> d_hold;                  // [n]
  Dev<float> d_min;                   // [n]
  Dev<unsigned long long> d_keys;         // [depth] maximum and first index of each slot's row
  Pinned<char> h_in;                  // pinned staging of one host push: live, max, min rows ...
  Dev<float> d_in;                    // ... and where they land
  Dev<unsigned char> d_tmp;           // what one view needs beside its destinations
  Pinned<char> h_small;               // pinned: the scalars one view reads back
};

namespace {

constexpr int kHistMaxPushRows = 1 << 20;

struct Small {   // the scalars of a view, in device memory at the start of d_tmp
  unsigned long long live_key;
  float hold_value;
  int hold_bin;
};
constexpr size_t kSmallBytes = 256;

int hist_check(tdsa_history h) { return h ? TDSA_OK : fail(TDSA_ERR_ARG, "null history"); }

// enqueue n_rows rows at `rows` (device) on stream s
int hist_run(tdsa_history h, hipStream_t s, const float* rows, int n_rows, const float* hold_in, const float* min_in,
             int update_hold) {
  TRY(h->order(s));
  const int skip = n_rows > h->depth ? n_rows - h->depth : 0;
  const int first = (h->head + skip) % h->depth, count = n_rows - skip;   // the slots this push writes: their keys start at 0
  const int piece = count < h->depth - first ? count : h->depth - first;
  HIPCHK(hipMemsetAsync(h->d_keys + first, 0, size_t(piece) * 8, s));
  if (count > piece) HIPCHK(hipMemsetAsync(h->d_keys, 0, size_t(count - piece) * 8, s));
  HistPush a;
  a.in = rows;
  a.hold_in = hold_in;
  a.min_in = min_in;
  a.ring = h->d_ring;
  a.hold = h->d_hold;
  a.min_out = h->d_min;
  a.keys = h->d_keys;
  a.n = h->n;
  a.depth = h->depth;
  a.head = h->head;
  a.n_rows = n_rows;
  a.skip = skip;
  a.heights = h->kind == TDSA_HIST_HEIGHTS;
  a.update_hold = update_hold;
  a.bottom = float(h->ref_level - h->range_db);
  a.range = float(h->range_db);
  a.zscale = 8.0f;
  HIPCHK(launch_hist_push(a, s));
  TRY(h->done(s));
  h->head = int((static_cast<long long>(h->head) + n_rows) % h->depth);
  h->pushed += n_rows;
  h->has_min = a.heights && min_in != nullptr;
  return TDSA_OK;
}

size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

// the view's scratch: `bytes[k]` each on a 256-byte boundary behind the scalars; at[k] receives the pointers
int hist_scratch(tdsa_history h, const size_t* bytes, int k, unsigned char** at) {
  size_t need = kSmallBytes;
  for (int i = 0; i < k; ++i) need += round256(bytes[i]);
  TRY(h->d_tmp.grow(need, h->stream));
  size_t off = kSmallBytes;
  for (int i = 0; i < k; ++i) {
    at[i] = bytes[i] ? h->d_tmp + off : nullptr;
    off += round256(bytes[i]);
  }
  return TDSA_OK;
}

HistSrc hist_ring_src(tdsa_history h, int first) {
  HistSrc s;
  s.base = h->d_ring;
  s.n = h->n;
  s.depth = h->depth;
  s.head = h->head;
  s.first = first;
  return s;
}

HistSrc hist_linear_src(const float* base, int n) {
  HistSrc s;
  s.base = base;
  s.n = n;
  s.linear = 1;
  return s;
}

int hist_check_view(tdsa_history h, int columns, const tdsa_history_out* out, const tdsa_history_info* info) {
  TRY(hist_check(h));
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  if (!info) return fail(TDSA_ERR_ARG, "null info");
  if (columns < 0 || columns > h->n) return fail(TDSA_ERR_ARG, "columns=%d: 0 (every bin) or 1 .. %d", columns, h->n);
  if (out->on_device != 0 && out->on_device != 1) return fail(TDSA_ERR_ARG, "on_device=%d: 0 / 1", out->on_device);
  if (out->on_device)
    for (const void* p : {(const void*)out->primary, (const void*)out->colours, (const void*)out->bins, (const void*)out->hold,
                          (const void*)out->hold_bins, (const void*)out->min_row, (const void*)out->min_bins})
      if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return fail(TDSA_ERR_ARG, "device destinations must be aligned to 16 bytes");
  return TDSA_OK;
}

// a result that was computed at `src` (device) goes to the caller's `dst`, host or device; nothing if it is the place
int hist_deliver(tdsa_history h, const tdsa_history_out* out, void* dst, const void* src, size_t bytes) {
  if (!dst || dst == src || bytes == 0) return TDSA_OK;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, out->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  return TDSA_OK;
}

// the scalars every view reports; synchronises the handle's stream
int hist_finish(tdsa_history h, tdsa_history_info* info, int rows, int cols, int first, bool hold_peak) {
  Small* d = h->d_tmp.as<Small>();
  if (h->pushed > 0) {
    const int newest = (h->head - 1 + h->depth) % h->depth;
    HIPCHK(hipMemcpyAsync(&d->live_key, h->d_keys + newest, 8, hipMemcpyDeviceToDevice, h->stream));
  }
  if (hold_peak) {
    HistReduce r;
    r.src = hist_linear_src(h->d_hold, h->n);
    r.rows = 1;
    r.columns = 1;
    r.vals = &d->hold_value;
    r.bins = &d->hold_bin;
    HIPCHK(launch_hist_reduce(r, h->stream));
  }
  TRY(h->done(h->stream));
  HIPCHK(hipMemcpyAsync(h->h_small, d, sizeof(Small), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  Small sm;
  std::memcpy(&sm, h->h_small, sizeof(sm));
  std::memset(info, 0, sizeof(*info));
  info->pushed = h->pushed;
  info->rows = rows;
  info->cols = cols;
  const long long held = h->pushed < h->depth ? h->pushed : h->depth;
  info->valid_rows = int(held - first > 0 ? (held - first < rows ? held - first : rows) : 0);
  info->has_min = h->has_min;
  if (h->pushed > 0) hist_key_decode(sm.live_key, &info->live_value, &info->live_bin);
  if (hold_peak) {
    info->hold_value = sm.hold_value;
    info->hold_bin = sm.hold_bin;
  }
  return TDSA_OK;
}

// one row (hold, min trace) as it is or reduced, delivered to `dst` / `dst_bins`
int hist_row_out(tdsa_history h, const tdsa_history_out* out, const float* row, int columns, float* d_vals, int* d_bins,
                 float* dst, int* dst_bins) {
  if (!dst && !dst_bins) return TDSA_OK;
  if (columns == 0) return hist_deliver(h, out, dst, row, size_t(h->n) * 4);
  HistReduce r;
  r.src = hist_linear_src(row, h->n);
  r.rows = 1;
  r.columns = columns;
  r.vals = d_vals;
  r.bins = d_bins;
  HIPCHK(launch_hist_reduce(r, h->stream));
  TRY(hist_deliver(h, out, dst, d_vals, size_t(columns) * 4));
  return hist_deliver(h, out, dst_bins, d_bins, size_t(columns) * 4);
}

}  // namespace

int tdsa_history_create(int device_id, int depth, int n_bins, int kind, tdsa_history* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (kind != TDSA_HIST_HEIGHTS && kind != TDSA_HIST_LEVELS) return fail(TDSA_ERR_ARG, "kind=%d: TDSA_HIST_HEIGHTS / _LEVELS", kind);
  if (n_bins < 2) return fail(TDSA_ERR_ARG, "n_bins=%d: at least 2", n_bins);
  if (depth < 1 || static_cast<long long>(depth) * n_bins > kHistMaxCells)
    return fail(TDSA_ERR_ARG, "depth=%d, n_bins=%d: depth >= 1, depth * n_bins <= %lld", depth, n_bins, kHistMaxCells);
  HIPCHK(hipSetDevice(device_id));
  tdsa_history h = new (std::nothrow) tdsa_history_s();
  if (!h) return fail(TDSA_ERR_NOMEM, "out of host memory");
  h->device = device_id;
  h->depth = depth;
  h->n = n_bins;
  h->kind = kind;
  const size_t cells = size_t(depth) * size_t(n_bins);
  hipError_t e = h->open(true);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = h->d_ring.alloc(cells);
  if (e == hipSuccess) e = h->d_hold.alloc(size_t(n_bins));
  if (e == hipSuccess) e = h->d_min.alloc(size_t(n_bins));
  if (e == hipSuccess) e = h->d_keys.alloc(size_t(depth));
  if (e == hipSuccess) e = h->h_small.alloc(kSmallBytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)tdsa_history_destroy(h);
    return fail(TDSA_ERR_HIP, "history create: %s", hipGetErrorString(e));
  }
  const int rc = tdsa_history_reset(h);
  if (rc != TDSA_OK) {
    (void)tdsa_history_destroy(h);
    return rc;
  }
  *out = h;
  return TDSA_OK;
}

int tdsa_history_destroy(tdsa_history h) {
  if (!h) return TDSA_OK;
  h->drain();
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  delete h;
  return TDSA_OK;
}

int tdsa_history_set_amplitude(tdsa_history h, double ref_level, double range_db) {
  TRY(hist_check(h));
  if (!std::isfinite(ref_level) || !std::isfinite(range_db))
    return fail(TDSA_ERR_ARG, "ref_level=%g, range_db=%g: finite", ref_level, range_db);
  if (h->kind == TDSA_HIST_HEIGHTS && !(range_db > 0.0)) return fail(TDSA_ERR_ARG, "range_db=%g: above 0 for heights", range_db);
  h->ref_level = ref_level;   // rows already in the ring keep their z
  h->range_db = range_db;
  return TDSA_OK;
}

int tdsa_history_reset(tdsa_history h) {
  TRY(hist_check(h));
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_ring, 0, size_t(h->depth) * size_t(h->n) * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->d_hold, 0, size_t(h->n) * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->d_min, 0, size_t(h->n) * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->d_keys, 0, size_t(h->depth) * 8, h->stream));
  h->pushed = 0;
  h->head = 0;
  h->has_min = 0;
  return h->done(h->stream);
}

int tdsa_history_reset_hold(tdsa_history h) {
  TRY(hist_check(h));
  TRY(h->own_stream());
  HIPCHK(hipMemsetAsync(h->d_hold, 0, size_t(h->n) * 4, h->stream));
  return h->done(h->stream);
}

int tdsa_history_push(tdsa_history h, const float* live_host, const float* max_host, const float* min_host, int update_hold) {
  TRY(hist_check(h));
  if (!live_host) return fail(TDSA_ERR_ARG, "null row");
  if (h->kind != TDSA_HIST_HEIGHTS && (max_host || min_host)) return fail(TDSA_ERR_ARG, "max / min traces go with heights only");
  TRY(h->own_stream());
  const size_t n = size_t(h->n), row = round256(n * 4);
  TRY(h->h_in.grow(3 * row, h->stream));
  TRY(h->d_in.grow(3 * row / 4, h->stream));
  HIPCHK(hipEventSynchronize(h->ev_in));   // the previous rows have left the staging
  unsigned char* st = h->h_in.as<unsigned char>();
  const int k = min_host ? 3 : max_host ? 2 : 1;
  std::memcpy(st, live_host, n * 4);
  if (max_host) std::memcpy(st + row, max_host, n * 4);
  if (min_host) std::memcpy(st + 2 * row, min_host, n * 4);
  HIPCHK(hipMemcpyAsync(h->d_in, st, size_t(k) * row, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->ev_in, h->stream));
  return hist_run(h, h->stream, h->d_in, 1, max_host ? h->d_in + row / 4 : nullptr, min_host ? h->d_in + 2 * row / 4 : nullptr,
                  update_hold != 0);
}

int tdsa_history_push_dev(tdsa_history h, tdsa_plan p, const float* rows_dev, int n_rows) {
  TRY(hist_check(h));
  if (n_rows < 0 || n_rows > kHistMaxPushRows) return fail(TDSA_ERR_ARG, "n_rows=%d: 0 .. %d", n_rows, kHistMaxPushRows);
  if (n_rows > 0 && !rows_dev) return fail(TDSA_ERR_ARG, "null rows");
  if (reinterpret_cast<uintptr_t>(rows_dev) % 4 != 0) return fail(TDSA_ERR_ARG, "rows pointer must be aligned to one float");
  if (p && p->device != h->device) return fail(TDSA_ERR_ARG, "plan and history live on different devices");
  if (n_rows == 0) return TDSA_OK;
  hipStream_t s;
  TRY(h->producer_stream(p, &s));
  return hist_run(h, s, rows_dev, n_rows, nullptr, nullptr, 1);
}

int tdsa_history_ribbon(tdsa_history h, const float* x_host, int columns, const tdsa_history_out* out, tdsa_history_info* info) {
  TRY(hist_check_view(h, columns, out, info));
  if (h->kind != TDSA_HIST_HEIGHTS) return fail(TDSA_ERR_ARG, "the ribbon view needs a history of heights");
  if (!x_host) return fail(TDSA_ERR_ARG, "null x");
  TRY(h->own_stream());
  const int rows = h->depth < kHistRibbonRows ? h->depth : kHistRibbonRows;
  const int cols = columns ? columns : h->n;
  const size_t cells = size_t(rows) * size_t(cols);
  const bool own = !out->on_device;
  const size_t bytes[5] = {size_t(h->n) * 4, columns ? cells * 4 : 0, columns ? cells * 4 : 0,
                           own || !out->primary ? cells * 24 : 0, own || !out->colours ? cells * 32 : 0};
  unsigned char* at[5];
  TRY(hist_scratch(h, bytes, 5, at));
  HIPCHK(hipMemcpyAsync(at[0], x_host, size_t(h->n) * 4, hipMemcpyHostToDevice, h->stream));
  HistRibbon a;
  a.src = hist_ring_src(h, 0);
  if (columns) {
    HistReduce r;
    r.src = a.src;
    r.rows = rows;
    r.columns = columns;
    r.vals = reinterpret_cast<float*>(at[1]);
    r.bins = reinterpret_cast<int*>(at[2]);
    HIPCHK(launch_hist_reduce(r, h->stream));
    a.src = hist_linear_src(r.vals, columns);
    a.bins = r.bins;
  }
  a.rows = rows;
  a.x = reinterpret_cast<const float*>(at[0]);
  a.verts = at[3] ? reinterpret_cast<float*>(at[3]) : static_cast<float*>(out->primary);
  a.colours = at[4] ? reinterpret_cast<float*>(at[4]) : static_cast<float*>(out->colours);
  for (int r = 0; r < kHistRibbonRows; ++r) {   // Ribbon._row_verts_colors: the row's scalars, in double
    const double age = double(r) / 29.0;
    const double y_front = r * 0.7, y_back = y_front + 0.7 * 0.85;
    double val = 1.0 - age * 0.6;
    val = val < 0.3 ? 0.3 : val > 1.0 ? 1.0 : val;
    const double alpha = 1.0 - age * 0.5 > 0.3 ? 1.0 - age * 0.5 : 0.3;
    a.row[r] = {float(y_front), float(y_back), float(0.3 + 0.7 * age), float(alpha), val};
  }
  HIPCHK(launch_hist_ribbon(a, h->stream));
  TRY(hist_deliver(h, out, out->primary, a.verts, cells * 24));
  TRY(hist_deliver(h, out, out->colours, a.colours, cells * 32));
  if (columns) TRY(hist_deliver(h, out, out->bins, a.bins, cells * 4));
  return hist_finish(h, info, rows, cols, 0, false);
}

int tdsa_history_lines(tdsa_history h, int first, int count, int colour_mode, const float* palette_host, int columns,
                       const tdsa_history_out* out, tdsa_history_info* info) {
  TRY(hist_check_view(h, columns, out, info));
  if (h->kind != TDSA_HIST_HEIGHTS) return fail(TDSA_ERR_ARG, "the line stack needs a history of heights");
  if (colour_mode != TDSA_HIST_COLOUR_INDEX && colour_mode != TDSA_HIST_COLOUR_RGBA)
    return fail(TDSA_ERR_ARG, "colour_mode=%d: TDSA_HIST_COLOUR_INDEX / _RGBA", colour_mode);
  if (colour_mode == TDSA_HIST_COLOUR_RGBA && !palette_host) return fail(TDSA_ERR_ARG, "null palette");
  if (first < 0 || count < 0 || first > h->depth || count > h->depth - first)
    return fail(TDSA_ERR_ARG, "first=%d, count=%d: lines 0 .. %d", first, count, h->depth);
  TRY(h->own_stream());
  const int cols = columns ? columns : h->n;
  const size_t cells = size_t(count) * size_t(cols);
  const size_t px = colour_mode == TDSA_HIST_COLOUR_RGBA ? 16 : 1;
  const bool own = !out->on_device;
  const size_t bytes[8] = {columns ? cells * 4 : 0, columns ? cells * 4 : 0, own || !out->primary ? cells * 4 : 0,
                           own || !out->colours ? cells * px : 0, columns ? size_t(cols) * 4 : 0, columns ? size_t(cols) * 4 : 0,
                           columns ? size_t(cols) * 4 : 0, columns ? size_t(cols) * 4 : 0};
  unsigned char* at[8];
  TRY(hist_scratch(h, bytes, 8, at));
  const long long held = h->pushed < h->depth ? h->pushed : h->depth;
  if (count > 0) {
    HistLines a;
    a.src = hist_ring_src(h, first);
    if (columns) {
      HistReduce r;
      r.src = a.src;
      r.rows = count;
      r.columns = columns;
      r.vals = reinterpret_cast<float*>(at[0]);
      r.bins = reinterpret_cast<int*>(at[1]);
      HIPCHK(launch_hist_reduce(r, h->stream));
      a.src = hist_linear_src(r.vals, columns);
      TRY(hist_deliver(h, out, out->bins, r.bins, cells * 4));
    }
    a.rows = count;
    a.valid = int(held - first > 0 ? held - first : 0);
    a.rgba = colour_mode == TDSA_HIST_COLOUR_RGBA;
    a.z = at[2] ? reinterpret_cast<float*>(at[2]) : static_cast<float*>(out->primary);
    a.colours = at[3] ? static_cast<void*>(at[3]) : out->colours;
    std::memset(a.palette, 0, sizeof(a.palette));
    if (a.rgba) std::memcpy(a.palette, palette_host, sizeof(a.palette));
    HIPCHK(launch_hist_lines(a, h->stream));
    TRY(hist_deliver(h, out, out->primary, a.z, cells * 4));
    TRY(hist_deliver(h, out, out->colours, a.colours, cells * px));
  }
  TRY(hist_row_out(h, out, h->d_hold, columns, reinterpret_cast<float*>(at[4]), reinterpret_cast<int*>(at[5]), out->hold,
                   out->hold_bins));
  if (h->has_min)
    TRY(hist_row_out(h, out, h->d_min, columns, reinterpret_cast<float*>(at[6]), reinterpret_cast<int*>(at[7]), out->min_row,
                     out->min_bins));
  return hist_finish(h, info, count, cols, first, true);
}

int tdsa_history_surface(tdsa_history h, int columns, const tdsa_history_out* out, tdsa_history_info* info) {
  TRY(hist_check_view(h, columns, out, info));
  if (h->kind != TDSA_HIST_LEVELS) return fail(TDSA_ERR_ARG, "the surface view needs a history of levels");
  TRY(h->own_stream());
  const int rows = h->depth, cols = columns ? columns : h->n;
  const size_t cells = size_t(rows) * size_t(cols);
  const bool own = !out->on_device;
  const size_t bytes[4] = {columns ? cells * 4 : 0, columns ? cells * 4 : 0, own || !out->primary ? cells * 4 : 0,
                           own || !out->colours ? cells * 12 : 0};
  unsigned char* at[4];
  TRY(hist_scratch(h, bytes, 4, at));
  HistSurface a;
  a.src = hist_ring_src(h, 0);
  if (columns) {
    HistReduce r;
    r.src = a.src;
    r.rows = rows;
    r.columns = columns;
    r.vals = reinterpret_cast<float*>(at[0]);
    r.bins = reinterpret_cast<int*>(at[1]);
    HIPCHK(launch_hist_reduce(r, h->stream));
    a.src = hist_linear_src(r.vals, columns);
    TRY(hist_deliver(h, out, out->bins, r.bins, cells * 4));
  }
  const double zmin = h->ref_level - h->range_db, zmax = h->ref_level;
  a.rows = rows;
  a.flat = zmax == zmin;
  a.zmin = zmin;
  a.span = zmax - zmin;
  a.z = at[2] ? reinterpret_cast<float*>(at[2]) : static_cast<float*>(out->primary);
  a.colours = at[3] ? reinterpret_cast<float*>(at[3]) : static_cast<float*>(out->colours);
  HIPCHK(launch_hist_surface(a, h->stream));
  TRY(hist_deliver(h, out, out->primary, a.z, cells * 4));
  TRY(hist_deliver(h, out, out->colours, a.colours, cells * 12));
  TRY(hist_finish(h, info, rows, cols, 0, false));
  float t = 0.5f;   // the widget's marker: from the float32 live row, so in float32 (the grid comes from float64)
  if (!a.flat) {
    t = (info->live_value - float(zmin)) / float(zmax - zmin);
    t = t >= 0.f ? (t <= 1.f ? t : 1.f) : 0.f;
  }
  info->live_norm = double(t);
  return TDSA_OK;
}

int tdsa_history_timer_begin(tdsa_history h) {
  TRY(hist_check(h));
  return Lane::timer_begin(h, "history");
}

int tdsa_history_timer_end(tdsa_history h, float* elapsed_ms) {
  TRY(hist_check(h));
  return Lane::timer_end(h, "history", elapsed_ms);
}
