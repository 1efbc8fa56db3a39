// tdsa_capi_constellation.cpp - tdsa_constellation_*.
#include "tdsa_capi_internal.hpp"
#include "tdsa_constellation.hpp"

using namespace tdsa;

// ---- constellation analysis (tdsa_constellation.hip) ---------------------------------------------
struct tdsa_constellation_s : Lane {
  size_t max_host = 0;
  Pinned<char> h_in;             // pinned staging of a host block (up to 8 bytes per sample)
  Dev<char> d_in;
  Dev<char> d_tab;               // [2][kCstMaxPoints] doubles (floats for a float32 table)
  CstTable tab;
  int bins = kCstMaxBins;
  double range = 1.5;
  Dev<float> d_bs_pow;     // per-block sums, grown on demand
  Dev<char> d_bs_evm;
  Dev<float> d_rms;              // per-segment results, grown on demand
  Dev<double> d_evm;
  Dev<unsigned char> d_res;         // the host path's results: evm, rms, counts, tail i[n_tail] then q[n_tail] ...
  Pinned<unsigned char> h_out;      // ... and their pinned read-back (one copy)
};

namespace {

constexpr size_t kCstOutCounts = 16;   // byte offsets in d_res / h_out
constexpr size_t kCstOutTail = kCstOutCounts + size_t(kCstMaxBins) * kCstMaxBins * sizeof(unsigned);

int cst_check_format(int fmt) {
  if (fmt == TDSA_IN_I8 || fmt == TDSA_IN_U8 || fmt == TDSA_IN_C64) return TDSA_OK;
  return fail(TDSA_ERR_ARG, "in_format=%d: the constellation pass takes complex IQ (TDSA_IN_I8 / _U8 / _C64); real input "
              "(the reference's Hilbert transform) is not supported", fmt);
}

// no stream to drain: every call that launches ends with a wait
int cst_reserve(tdsa_constellation c, size_t n_blocks, size_t n_seg) {
  TRY(c->d_bs_pow.grow(n_blocks, nullptr));
  TRY(c->d_bs_evm.grow(n_blocks * sizeof(double), nullptr));
  TRY(c->d_rms.grow(n_seg, nullptr));
  return c->d_evm.grow(n_seg, nullptr);
}

CstLaunch cst_args(tdsa_constellation c, int fmt, const void* in, size_t seg_len, size_t hop, int n_seg) {
  CstLaunch a;
  a.in = in;
  a.fmt = fmt;
  a.seg_len = (long long)seg_len;
  a.hop = (long long)hop;
  a.n_seg = n_seg;
  a.bs_pow = c->d_bs_pow;
  a.bs_evm = c->d_bs_evm;
  a.rms = c->d_rms;
  a.evm = c->d_evm;
  a.bins = c->bins;
  a.range = c->range;
  a.step = (c->range - -c->range) / double(c->bins);   // np.linspace: delta / div
  a.tab = c->tab;
  return a;
}

}  // namespace

int tdsa_constellation_create(int device_id, size_t max_host_samples, tdsa_constellation* out) {
  if (!out) return fail(TDSA_ERR_ARG, "null out");
  *out = nullptr;
  if (max_host_samples < 1) return fail(TDSA_ERR_ARG, "max_host_samples=%zu", max_host_samples);
  HIPCHK(hipSetDevice(device_id));
  tdsa_constellation c = new (std::nothrow) tdsa_constellation_s();
  if (!c) return fail(TDSA_ERR_NOMEM, "out of host memory");
  c->device = device_id;
  c->max_host = max_host_samples;
  const size_t in_bytes = max_host_samples * 8;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = c->h_in.alloc(in_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = c->d_in.alloc(in_bytes);
  if (e == hipSuccess) e = c->d_tab.alloc(2 * kCstMaxPoints * sizeof(double));
  if (e == hipSuccess) e = c->d_res.alloc(kCstOutTail + in_bytes);
  if (e == hipSuccess)
    e = c->h_out.alloc(kCstOutTail + in_bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)tdsa_constellation_destroy(c);
    return fail(TDSA_ERR_HIP, "constellation create: %s", hipGetErrorString(e));
  }
  c->tab.dev = c->d_tab;
  const size_t nblk = (max_host_samples + kCstBlock - 1) / kCstBlock;
  const int rc = cst_reserve(c, nblk, 1);
  if (rc != TDSA_OK) {
    (void)tdsa_constellation_destroy(c);
    return rc;
  }
  *out = c;
  return TDSA_OK;
}

int tdsa_constellation_destroy(tdsa_constellation c) {
  if (!c) return TDSA_OK;
  c->drain();
  delete c;
  return TDSA_OK;
}

int tdsa_constellation_set_refs(tdsa_constellation c, const void* xy, int n_points, int is_f64) {
  if (!c) return fail(TDSA_ERR_ARG, "null constellation");
  if (n_points < 0 || n_points > kCstMaxPoints) return fail(TDSA_ERR_ARG, "n_points=%d: 0 .. %d", n_points, kCstMaxPoints);
  if (n_points > 0 && !xy) return fail(TDSA_ERR_ARG, "null points");
  if (is_f64 != 0 && is_f64 != 1) return fail(TDSA_ERR_ARG, "is_f64=%d", is_f64);
  std::vector<double> px(n_points), py(n_points);
  for (int k = 0; k < n_points; ++k) {
    px[k] = is_f64 ? static_cast<const double*>(xy)[2 * k] : double(static_cast<const float*>(xy)[2 * k]);
    py[k] = is_f64 ? static_cast<const double*>(xy)[2 * k + 1] : double(static_cast<const float*>(xy)[2 * k + 1]);
  }
  // a grid table: the points are exactly the distinct pairs of the distinct x and y levels
  std::vector<double> xs, ys;
  auto add_level = [](std::vector<double>& v, double x) {
    for (double y : v)
      if (y == x) return;
    v.push_back(x);
  };
  bool distinct = true;
  for (int k = 0; k < n_points; ++k) {
    // the kernel's fmin would drop a NaN point where np.min propagates it; the reference has no such table
    if (!std::isfinite(px[k]) || !std::isfinite(py[k]))
      return fail(TDSA_ERR_ARG, "point %d = (%g, %g): reference points must be finite", k, px[k], py[k]);
    add_level(xs, px[k]);
    add_level(ys, py[k]);
    for (int j = 0; j < k; ++j) distinct = distinct && !(px[j] == px[k] && py[j] == py[k]);
  }
  const bool sep = n_points > 0 && distinct && xs.size() * ys.size() == size_t(n_points);
  const std::vector<double>& ax = sep ? xs : px;
  const std::vector<double>& ay = sep ? ys : py;
  double tab[2 * kCstMaxPoints] = {};
  float* tf = reinterpret_cast<float*>(tab);
  for (size_t k = 0; k < ax.size(); ++k) {
    if (is_f64) tab[k] = ax[k];
    else tf[k] = float(ax[k]);
  }
  for (size_t k = 0; k < ay.size(); ++k) {
    if (is_f64) tab[kCstMaxPoints + k] = ay[k];
    else tf[kCstMaxPoints + k] = float(ay[k]);
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->tab.n_points = n_points;
  c->tab.is_f64 = is_f64;
  c->tab.separable = sep ? 1 : 0;
  c->tab.nx = sep ? int(xs.size()) : 0;
  c->tab.ny = sep ? int(ys.size()) : 0;
  return TDSA_OK;
}

int tdsa_constellation_set_density(tdsa_constellation c, double range, int bins) {
  if (!c) return fail(TDSA_ERR_ARG, "null constellation");
  if (bins < 1 || bins > kCstMaxBins) return fail(TDSA_ERR_ARG, "bins=%d: 1 .. %d", bins, kCstMaxBins);
  if (!(range > 0.0) || !std::isfinite(range)) return fail(TDSA_ERR_ARG, "range=%g: need a finite range > 0", range);
  c->bins = bins;
  c->range = range;
  return TDSA_OK;
}

int tdsa_constellation_process(tdsa_constellation c, int in_format, const void* iq_host, size_t n, int n_tail,
                               float* rms, double* evm, int* has_evm, uint32_t* counts, float* tail_iq) {
  if (!c) return fail(TDSA_ERR_ARG, "null constellation");
  TRY(cst_check_format(in_format));
  if (n == 0) return fail(TDSA_ERR_ARG, "empty block");
  if (!iq_host) return fail(TDSA_ERR_ARG, "null samples");
  if (n > c->max_host)
    return fail(TDSA_ERR_ARG, "block of %zu samples, the handle stages at most %zu (max_host_samples)", n, c->max_host);
  if (n_tail < 0) return fail(TDSA_ERR_ARG, "n_tail=%d", n_tail);
  const size_t nt = tail_iq ? (size_t(n_tail) < n ? size_t(n_tail) : n) : 0;
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = n * size_t(bytes_per_sample(in_format));
  std::memcpy(c->h_in, iq_host, bytes);   // the previous call has waited: the staging is free
  HIPCHK(hipMemcpyAsync(c->d_in, c->h_in, bytes, hipMemcpyHostToDevice, c->stream));
  const size_t cnt_bytes = size_t(c->bins) * c->bins * sizeof(unsigned);
  CstLaunch a = cst_args(c, in_format, c->d_in, n, n, 1);
  a.evm = c->d_res.as<double>();
  a.rms = reinterpret_cast<float*>(c->d_res + 8);
  a.counts = counts ? reinterpret_cast<unsigned*>(c->d_res + kCstOutCounts) : nullptr;
  a.tail = nt ? reinterpret_cast<float*>(c->d_res + kCstOutTail) : nullptr;
  a.n_tail = int(nt);
  HIPCHK(launch_constellation(a, c->stream));
  const size_t back = nt ? kCstOutTail + 2 * nt * sizeof(float) : kCstOutCounts + (counts ? cnt_bytes : 0);
  HIPCHK(hipMemcpyAsync(c->h_out, c->d_res, back, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  double e;
  float r;
  std::memcpy(&e, c->h_out, sizeof(e));
  std::memcpy(&r, c->h_out + 8, sizeof(r));
  if (rms) *rms = r;
  if (evm) *evm = e;
  if (has_evm) *has_evm = c->tab.n_points > 0;
  if (counts) std::memcpy(counts, c->h_out + kCstOutCounts, cnt_bytes);
  if (nt) std::memcpy(tail_iq, c->h_out + kCstOutTail, 2 * nt * sizeof(float));
  return TDSA_OK;
}

int tdsa_constellation_process_dev(tdsa_constellation c, tdsa_plan p, int in_format, const void* iq_dev,
                                   size_t seg_len, size_t hop, int n_seg, float* rms_host, double* evm_host,
                                   uint32_t* counts_dev) {
  if (!c) return fail(TDSA_ERR_ARG, "null constellation");
  TRY(cst_check_format(in_format));
  if (!iq_dev) return fail(TDSA_ERR_ARG, "null samples");
  if ((reinterpret_cast<uintptr_t>(iq_dev) % uintptr_t(bytes_per_sample(in_format))) != 0)
    return fail(TDSA_ERR_ARG, "samples pointer must be aligned to one sample (%d bytes)", bytes_per_sample(in_format));
  if (seg_len == 0 || n_seg < 1) return fail(TDSA_ERR_ARG, "seg_len=%zu n_seg=%d: need non-empty segments", seg_len, n_seg);
  if (n_seg > 1 && hop == 0) return fail(TDSA_ERR_ARG, "hop=0 with %d segments", n_seg);
  if (p && p->device != c->device) return fail(TDSA_ERR_ARG, "plan and constellation live on different devices");
  HIPCHK(hipSetDevice(c->device));
  const size_t nblk = (seg_len + kCstBlock - 1) / kCstBlock;
  TRY(cst_reserve(c, nblk * size_t(n_seg), size_t(n_seg)));
  if (p) TRY(plan_order_before(p, c->stream));   // order after the producer
  CstLaunch a = cst_args(c, in_format, iq_dev, seg_len, hop, n_seg);
  a.counts = reinterpret_cast<unsigned*>(counts_dev);
  HIPCHK(launch_constellation(a, c->stream));
  if (rms_host) HIPCHK(hipMemcpyAsync(rms_host, c->d_rms, size_t(n_seg) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (evm_host)
    HIPCHK(hipMemcpyAsync(evm_host, c->d_evm, size_t(n_seg) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDSA_OK;
}
