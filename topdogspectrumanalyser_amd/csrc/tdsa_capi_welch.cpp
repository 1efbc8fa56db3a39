// tdsa_capi_welch.cpp - partial Welch means leaving / entering a plan (export, combine) and the HIP-IPC peer buffers
// they travel through between the processes of a node.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

// the staging buffer, grown on demand (no stream is drained ahead of the free)
static int welch_stage(tdsa_plan p, size_t bytes) { return p->d_welch.grow(bytes, nullptr); }

extern "C" {

int tdsa_welch_export(tdsa_plan p, void* mean_host, int as_f32, int* count) {
  if (!p || !mean_host) return fail(TDSA_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (count) *count = p->avg_count;
  if (p->avg_count <= 0) return TDSA_OK;
  const size_t n = size_t(p->nfft), nb = n * (as_f32 ? sizeof(float) : sizeof(double));
  const bool from_sum = p->big && p->big_mean_in_sum;
  if (!as_f32 && !from_sum) {       // the state is the float64 mean already
    HIPCHK(hipMemcpyAsync(mean_host, p->d_avg, nb, hipMemcpyDeviceToHost, p->stream));
  } else {
    TRY(welch_stage(p, nb));
    HIPCHK(launch_welch_export(from_sum ? p->d_sum : p->d_avg, from_sum ? double(p->avg_count) : 1.0, p->d_welch, as_f32,
                               (long long)n, p->stream));
    HIPCHK(hipMemcpyAsync(mean_host, p->d_welch, nb, hipMemcpyDeviceToHost, p->stream));
  }
  HIPCHK(hipStreamSynchronize(p->stream));
  return TDSA_OK;
}

int tdsa_welch_export_dev(tdsa_plan p, void* mean_dev, int as_f32, int* count) {
  if (!p || !mean_dev) return fail(TDSA_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (count) *count = p->avg_count;
  if (p->avg_count <= 0) return TDSA_OK;
  const bool from_sum = p->big && p->big_mean_in_sum;
  HIPCHK(launch_welch_export(from_sum ? p->d_sum : p->d_avg, from_sum ? double(p->avg_count) : 1.0, mean_dev, as_f32,
                             (long long)p->nfft, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));     // the caller tells the combining process next: the values must have landed
  return TDSA_OK;
}

// ---- device buffers another process of the node can read in place (HIP IPC; peer reads go over xGMI) ----
int tdsa_peer_alloc(int device_id, size_t bytes, void** dev_ptr, unsigned char* handle64) {
  if (!dev_ptr || !handle64 || bytes == 0) return fail(TDSA_ERR_ARG, "null / empty argument");
  static_assert(sizeof(hipIpcMemHandle_t) == TDSA_PEER_HANDLE_BYTES, "handle size");
  *dev_ptr = nullptr;
  HIPCHK(hipSetDevice(device_id));
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, bytes));
  hipIpcMemHandle_t h;
  const hipError_t e = hipIpcGetMemHandle(&h, d);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(TDSA_ERR_HIP, "hipIpcGetMemHandle: %s", hipGetErrorString(e));
  }
  HIPCHK(hipMemset(d, 0, bytes));
  std::memcpy(handle64, &h, sizeof(h));
  *dev_ptr = d;
  return TDSA_OK;
}

int tdsa_peer_free(int device_id, void* dev_ptr) {
  if (!dev_ptr) return TDSA_OK;
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipFree(dev_ptr));
  return TDSA_OK;
}

int tdsa_peer_can_access(int device_id, int peer_device_id, int* can_access) {
  if (!can_access) return fail(TDSA_ERR_ARG, "null argument");
  *can_access = 0;
  if (device_id == peer_device_id) { *can_access = 1; return TDSA_OK; }
  HIPCHK(hipDeviceCanAccessPeer(can_access, device_id, peer_device_id));
  return TDSA_OK;
}

int tdsa_peer_open(int device_id, const unsigned char* handle64, int owner_device_id, void** dev_ptr) {
  if (!dev_ptr || !handle64) return fail(TDSA_ERR_ARG, "null argument");
  *dev_ptr = nullptr;
  HIPCHK(hipSetDevice(device_id));
  if (owner_device_id >= 0 && owner_device_id != device_id) {
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, device_id, owner_device_id));
    if (!can) return fail(TDSA_ERR_STATE, "device %d cannot read device %d's memory", device_id, owner_device_id);
  }
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle64, sizeof(h));
  void* d = nullptr;
  HIPCHK(hipIpcOpenMemHandle(&d, h, hipIpcMemLazyEnablePeerAccess));
  // probe: a mapping this device cannot read must show up here as an error code, not later as a fault inside a kernel
  unsigned probe = 0;
  const hipError_t e = hipMemcpy(&probe, d, sizeof(probe), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    (void)hipIpcCloseMemHandle(d);
    return fail(TDSA_ERR_HIP, "mapped peer buffer is not readable: %s", hipGetErrorString(e));
  }
  *dev_ptr = d;
  return TDSA_OK;
}

int tdsa_peer_close(int device_id, void* dev_ptr) {
  if (!dev_ptr) return TDSA_OK;
  HIPCHK(hipSetDevice(device_id));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipIpcCloseMemHandle(dev_ptr));
  return TDSA_OK;
}

// parts_host != null: the partial means sit part_stride_bytes apart in host memory and are staged on this device first;
// else parts_dev[r] are device pointers this device can read (its own memory or tdsa_peer_open'ed buffers of other ranks)
static int welch_combine_impl(tdsa_plan p, const void* parts_host, size_t part_stride_bytes, const void* const* parts_dev,
                              const int32_t* counts, int n_parts, int as_f32, float* out_db_dev, float* out_db_host) {
  if (!p || !(parts_host || parts_dev) || !counts) return fail(TDSA_ERR_ARG, "null argument");
  if (n_parts < 1 || n_parts > kWelchMaxParts) return fail(TDSA_ERR_ARG, "n_parts=%d outside [1, %d]", n_parts, kWelchMaxParts);
  const tdsa_mode& m = p->mode;
  const size_t n = size_t(p->nfft), nb = n * (as_f32 ? sizeof(float) : sizeof(double));
  if (parts_host && part_stride_bytes < nb)
    return fail(TDSA_ERR_ARG, "part_stride_bytes=%zu < %zu bytes of one partial", part_stride_bytes, nb);
  long long total = 0;
  int cnt[kWelchMaxParts];
  for (int r = 0; r < n_parts; ++r) {
    if (counts[r] < 0) return fail(TDSA_ERR_ARG, "counts[%d]=%d", r, counts[r]);
    cnt[r] = counts[r];
    total += counts[r];
  }
  if (total == 0) return fail(TDSA_ERR_ARG, "no segments behind the partial means");
  if (!(avg_active(m) && m.avg_mode == TDSA_AVG_LIN && total <= m.avg_n))
    return fail(TDSA_ERR_STATE, "partial means combine only into an uncapped running mean: avg lin with avg_n >= %lld segments", total);
  if (p->chirp) return fail(TDSA_ERR_STATE, "not available for chirp-z plans");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const size_t staged = parts_host ? nb * size_t(n_parts) : 0;
  TRY(welch_stage(p, staged + (out_db_host && !out_db_dev ? n * sizeof(float) : 0)));
  const void* part[kWelchMaxParts];
  if (parts_host) {
    // one strided copy: the parts may sit part_stride_bytes apart in the caller's (pinned, shared) slab
    HIPCHK(hipMemcpy2DAsync(p->d_welch, nb, parts_host, part_stride_bytes, nb, size_t(n_parts), hipMemcpyHostToDevice, p->stream));
    for (int r = 0; r < n_parts; ++r) part[r] = p->d_welch.as<const unsigned char>() + nb * size_t(r);
  } else {
    for (int r = 0; r < n_parts; ++r) {
      if (cnt[r] != 0 && !parts_dev[r]) return fail(TDSA_ERR_ARG, "parts_dev[%d] is null", r);
      part[r] = parts_dev[r];
    }
  }
  float* out_dev = out_db_dev ? out_db_dev
                              : (out_db_host ? reinterpret_cast<float*>(p->d_welch + staged) : nullptr);
  const bool hmax = (m.hold_flags & TDSA_HOLD_MAX) != 0, hmin = (m.hold_flags & TDSA_HOLD_MIN) != 0;
  const float pscale = (p->big && m.db_mode == TDSA_DB_POW) ? m.power_scale : 1.0f;
  HIPCHK(launch_welch_combine(part, cnt, n_parts, as_f32, (long long)n, p->big ? p->d_sum : nullptr,
                              p->big ? nullptr : p->d_avg, int(total), p->big ? 0 : 1, m.db_mode, pscale, m.log_floor,
                              m.cal_offset_db, p->tare_active ? p->d_tare_base : nullptr, out_dev,
                              hmax ? p->d_hold_max : nullptr, hmin ? p->d_hold_min : nullptr, p->held_max == 0,
                              p->held_min == 0, p->stream));
  p->avg_count = int(total);
  if (p->big) p->big_mean_in_sum = true;
  if (hmax) p->held_max += 1;
  if (hmin) p->held_min += 1;
  if (out_db_host) {
    HIPCHK(hipMemcpyAsync(out_db_host, out_dev, n * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
  }
  return TDSA_OK;
}

int tdsa_welch_combine(tdsa_plan p, const void* parts_host, size_t part_stride_bytes, const int32_t* counts, int n_parts,
                       int as_f32, float* out_db_dev, float* out_db_host) {
  if (!parts_host) return fail(TDSA_ERR_ARG, "null argument");
  return welch_combine_impl(p, parts_host, part_stride_bytes, nullptr, counts, n_parts, as_f32, out_db_dev, out_db_host);
}

int tdsa_welch_combine_dev(tdsa_plan p, const void* const* parts_dev, const int32_t* counts, int n_parts, int as_f32,
                           float* out_db_dev, float* out_db_host) {
  if (!parts_dev) return fail(TDSA_ERR_ARG, "null argument");
  return welch_combine_impl(p, nullptr, 0, parts_dev, counts, n_parts, as_f32, out_db_dev, out_db_host);
}

}  // extern "C"
