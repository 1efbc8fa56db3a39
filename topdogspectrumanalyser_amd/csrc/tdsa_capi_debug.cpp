// tdsa_capi_debug.cpp - developer hooks of a plan: knobs, workgroup timeline, launch profiling, timers, shader clock.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

extern "C" {

int tdsa_shader_clock(tdsa_plan p, float* shader_mhz, float* ns_per_valu) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (!p->d_clock) HIPCHK(p->d_clock.alloc(size_t(p->num_cu) * 4));
  const int iters = 4000;                                    // 256 000 instructions per wave: about a millisecond
  HIPCHK(launch_valu_clock(p->d_clock, p->num_cu, 200, p->stream));
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  HIPCHK(launch_valu_clock(p->d_clock, p->num_cu, iters, p->stream));
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipEventSynchronize(p->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  // four waves per SIMD, each 64 * iters instructions: ns per wave-instruction per SIMD; a gfx950 SIMD retires one fp32
  // wave-instruction per 2 clocks (64 FLOP / clk / SIMD as FMAs: MI355X_MICROARCH.md)
  const double ns = double(ms) * 1e6 / (double(iters) * 64.0 * 4.0);
  if (ns_per_valu) *ns_per_valu = float(ns);
  if (shader_mhz) *shader_mhz = float(2.0e3 / ns);
  return TDSA_OK;
}

// developer hook: plan parameters the tools and the tests move to reach code paths that otherwise need other hardware
// or very long batches (rounds 1-4 read them from the environment at plan creation: ADVICE r4)
int tdsa_debug_knob(tdsa_plan p, const char* name, int value) {
  if (!p || !name) return fail(TDSA_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  const std::string k(name);
  if (k == "num_cu") {                       // persistent grids sized for fewer CUs
    if (value < 1 || value > p->num_cu) return fail(TDSA_ERR_ARG, "num_cu=%d outside [1, %d] (it can only shrink: buffers are sized for it)", value, p->num_cu);
    p->num_cu = value;
    p->agg_w_key[0] = -1;
  } else if (k == "avg_wg_min") {            // batches of more frames than this take the workgroup-chunk scan
    if (value < 1) return fail(TDSA_ERR_ARG, "avg_wg_min=%d", value);
    p->avg_wg_min = value;
  } else if (k == "avg_f64_chunks") {        // 1: always the scan over fixed 64-frame chunks with float64 aggregates
    p->avg_f64_chunks = value != 0;
    p->agg_w_key[0] = -1;
  } else if (k == "overlap_share") {         // percent of the CUs an overlapped launch is sized for
    if (value < 10 || value > 100) return fail(TDSA_ERR_ARG, "overlap_share=%d outside [10, 100]", value);
    p->overlap_share = value;
  } else if (k == "big_group") {             // long-frame plans: segments per column / row round (<= the 64 the plan was made for)
    if (!p->big || value < 1 || value > 64) return fail(TDSA_ERR_ARG, "big_group=%d (long-frame plans, 1 .. 64)", value);
    if (p->d_z && value > p->big_group) return fail(TDSA_ERR_STATE, "big_group can only shrink once the plan has run");
    p->big_group = value;
  } else if (k == "big_fuse_gather") {
    p->big_fuse_gather = value;
  } else if (k == "big_queue_gave_up") {       // reads (value ignored): how many workgroups of the fused launch ever gave up waiting - as the error text
    unsigned long long q[4] = {0, 0, 0, 0};
    if (p->d_bigq) { HIPCHK(hipStreamSynchronize(p->stream)); HIPCHK(hipMemcpy(q, p->d_bigq, sizeof(q), hipMemcpyDeviceToHost)); }
    return q[2] == 0 ? TDSA_OK : fail(TDSA_ERR_STATE, "%llu workgroups of a fused row + gather launch gave up waiting", q[2]);
  } else if (k == "smooth") {                // sizes 2^a 3^b 5^c (<= 10 000 in one pass, two passes above): 1 = mixed-radix transform of N points (default), 0 = chirp-z
    p->smooth_on = value != 0;
  } else if (k == "smooth_n1") {             // two-pass sizes: the column pass's transform length (a divisor; both factors <= 10 000)
    if (!p->smooth || p->smooth_n1 == 0) return fail(TDSA_ERR_STATE, "not a two-pass mixed-radix plan");
    if (value < 2 || p->nfft % value != 0 || value > kSmoothMaxN || p->nfft / value > kSmoothMaxN)
      return fail(TDSA_ERR_ARG, "smooth_n1=%d does not split %d into two factors <= %d", value, p->nfft, kSmoothMaxN);
    p->smooth_n1 = value;
    p->smooth_n2 = p->nfft / value;
    p->smooth_stages = smooth_radices(p->smooth_n1, p->smooth_radix);
    p->smooth_stages2 = smooth_radices(p->smooth_n2, p->smooth_radix2);
  } else if (k == "chirp_fuse_big") {        // long chirp-z frames: 1 = element-wise passes inside the column passes (default)
    p->chirp_fuse_big = value != 0;
  } else if (k == "chirp_single") {          // chirp-z plans: 1 = one launch per call (default), 0 = the separate passes
    p->chirp_single = value != 0;
#ifdef TDSA_DEV
  } else if (k == "cu_mask") {               // the plan's stream confined to a set of CUs (tools/c5_two_plans.py): 1 / 2 = mask words
    // 0-3 / 4-7 (four whole XCDs each on this chip), 3 / 4 = every second CU (even / odd bits of all eight words)
    if (value < 1 || value > 4) return fail(TDSA_ERR_ARG, "cu_mask=%d outside [1, 4]", value);
    uint32_t mask[8];
    for (int w = 0; w < 8; ++w)
      mask[w] = value == 1 ? (w < 4 ? 0xffffffffu : 0u) : value == 2 ? (w < 4 ? 0u : 0xffffffffu) : value == 3 ? 0x55555555u : 0xaaaaaaaau;
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipStreamDestroy(p->stream));
    p->stream = nullptr;
    HIPCHK(hipExtStreamCreateWithCUMask(&p->stream, 8, mask));
  } else if (k == "big_pre_wgs") {           // long-frame plans: empty workgroups ahead of every column pass (XCD phase)
    if (value < 0 || value > 64) return fail(TDSA_ERR_ARG, "big_pre_wgs=%d outside [0, 64]", value);
    p->big_pre_wgs = value;
#endif
  } else {
    return fail(TDSA_ERR_ARG, "unknown knob '%s'", name);
  }
  return TDSA_OK;
}

// developer hook (developer section of include/tdsa_hip.h): phase timeline of workgroup 0, TDSA_TIMELINE builds
int tdsa_debug_timeline(tdsa_plan p, unsigned long long* host_out_2048) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  if (!p->d_dbg) {
    HIPCHK(p->d_dbg.alloc(2048));
    HIPCHK(hipMemset(p->d_dbg, 0, 2048 * sizeof(unsigned long long)));
  }
  if (host_out_2048) {
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(host_out_2048, p->d_dbg, 2048 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  return TDSA_OK;
}

int tdsa_profile_enable(tdsa_plan p, int enable) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  p->profiling = enable != 0;
  return TDSA_OK;
}

int tdsa_profile_read(tdsa_plan p, int* launches, float* total_ms) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipStreamSynchronize(p->stream));
  float total = 0.f;
  for (size_t i = 0; i + 1 < p->prof_used; i += 2) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p->prof_events[i], p->prof_events[i + 1]));
    total += ms;
  }
  if (launches) *launches = int(p->prof_used / 2);
  if (total_ms) *total_ms = total;
  p->prof_used = 0;
  return TDSA_OK;
}

int tdsa_timer_begin(tdsa_plan p) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  return TDSA_OK;
}
int tdsa_timer_end(tdsa_plan p, float* elapsed_ms) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipEventSynchronize(p->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  if (elapsed_ms) *elapsed_ms = ms;
  return TDSA_OK;
}

}  // extern "C"
