// tdsa_capi_big.cpp - long-frame plans, N = 2^15 .. 2^20 = N1 x 16384: the host side of tdsa_big.hip.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

namespace tdsa {

// Long-frame plans.  Modes (decided by the plan's averaging settings):
//   * "lin" with avg_n >= frames seen so far + n_frames: Welch - the K segments of the call (and of earlier
//     calls since the last reset) are averaged, out_db_dev receives ONE row, the dB of the running mean;
//   * otherwise one frame per call (n_frames == 1): plain dB, or TraceAverager exp / capped lin on the
//     float64 state exactly as for the LDS-resident sizes.
// TraceAverager._buffer of a long-frame plan after Welch calls: the gather leaves the float64 SUM of the segments and the
// dB row; the mean itself (8 N bytes more per capture) is only formed for whoever reads the state - tdsa_get_avg,
// tdsa_welch_export, or the capped running mean that takes over once avg_n frames have been seen.
int big_materialize_mean(tdsa_plan p) {
  if (p->big_mean_in_sum && p->avg_count > 0)
    HIPCHK(launch_big_finish(p->d_sum, (long long)p->nfft, p->d_avg, p->avg_count, TDSA_DB_POW, 1.0f, 1.0f, 0.0f, nullptr,
                             nullptr, nullptr, nullptr, 0, 0, p->stream));
  p->big_mean_in_sum = false;
  return TDSA_OK;
}

int process_big(tdsa_plan p, int in_format, const void* iq_dev, int hop, int n_frames, float* out_db_dev) {
  const tdsa_mode& m = p->mode;
  const bool averaging = avg_active(m);
  const bool welch = averaging && m.avg_mode == TDSA_AVG_LIN && (long long)p->avg_count + n_frames <= m.avg_n;
  if (!welch && n_frames != 1)
    return fail(TDSA_ERR_ARG, "a %d-point plan takes one frame per call unless it is Welch-averaging "
                "(avg lin with avg_n >= total frames: count %d + %d > %d)", p->nfft, p->avg_count, n_frames,
                averaging ? m.avg_n : 0);
  const size_t N = size_t(p->nfft);
  const int n1 = p->nfft >> 14;
  const int group = n_frames < p->big_group ? n_frames : p->big_group;
  if (!p->d_z) HIPCHK(p->d_z.alloc(size_t(p->max_frames < p->big_group ? p->max_frames : p->big_group) * N));
  const int in_c64 = in_format == TDSA_IN_C64;
  const auto [xor_mask, in_off, in_scale] = in_format_consts(in_format);
  const long long stride = (long long)hop * bytes_per_sample(in_format);
  const float2* dc_sub = nullptr;
  if (m.dc_alpha >= 0.0f) {   // per-segment mean (alpha = 1) or tracker (alpha < 1)
    if (!p->d_sums64) HIPCHK(p->d_sums64.alloc(size_t(p->max_frames) * 2));
    HIPCHK(launch_big_dc(iq_dev, in_c64, xor_mask, stride, p->nfft, n_frames, m.dc_alpha > 1.0f ? 1.0 : double(m.dc_alpha),
                         double(in_off), double(in_scale), p->d_sums64, p->d_dc_state, p->d_dc_sub, p->stream));
    dc_sub = p->d_dc_sub;
  }
  // column pass and row pass alternate over rounds of segments.  The row pass leaves per-workgroup partial power
  // sums in d_acc (P[k1 * split + j][k2]): the first round of a call overwrites its rows, later rounds add to them,
  // the gather sums over j - nothing is carried from call to call, so a failed call leaves no residue
  const int split_max = p->num_cu / n1 > 1 ? p->num_cu / n1 : 1;
  int split_layout = 1;
  bool fused_tail = false;
  for (int s0 = 0; s0 < n_frames; s0 += group) {
    const int ns = n_frames - s0 < group ? n_frames - s0 : group;
    const int act = ns < split_max ? ns : split_max;
    if (s0 == 0) split_layout = act;
#ifdef TDSA_DEV
    if (p->big_pre_wgs > 0) HIPCHK(launch_xcd_shift(p->big_pre_wgs, p->stream));
#endif
    HIPCHK(launch_big_cols(p->log2n, static_cast<const unsigned char*>(iq_dev) + (long long)s0 * stride, in_c64, stride, ns,
                           p->big_win[in_format], p->d_tw_seed, dc_sub ? dc_sub + s0 : nullptr, p->d_z,
                           xor_mask, in_off, p->stream));
    if (p->profiling) {
      if (p->prof_used + 2 > p->prof_events.size()) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        p->prof_events.push_back(a);
        p->prof_events.push_back(b);
      }
      HIPCHK(hipEventRecord(p->prof_events[p->prof_used], p->stream));
    }
    fused_tail = welch && p->big_fuse_gather && !p->profiling && n_frames <= group;
    if (fused_tail) {
      if (!p->d_bigq) {
        HIPCHK(p->d_bigq.alloc(32));
        HIPCHK(hipMemsetAsync(p->d_bigq, 0, 32, p->stream));
        p->bigq_tickets = p->bigq_rows = 0;
      }
      unsigned long long used = 0;
      p->bigq_rows += (unsigned long long)n1 * act;
      HIPCHK(launch_big_rows_gather(p->log2n, p->d_z, (long long)N * sizeof(float2), ns, n1, act, p->d_acc, p->d_tw_row, p->d_sum,
                                    p->avg_count > 0, nullptr, p->avg_count + n_frames, m.db_mode,
                                    m.db_mode == TDSA_DB_POW ? m.power_scale : 1.0f, m.log_floor, m.cal_offset_db,
                                    p->tare_active ? p->d_tare_base : nullptr, out_db_dev,
                                    (m.hold_flags & TDSA_HOLD_MAX) ? p->d_hold_max : nullptr,
                                    (m.hold_flags & TDSA_HOLD_MIN) ? p->d_hold_min : nullptr, p->held_max == 0, p->held_min == 0,
                                    p->d_bigq, p->bigq_tickets, p->bigq_rows, &used, p->big_fuse_gather >> 1, p->stream));
      p->bigq_tickets += used;
      break;
    }
    HIPCHK(launch_big_rows(p->d_z, (long long)N * sizeof(float2), ns, n1, act, p->d_acc, split_layout, s0 > 0, p->d_tw_row,
                                p->stream));
    if (p->profiling) {
      HIPCHK(hipEventRecord(p->prof_events[p->prof_used + 1], p->stream));
      p->prof_used += 2;
    }
  }
  const bool hmax = (m.hold_flags & TDSA_HOLD_MAX) != 0, hmin = (m.hold_flags & TDSA_HOLD_MIN) != 0;
  const float pscale = m.db_mode == TDSA_DB_POW ? m.power_scale : 1.0f;
  float* const tare = p->tare_active ? p->d_tare_base : nullptr;
  float* const hold_max = hmax ? p->d_hold_max : nullptr;
  float* const hold_min = hmin ? p->d_hold_min : nullptr;
  if (welch && fused_tail) {
    p->avg_count += n_frames;
    p->big_mean_in_sum = true;
  } else if (welch) {
    HIPCHK(launch_big_gather_finish(p->log2n, p->d_acc, split_layout, p->d_sum, p->avg_count > 0, nullptr, p->avg_count + n_frames,
                                    m.db_mode, pscale, m.log_floor, m.cal_offset_db, tare, out_db_dev, hold_max, hold_min,
                                    p->held_max == 0, p->held_min == 0, p->stream));
    p->avg_count += n_frames;
    p->big_mean_in_sum = true;
  } else if (averaging) {    // TraceAverager exp / capped lin, one frame (signal_processing.py:35-61)
    TRY(big_materialize_mean(p));
    HIPCHK(launch_big_gather(p->log2n, p->d_acc, split_layout, p->d_lin64, 0, p->stream));
    HIPCHK(launch_avg_host_frame(p->d_lin64, p->nfft, p->d_avg, p->avg_count, m.avg_mode, m.avg_n, p->stream));
    avg_advance(p, 1);
    HIPCHK(launch_big_finish(p->d_avg, (long long)N, nullptr, 1, m.db_mode, pscale, m.log_floor, m.cal_offset_db, tare,
                             out_db_dev, hold_max, hold_min, p->held_max == 0, p->held_min == 0, p->stream));
  } else {
    HIPCHK(launch_big_gather_finish(p->log2n, p->d_acc, split_layout, p->d_lin64, 0, nullptr, 1, m.db_mode, pscale, m.log_floor,
                                    m.cal_offset_db, tare, out_db_dev, hold_max, hold_min, p->held_max == 0,
                                    p->held_min == 0, p->stream));
  }
  if (hmax) p->held_max += 1;
  if (hmin) p->held_min += 1;
  p->frames_seen += n_frames;
  return TDSA_OK;
}

}  // namespace tdsa
