// tdsa_capi_process.cpp - the processing entry points of a plan: device calls, batches, the synchronous host calls and
// the real-input path; the averager set-up and the per-frame statistics plumbing they share.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

// stream for the next frame-kernel launch of an order-independent call
static int pick_stream(tdsa_plan p, hipStream_t* out) {
  *out = p->stream;
  if (p->n_overlap <= 1) return TDSA_OK;
  const int k = p->rr++ % p->n_overlap;
  if (k == 0) return TDSA_OK;
  if (p->state_dirty) {   // state set up on the main stream (window, fills, tare ...) must be visible
    HIPCHK(hipEventRecord(p->ev_state, p->stream));
    for (int i = 0; i < p->n_overlap - 1; ++i) HIPCHK(hipStreamWaitEvent(p->aux[i], p->ev_state, 0));
    p->state_dirty = false;
  }
  *out = p->aux[k - 1];
  p->aux_busy = true;
  return TDSA_OK;
}

// ---- per-frame scalars of a call (tdsa_set_frame_stats) -------------------------------------------------------------
// The frame kernel's STATS instantiations exist for frames of whole waves (N >= 1024), dB rows without tare, hold none / max.
static bool frame_stats_fusable(tdsa_plan p, bool averaging) {
  return p->fs_on && !averaging && !p->chirp && !p->big && p->log2n >= 10 && !p->tare_active &&
         (p->mode.hold_flags & TDSA_HOLD_MIN) == 0;
}
// the slot the call at hand writes (the next one of its stream's), grown to n_frames
static int frame_stats_begin(tdsa_plan p, int n_frames, hipStream_t s, tdsa_plan_s::FsSlot** out) {
  int si = 0;
  for (int i = 0; i < tdsa_plan_s::kMaxOverlap - 1; ++i)
    if (s == p->aux[i] && s != p->stream) si = i + 1;
  tdsa_plan_s::FsSlot& sl = p->fs[si][p->fs_count[si]++ % tdsa_plan_s::kFsKeep];
  if (size_t(n_frames) > sl.d_peak.cap()) {
    HIPCHK(hipStreamSynchronize(s));                         // whatever last wrote the slot ran on this stream
    if (p->fs_stream) HIPCHK(hipStreamSynchronize(p->fs_stream));
    const size_t cap = size_t(n_frames) > size_t(p->max_frames) ? size_t(n_frames) : size_t(p->max_frames);
    TRY(sl.d_part.grow(cap * 16 * kStatsRecBytes, nullptr));   // up to 16 waves per frame
    TRY(sl.d_peak.grow(cap, nullptr));
    TRY(sl.d_bin.grow(cap, nullptr));
    TRY(sl.d_band.grow(cap, nullptr));
  }
  sl.n_frames = n_frames;
  sl.state = 0;
  sl.pending = false;
  sl.stream = s;
  *out = &sl;
  return TDSA_OK;
}
static int frame_stats_end(tdsa_plan p, tdsa_plan_s::FsSlot* sl, int state) {
  sl->state = state;
  p->fs_hist[p->fs_seq++ % tdsa_plan_s::kFsKeep] = sl;
  return TDSA_OK;
}
// plans / modes without the fused epilogue: the same scalars from the rows the call wrote (rows_stats_kernel)
static int frame_stats_from_rows(tdsa_plan p, const float* rows, int n_frames, int n_seg, int frames_per_seg,
                                 long long seg_stride_elems, hipStream_t s) {
  if (!p->fs_on) return TDSA_OK;
  tdsa_plan_s::FsSlot* sl = nullptr;
  TRY(frame_stats_begin(p, n_frames, s, &sl));
  if (rows == nullptr) return frame_stats_end(p, sl, 2);
  for (int g = 0; g < n_seg; ++g)
    HIPCHK(launch_rows_stats(rows + (long long)g * seg_stride_elems, frames_per_seg, p->nfft, p->fs_lo, p->fs_hi, -1.0,
                             sl->d_peak + (size_t)g * frames_per_seg, sl->d_bin + (size_t)g * frames_per_seg,
                             sl->d_band + (size_t)g * frames_per_seg, s));
  return frame_stats_end(p, sl, 1);
}

// The n_frames / hop / n_samples / window checks of the processing entry points.  frames_each: the frames n_samples has
// to hold (one capture's); the texts are each entry point's own: with_tail - the n_samples text names the frames,
// need_window - the window is checked here (the host entry points leave that to the device call they make).
static int check_frames(tdsa_plan p, size_t n_samples, int hop, int n_frames, int frames_each, bool with_tail, bool need_window) {
  if (n_frames < 0 || frames_each > p->max_frames)
    return fail(TDSA_ERR_ARG, "n_frames=%d outside [0, max_frames=%d]", frames_each, p->max_frames);
  if (hop < 1) return fail(TDSA_ERR_ARG, "hop=%d must be >= 1", hop);
  if (n_samples < size_t(frames_each - 1) * size_t(hop) + size_t(p->nfft)) {
    if (!with_tail) return fail(TDSA_ERR_ARG, "n_samples=%zu too small", n_samples);
    return fail(TDSA_ERR_ARG, "n_samples=%zu too small for %d frames of %d at hop %d", n_samples, frames_each,
                p->nfft, hop);
  }
  if (need_window && !p->window_set) return fail(TDSA_ERR_STATE, "tdsa_set_window has not been called");
  return TDSA_OK;
}

// [chunks][N] carries of the averager's chained scan; work in flight may still read the old ones
static int grow_carry(tdsa_plan p, size_t need_chunks) {
  return p->d_carry.grow(need_chunks * size_t(p->nfft), p->d_carry ? p->stream : nullptr);
}

namespace tdsa {

int launch_spectrum_profiled(tdsa_plan p, int in_c64, const SpecParams& sp, const LaunchGeom& g, hipStream_t s) {
  if (!p->profiling) {
    HIPCHK(launch_spectrum(p->log2n, in_c64, sp, g, s ? s : p->stream));
    return TDSA_OK;
  }
  if (p->prof_used + 2 > p->prof_events.size()) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    p->prof_events.push_back(a);
    p->prof_events.push_back(b);
  }
  HIPCHK(hipEventRecord(p->prof_events[p->prof_used], p->stream));
  HIPCHK(launch_spectrum(p->log2n, in_c64, sp, g, p->stream));
  HIPCHK(hipEventRecord(p->prof_events[p->prof_used + 1], p->stream));
  p->prof_used += 2;
  return TDSA_OK;
}

// the averager scan's parameters every path fills the same way (tare and the hold traces: the caller's)
AvgParams avg_params(tdsa_plan p, const float* lin, int n_frames, int n, float* out_db) {
  const tdsa_mode& m = p->mode;
  AvgParams ap{};
  ap.lin = lin;
  ap.n_frames = n_frames;
  ap.n = n;
  ap.state = p->d_avg;
  ap.count_in = p->avg_count;
  ap.mode = m.avg_mode;
  ap.avg_n = m.avg_n;
  ap.log_floor = m.log_floor;
  ap.cal_db = m.cal_offset_db;
  ap.out_db = out_db;
  return ap;
}

// TraceAverager's count after n_frames more frames (signal_processing.py:35-61): lin counts up to its cap, exp stays at 1
void avg_advance(tdsa_plan p, int n_frames) {
  if (p->mode.avg_mode == TDSA_AVG_LIN) {
    const long long c = (long long)p->avg_count + n_frames;
    p->avg_count = int(c < p->mode.avg_n ? c : p->mode.avg_n);
  } else {
    p->avg_count = 1;
  }
}

// The chunk aggregates of the chained scan: their buffers (first use; agg_rows: rows of a native plan's largest grid) and
// the frames' weights, made again only when what they depend on has changed.  ap.wg_chunks is the caller's; path 0: the
// chunks are the frame kernel's workgroup ranges (fpu frames per unit), path 1: equal ranges of the batch.
static int avg_chunk_setup(tdsa_plan p, AvgParams& ap, size_t agg_rows, int fpu, int path, hipStream_t s) {
  if (!p->d_agg) HIPCHK(p->d_agg.alloc((agg_rows > 256 ? agg_rows : size_t(256)) * p->nfft));
  if (!p->d_agg_w) HIPCHK(p->d_agg_w.alloc(size_t(p->max_frames)));
  if (!p->d_chunk_a) HIPCHK(p->d_chunk_a.alloc(size_t(kAvgMaxWgChunks + 64)));
  if (!p->d_chunk_v) HIPCHK(p->d_chunk_v.alloc(size_t(kAvgMaxWgChunks + 64)));
  ap.chunk_a = p->d_chunk_a;
  ap.chunk_v = p->d_chunk_v;
  ap.agg = p->d_agg;
  if (path == 1) ap.agg_w_local = p->d_agg_w;
  // the weights depend on where the averager stands and on the chunking only: in steady state (exp mode, or lin
  // with its count at the cap) consecutive calls of one shape re-use them
  const long long key[7] = {p->avg_count, ap.mode, ap.avg_n, ap.n_frames, ap.wg_chunks, fpu, path};
  if (std::memcmp(key, p->agg_w_key, sizeof(key)) != 0) {
    HIPCHK(launch_avg_weights(ap, p->d_agg_w, p->d_chunk_a, p->d_chunk_v, s));
    std::memcpy(p->agg_w_key, key, sizeof(key));
  }
  return TDSA_OK;
}

// Long averaged batches of the sizes whose frame kernel cannot form the scan's chunk aggregates itself (several frames per
// workgroup slot below 4096 points; chirp-z plans): the chunks become up to 256 equal ranges of the batch, a pass of the
// scan's own forms their float32 aggregates (avg_agg_local_kernel) and the two-level chain of the workgroup-chunk path
// takes it from there.  With fixed chunks of 64 frames one thread per bin walked hundreds of chunks in order: 75 of the
// 169 us of a 19 531-frame batch at N = 1024.  Short batches keep the 64-frame chunks.
int avg_use_ranges(tdsa_plan p, AvgParams& ap, int n_frames, hipStream_t s) {
  if (p->avg_f64_chunks || n_frames <= 1024 || p->d_carry == nullptr) return TDSA_OK;
  const int ranges = (n_frames + 63) / 64 < 256 ? (n_frames + 63) / 64 : 256;
  if (size_t(ranges) > p->d_carry.cap() / size_t(p->nfft)) return TDSA_OK;
  // a range's aggregate is a float32 sum: kept to the ~160 frames the workgroup-chunk path allows itself; longer
  // ranges (batches of more than 40 960 frames here) take the 64-frame chunks with their float64 aggregates - the
  // reference's TraceAverager is float64 throughout (utils/signal_processing.py:48)
  if ((n_frames + ranges - 1) / ranges > 160) return TDSA_OK;
  // (rows of nfft floats - those of the real-input path are shorter: nfft / 2 + 1.  A native plan may also take the
  // workgroup-chunk path on another call: one row per workgroup of its grid)
  const size_t grid_rows = (p->chirp || p->big) ? 0 : size_t(spectrum_geometry(p->log2n, p->max_frames, p->num_cu).grid);
  ap.wg_chunks = ranges;
  ap.wg_fold = 1;
  return avg_chunk_setup(p, ap, grid_rows, 1, 1, s);
}

// several captures in one launch (tdsa_process_dev_batch): n_frames = n_seg * frames_per_seg frames in all
struct SegInfo {
  int n_seg = 1;
  int frames_per_seg = 0;
  long long in_stride_bytes = 0;
  long long out_stride_elems = 0;
  bool single_frames = false;   // one frame per capture: launched as ONE capture whose frames are in_stride_bytes apart
};

// before / after: optional events the device work waits for / signals (tdsa_pipe: H2D and D2H legs)
int process_dev_impl(tdsa_plan p, int in_format, const void* iq_dev, size_t n_samples, int hop, int n_frames,
                     float* out_db_dev, hipEvent_t before, hipEvent_t after, const SegInfo* seg) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (in_format < TDSA_IN_I8 || in_format > TDSA_IN_C64) return fail(TDSA_ERR_ARG, "in_format %d", in_format);
  if (n_frames == 0) return TDSA_OK;
  if (!iq_dev) return fail(TDSA_ERR_ARG, "iq pointer is null");
  const int frames_each = seg ? seg->frames_per_seg : n_frames;     // frames of ONE capture (n_samples is per capture)
  TRY(check_frames(p, n_samples, hop, n_frames, frames_each, true, true));
  const int bps = bytes_per_sample(in_format);
  if ((reinterpret_cast<uintptr_t>(iq_dev) % (bps == 8 ? 8 : 2)) != 0)
    return fail(TDSA_ERR_ARG, "iq pointer must be aligned to one sample (%d bytes)", bps);
  HIPCHK(hipSetDevice(p->device));
  if (p->chirp) {
    JOIN(p);
    if (before) HIPCHK(hipStreamWaitEvent(p->stream, before, 0));
    int rc_chirp = process_chirp(p, in_format, iq_dev, hop, n_frames, out_db_dev);
    if (rc_chirp == TDSA_OK) rc_chirp = frame_stats_from_rows(p, out_db_dev, n_frames, 1, n_frames, 0, p->stream);
    if (rc_chirp == TDSA_OK && after) HIPCHK(hipEventRecord(after, p->stream));
    return rc_chirp;
  }
  if (p->big) {
    JOIN(p);
    if (before) HIPCHK(hipStreamWaitEvent(p->stream, before, 0));
    const int rc_big = process_big(p, in_format, iq_dev, hop, n_frames, out_db_dev);
    if (rc_big == TDSA_OK && after) HIPCHK(hipEventRecord(after, p->stream));
    return rc_big;
  }

  const tdsa_mode& m = p->mode;
  const bool averaging = avg_active(m);
  // calls whose result does not depend on the order they execute in may overlap (tdsa_set_overlap)
  const bool order_free = !averaging && (m.dc_alpha < 0.0f || m.dc_alpha >= 1.0f);
  if (seg && !order_free) return fail(TDSA_ERR_STATE, "internal: a batched launch needs an order-free mode");
  hipStream_t s = p->stream;
  // synchronous host entry points (process_host) wait for this very launch: nothing runs beside it, so it keeps
  // the main stream and the whole chip (a half-chip launch there only lost throughput)
  const bool overlap = order_free && !p->sync_call && !p->profiling;   // (profiled launches: main stream, events around)
  if (overlap) {
    TRY(pick_stream(p, &s));
  } else {
    JOIN(p);
  }
  if (before) HIPCHK(hipStreamWaitEvent(s, before, 0));
  const bool hold = (m.hold_flags & 3u) != 0;
  const int in_c64 = in_format == TDSA_IN_C64;

  SpecParams sp{};
  sp.in = iq_dev;
  sp.frame_stride = (long long)hop * bps;
  sp.n_frames = n_frames;
  sp.first_frame_index = p->frames_seen > 0 ? 1 : 0;
  sp.window = p->d_window[in_format];
  sp.window_perm = p->d_window_perm[in_format];
  sp.tw = p->d_tw;
  const InFormat inf = in_format_consts(in_format);
  sp.xor_mask = inf.xor_mask;
  sp.in_off = inf.off;
  sp.in_scale = inf.scale;
  sp.db_mode = m.db_mode;
  sp.pscale = m.db_mode == TDSA_DB_POW ? m.power_scale : 1.0f;
  sp.log_floor = m.log_floor;
  sp.cal_db = m.cal_offset_db;
  sp.tare = p->tare_active ? p->d_tare_base : nullptr;
  sp.dbg = p->d_dbg;
  if (seg && seg->single_frames) {
    sp.frame_stride = seg->in_stride_bytes;      // seg_magic stays 0: frame f reads in + f * stride, row f follows row f - 1
  } else if (seg) {
    sp.seg_frames = unsigned(seg->frames_per_seg);
    sp.seg_magic = unsigned((0x100000000ull + sp.seg_frames - 1) / sp.seg_frames);   // ceil(2^32 / d)
    sp.seg_in_stride = seg->in_stride_bytes;
    sp.seg_out_stride = seg->out_stride_elems;
  }

  if (m.dc_alpha < 0.0f) {
    sp.dc_mode = DC_NONE;
  } else if (m.dc_alpha >= 1.0f) {
    sp.dc_mode = DC_FRAME_MEAN;
    sp.dc_state = p->d_dc_state;
  } else {
    sp.dc_mode = DC_TRACKED;
    // overlapping byte frames (the hop divides the frame): the sums of the hop-long blocks are formed once and a frame's
    // sum is `parts` of them - integer-valued floats, exact in any order - instead of every sample being summed parts times
    const int parts = (!in_c64 && hop >= 64 && hop % 4 == 0 && p->nfft % hop == 0 && p->nfft / hop >= 2 && p->nfft / hop <= 8)
                          ? p->nfft / hop : 1;
    HIPCHK(launch_frame_sums(iq_dev, in_c64, sp.xor_mask, sp.frame_stride, parts > 1 ? hop : p->nfft,
                             parts > 1 ? n_frames + parts - 1 : n_frames, p->d_sums, p->stream));
    HIPCHK(launch_dc_track(p->d_sums, p->nfft, n_frames, m.dc_alpha, sp.in_off, sp.in_scale, p->d_dc_state,
                           p->d_dc_sub, p->stream, parts));
    sp.dc_sub = p->d_dc_sub;
  }

  // With three or more streams the overlapped launches are sized for HALF the CUs: two of them run side by side, the
  // next one queues behind whichever ends first.  Each workgroup then carries twice the frames - its fixed costs (cold
  // first fetch, hold merge: ~5 us) count half - and the ragged end of one launch is filled by the next:
  // C3 76.4 -> 74.3 us per step, C2 26.7 -> 26.0 (profiles/r02_c3_experiments.txt).  More than three streams in flight
  // measured worse (4: 91 us), and strictly serial launches keep the whole chip.
  const LaunchGeom g = spectrum_geometry(p->log2n, n_frames,
                                         (overlap && p->n_overlap >= 3) ? (p->num_cu * p->overlap_share + 99) / 100 : p->num_cu);
  if (averaging) {
    if (!p->d_lin) HIPCHK(p->d_lin.alloc(size_t(p->max_frames) * p->nfft));
    // Long batches run as a chained scan over chunks of frames (tdsa_trace.hip).  The chunks ARE the frame ranges of the
    // frame kernel's workgroups, which form their chunk's aggregate themselves while the rows pass through their
    // registers - the scan's first pass over the rows disappears (below 4096 points a workgroup's slots take consecutive
    // runs of its range and add their partial sums through LDS).
    // Up to 256 chunks: grids of more workgroups (N = 8192: 512, N <= 4096: 1024) fold 2 / 4 consecutive ranges into one.
    const int wg_fold = (g.grid + 255) / 256;
    const int units = (n_frames + g.fpw - 1) / g.fpw;
    const bool wg_chunks = n_frames > p->avg_wg_min && g.grid <= kAvgMaxWgChunks &&
                           ((units + g.grid - 1) / g.grid) * g.fpw * wg_fold <= 160 && !p->avg_f64_chunks;
    const size_t agg_rows = size_t(spectrum_geometry(p->log2n, p->max_frames, p->num_cu).grid);
    const size_t need_chunks = wg_chunks ? (agg_rows < 256 ? agg_rows : size_t(256))
                                         : (p->max_frames > 128 ? size_t(avg_scan_chunks(p->max_frames)) : 0);
    TRY(grow_carry(p, need_chunks));
    AvgParams ap = avg_params(p, p->d_lin, n_frames, p->nfft, out_db_dev);
    ap.tare = sp.tare;
    ap.state_max = (m.hold_flags & TDSA_HOLD_MAX) ? p->d_hold_max : nullptr;
    ap.state_min = (m.hold_flags & TDSA_HOLD_MIN) ? p->d_hold_min : nullptr;
    if (wg_chunks) {
      ap.wg_chunks = g.grid;
      ap.wg_fold = wg_fold;
      ap.wg_fpw = g.fpw;
      TRY(avg_chunk_setup(p, ap, agg_rows, g.fpw, 0, p->stream));
      sp.agg_w = p->d_agg_w;
      sp.agg_out = p->d_agg;
      // only the averager's state is wanted (no dB rows, no hold: the averaged spectrum of a capture - Welch at a native
      // size): the linear rows are neither written nor re-scanned
      if (out_db_dev == nullptr && ap.state_max == nullptr && ap.state_min == nullptr) { sp.agg_only = 1; ap.state_only = 1; }
    } else {
      TRY(avg_use_ranges(p, ap, n_frames, p->stream));
    }
    sp.out_lin = p->d_lin;
    sp.hold_flags = 0;
    TRY(launch_spectrum_profiled(p, in_c64, sp, g));
    HIPCHK(launch_avg_scan(ap, p->stream, p->d_carry));
    TRY(frame_stats_from_rows(p, out_db_dev, n_frames, 1, n_frames, 0, p->stream));
    avg_advance(p, n_frames);
  } else {
    sp.out_db = out_db_dev;
    sp.hold_flags = int(m.hold_flags & 3u);
    if (hold) {   // workgroups merge their register-resident traces into the plan's traces with atomics
      sp.part_max = p->d_hold_max;
      sp.part_min = p->d_hold_min;
    }
    tdsa_plan_s::FsSlot* fsl = nullptr;
    const bool fs_fused = frame_stats_fusable(p, false);
    if (fs_fused) {
      TRY(frame_stats_begin(p, n_frames, s, &fsl));
      sp.stats_part = fsl->d_part;
      sp.band_lohi = p->fs_lo <= p->fs_hi ? (unsigned(p->fs_lo) | (unsigned(p->fs_hi) << 16)) : 1u;
    }
    TRY(launch_spectrum_profiled(p, in_c64, sp, g, s));
    if (fs_fused) {
      // the records hold the power before the calibration offset: 10^(dB / 10) = power x 10^(cal / 10).  They are folded
      // when someone asks (tdsa_get_frame_stats): nothing runs behind the frame kernel on its stream
      fsl->pending = true;
      fsl->wpf = spectrum_waves_per_frame(p->log2n);
      fsl->cal_lin = std::pow(10.0, double(m.cal_offset_db) / 10.0);
      TRY(frame_stats_end(p, fsl, 1));
    } else if (p->fs_on) {
      const bool one = !seg || seg->single_frames;
      TRY(frame_stats_from_rows(p, out_db_dev, n_frames, one ? 1 : seg->n_seg, one ? n_frames : seg->frames_per_seg,
                                one ? 0 : seg->out_stride_elems, s));
    }
  }
  if (after) HIPCHK(hipEventRecord(after, s));
  if (m.hold_flags & TDSA_HOLD_MAX) p->held_max += n_frames;
  if (m.hold_flags & TDSA_HOLD_MIN) p->held_min += n_frames;
  p->frames_seen += n_frames;
  return TDSA_OK;
}

// pinned, device-visible bounce buffers of the host entry points (grown on demand; every host call ends with a
// synchronize, so they are free when the next one starts)
int ensure_pins(tdsa_plan p, size_t in_bytes, size_t out_bytes) {
  TRY(p->h_in_pin.grow(in_bytes, p->h_in_pin ? p->stream : nullptr));
  TRY(p->h_out_pin.grow(out_bytes, p->h_out_pin ? p->stream : nullptr));
  return TDSA_OK;
}

}  // namespace tdsa

extern "C" {

int tdsa_process_dev(tdsa_plan p, int in_format, const void* iq_dev, size_t n_samples, int hop, int n_frames,
                     float* out_db_dev) {
  return process_dev_impl(p, in_format, iq_dev, n_samples, hop, n_frames, out_db_dev, nullptr, nullptr);
}

// n_segments captures of one shape.  Where the plan's mode makes the captures independent of the order they are
// processed in (no averaging, no tracked DC remover) and the frames are LDS resident, ALL of them go out as ONE
// persistent launch: the per-launch costs (cold first fetch of window / twiddles, hold merge, the ragged last round
// of frames over the CUs) are paid once per call instead of once per capture.  Every other mode runs the captures
// one after the other through the same code as tdsa_process_dev - the results are the same either way.
int tdsa_process_dev_batch(tdsa_plan p, int in_format, const void* iq_dev, size_t seg_stride_bytes, int n_segments,
                           size_t n_samples_per_seg, int hop, int frames_per_seg, float* out_db_dev,
                           size_t out_seg_stride_floats) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_segments < 0) return fail(TDSA_ERR_ARG, "n_segments=%d", n_segments);
  if (n_segments == 0 || frames_per_seg == 0) return TDSA_OK;
  if (in_format < TDSA_IN_I8 || in_format > TDSA_IN_C64) return fail(TDSA_ERR_ARG, "in_format %d", in_format);
  const size_t bps = size_t(bytes_per_sample(in_format));
  if (n_segments > 1 && seg_stride_bytes % (bps == 8 ? 8 : 2) != 0)
    return fail(TDSA_ERR_ARG, "seg_stride_bytes=%zu must be a multiple of one sample", seg_stride_bytes);
  if (frames_per_seg < 0) return fail(TDSA_ERR_ARG, "frames_per_seg=%d", frames_per_seg);
  if (out_seg_stride_floats == 0) out_seg_stride_floats = size_t(frames_per_seg) * size_t(p->nfft);   // captures back to back
  // the captures' rows must not overlap: with a stride below one capture's rows the one-launch path would have
  // several workgroups write the same rows concurrently (which capture survives would not be deterministic)
  if (n_segments > 1 && out_db_dev != nullptr && !p->big &&
      out_seg_stride_floats < size_t(frames_per_seg) * size_t(p->nfft))
    return fail(TDSA_ERR_ARG, "out_seg_stride_floats=%zu is smaller than one capture's rows (%d x %d)",
                out_seg_stride_floats, frames_per_seg, p->nfft);
  const tdsa_mode& m = p->mode;
  const bool order_free = !avg_active(m) && (m.dc_alpha < 0.0f || m.dc_alpha >= 1.0f);
  const long long total = (long long)n_segments * frames_per_seg;
  // frames_per_seg == 1: ceil(2^32 / 1) does not fit SpecParams::seg_magic (it would read as 0 = "one capture").
  // One frame per capture IS one capture whose frames sit seg_stride apart, as long as its rows are contiguous;
  // with gapped rows the captures go out one by one.
  const bool single_frames = frames_per_seg == 1;
  const bool rows_contiguous = out_db_dev == nullptr || out_seg_stride_floats == size_t(p->nfft);
  const bool one_launch = n_segments > 1 && order_free && !p->chirp && !p->big && frames_per_seg > 0 &&
                          total * frames_per_seg < 0x100000000ll && total < 0x7fffffffll &&
                          (!single_frames || rows_contiguous);
  if (!one_launch) {
    for (int sg = 0; sg < n_segments; ++sg) {
      TRY(process_dev_impl(p, in_format, static_cast<const unsigned char*>(iq_dev) + size_t(sg) * seg_stride_bytes,
                           n_samples_per_seg, hop, frames_per_seg,
                           out_db_dev ? out_db_dev + size_t(sg) * out_seg_stride_floats : nullptr, nullptr, nullptr));
    }
    return TDSA_OK;
  }
  SegInfo seg;
  seg.n_seg = n_segments;
  seg.frames_per_seg = frames_per_seg;
  seg.in_stride_bytes = (long long)seg_stride_bytes;
  seg.out_stride_elems = (long long)out_seg_stride_floats;
  seg.single_frames = single_frames;
  return process_dev_impl(p, in_format, iq_dev, n_samples_per_seg, hop, int(total), out_db_dev, nullptr, nullptr, &seg);
}

static int process_host(tdsa_plan p, int fmt, const void* iq_host, size_t n_samples, int hop, int n_frames,
                        float* out_db_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (n_frames == 0) return TDSA_OK;
  if (!iq_host) return fail(TDSA_ERR_ARG, "iq pointer is null");
  TRY(check_frames(p, n_samples, hop, n_frames, n_frames, true, false));
  const size_t need = size_t(n_frames - 1) * size_t(hop) + size_t(p->nfft);
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const size_t in_bytes = need * bytes_per_sample(fmt);
  TRY(p->d_in_stage.grow(in_bytes, p->stream));
  if (out_db_host && !p->d_out_stage)
    HIPCHK(p->d_out_stage.alloc(size_t(p->big ? 1 : p->max_frames) * p->nfft));
  const size_t out_bytes = out_db_host ? size_t(p->big ? 1 : n_frames) * p->nfft * sizeof(float) : 0;
  const bool bounce = in_bytes <= kPinnedBounceMax && out_bytes <= kPinnedBounceMax;
  if (bounce) {
    TRY(ensure_pins(p, in_bytes, out_bytes));
    std::memcpy(p->h_in_pin, iq_host, in_bytes);      // the previous call ended with a synchronize: the buffer is free
  }
  // the smallest calls (one displayed frame) skip the two DMA operations as well: the kernels read the samples from
  // and write the row to the pinned buffers directly over the bus (hipHostMalloc memory is device-visible)
  const bool direct = bounce && in_bytes + out_bytes <= kZeroCopyMax && !p->big;
  if (direct) {
    p->sync_call = true;
    int rc_d = tdsa_process_dev(p, fmt, p->h_in_pin, need, hop, n_frames,
                                out_db_host ? p->h_out_pin.as<float>() : nullptr);
    p->sync_call = false;
    TRY(rc_d);
    JOIN(p);
    HIPCHK(hipStreamSynchronize(p->stream));
    if (out_db_host) std::memcpy(out_db_host, p->h_out_pin, out_bytes);
    return TDSA_OK;
  }
  HIPCHK(hipMemcpyAsync(p->d_in_stage, bounce ? p->h_in_pin : iq_host, in_bytes, hipMemcpyHostToDevice, p->stream));
  p->sync_call = true;
  int rc = tdsa_process_dev(p, fmt, p->d_in_stage, need, hop, n_frames, out_db_host ? p->d_out_stage : nullptr);
  p->sync_call = false;
  TRY(rc);
  // with tdsa_set_overlap(n > 1) the frame kernel may have gone to an auxiliary stream: order the main
  // stream (read-back + the synchronize below) behind it, so the host call stays sequentially consistent
  JOIN(p);
  if (out_db_host)
    HIPCHK(hipMemcpyAsync(bounce ? p->h_out_pin : static_cast<void*>(out_db_host), p->d_out_stage, out_bytes,
                          hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  if (bounce && out_db_host) std::memcpy(out_db_host, p->h_out_pin, out_bytes);
  return TDSA_OK;
}

int tdsa_process_i8(tdsa_plan p, const int8_t* iq_host, size_t n_samples, int hop, int n_frames,
                    float* out_db_host) {
  return process_host(p, TDSA_IN_I8, iq_host, n_samples, hop, n_frames, out_db_host);
}
int tdsa_process_u8(tdsa_plan p, const uint8_t* iq_host, size_t n_samples, int hop, int n_frames,
                    float* out_db_host) {
  return process_host(p, TDSA_IN_U8, iq_host, n_samples, hop, n_frames, out_db_host);
}
int tdsa_process_c64(tdsa_plan p, const float* iq_host, size_t n_samples, int hop, int n_frames,
                     float* out_db_host) {
  return process_host(p, TDSA_IN_C64, iq_host, n_samples, hop, n_frames, out_db_host);
}

int tdsa_real_input_supported(int nfft) {
  if (nfft < 2) return 0;
  const bool pow2 = (nfft & (nfft - 1)) == 0;
  if (pow2) return nfft <= (1 << kMaxLog2N) ? 1 : 0;        // the native long-frame plans have no real-input path
  return nfft <= (1 << 19) ? 1 : 0;                          // chirp-z plans; above 2^19 they split the frame in two
}

int tdsa_process_real2(tdsa_plan p, const float* lr_host, size_t n_samples, int hop, int n_frames, int channel,
                       float* out_db_host) {
  if (!p) return fail(TDSA_ERR_ARG, "null plan");
  if (p->big) return fail(TDSA_ERR_ARG, "real-input path needs an FFT size of at most 16384");
  if (p->chirp_split)      // (before any allocation or launch: the call leaves the plan as it found it)
    return fail(TDSA_ERR_ARG, "real-input path: frames above 2^19 points that are not a power of two have no plan (nfft=%d)", p->nfft);
  if (channel < TDSA_CH_MONO || channel > TDSA_CH_STEREO) return fail(TDSA_ERR_ARG, "channel %d", channel);
  if (n_frames == 0) return TDSA_OK;
  if (!lr_host || !out_db_host) return fail(TDSA_ERR_ARG, "null buffer");
  TRY(check_frames(p, n_samples, hop, n_frames, n_frames, false, true));
  const size_t need = size_t(n_frames - 1) * size_t(hop) + size_t(p->nfft);
  const tdsa_mode& m = p->mode;
  if (m.db_mode != TDSA_DB_POW) return fail(TDSA_ERR_ARG, "real-input path computes power dB: set TDSA_DB_POW");
  if (avg_active(m) && channel == TDSA_CH_STEREO)
    return fail(TDSA_ERR_ARG, "stereo with averaging: process frame by frame (left is averaged, right is not)");
  HIPCHK(hipSetDevice(p->device));
  JOIN(p);
  const int n = p->nfft, nb = n / 2 + 1;
  const size_t in_bytes = need * sizeof(float2);
  TRY(p->d_in_stage.grow(in_bytes, p->stream));
  if (!p->d_cplx) HIPCHK(p->d_cplx.alloc(size_t(p->max_frames) * n));
  if (!p->d_lin1) HIPCHK(p->d_lin1.alloc(size_t(p->max_frames) * 2 * nb));
  if (!p->d_db1) HIPCHK(p->d_db1.alloc(size_t(p->max_frames) * 2 * nb));
  const int n_sig = channel == TDSA_CH_STEREO ? 2 : 1;
  TRY(p->d_real.grow(need * size_t(n_sig), p->stream));
  // one tick of audio is small: samples and dB rows go through pinned, device-visible buffers that the kernels read
  // and write in place (no DMA operation either way); larger batches are copied as before
  const int rows_out = channel == TDSA_CH_STEREO ? 2 * n_frames : n_frames;
  const size_t out_bytes = size_t(rows_out) * nb * sizeof(float);
  const bool direct = in_bytes <= kZeroCopyMax && out_bytes <= kZeroCopyMax;
  const float2* lr_dev = p->d_in_stage.as<const float2>();
  float* db_dst = p->d_db1;
  if (direct) {
    TRY(ensure_pins(p, in_bytes, out_bytes));
    std::memcpy(p->h_in_pin, lr_host, in_bytes);
    lr_dev = p->h_in_pin.as<const float2>();
    db_dst = p->h_out_pin.as<float>();
  } else {
    HIPCHK(hipMemcpyAsync(p->d_in_stage, lr_host, in_bytes, hipMemcpyHostToDevice, p->stream));
  }
  // one transform per real signal (no left / right packing: see real_select_kernel)
  float2* const za = p->d_real;
  float2* const zb = p->d_real + need;
  HIPCHK(launch_real_select(lr_dev, need, channel, za, zb, p->stream));
  for (int sig = 0; sig < n_sig; ++sig) {
    if (p->chirp) {
      // a size that is not a power of two: signal + 0i through the chirp-z core, mean removed (exact sums), and
      // the one-sided power straight from the full spectrum
      const float2* zin = sig == 0 ? za : zb;
      const long long stride = (long long)hop * sizeof(float2);
      if (chirp_sum_chunks(n) > 1 && !p->d_sums64)
        HIPCHK(p->d_sums64.alloc(size_t(p->max_frames) * chirp_sum_chunks(n) * 2));
      HIPCHK(launch_chirp_sums(zin, 1, 0u, stride, n, n_frames, 0, p->d_sums, nullptr, 1.0f, p->stream, p->d_sums64));
      TRY(chirp_transform(p, zin, TDSA_IN_C64, stride, n_frames, p->d_sums, 0u, 0.0f));
      HIPCHK(launch_chirp_post_real(p->d_u0, n, p->m_fft, n_frames, n_sig, sig, m.power_scale, p->d_lin1, p->stream));
      continue;
    }
    SpecParams sp{};
    sp.in = sig == 0 ? za : zb;
    sp.frame_stride = (long long)hop * sizeof(float2);
    sp.n_frames = n_frames;
    sp.first_frame_index = 1;
    sp.window = p->d_window[TDSA_IN_C64];
    sp.window_perm = p->d_window_perm[TDSA_IN_C64];
    sp.tw = p->d_tw;
    sp.out_cplx = p->d_cplx;
    sp.in_scale = 1.0f;
    sp.dc_mode = DC_FRAME_MEAN;                     // signal - signal.mean()  (audio_samples.py:123)
    sp.db_mode = TDSA_DB_POW;
    sp.pscale = 1.0f;
    const LaunchGeom g = spectrum_geometry(p->log2n, n_frames, p->num_cu);
    HIPCHK(launch_spectrum(p->log2n, 1, sp, g, p->stream));
    HIPCHK(launch_real_fold(p->d_cplx, n, n_frames, n_sig, sig, m.power_scale, p->d_lin1, p->stream));
  }
  const int rows = channel == TDSA_CH_STEREO ? 2 * n_frames : n_frames;
  if (avg_active(m)) {
    AvgParams ap = avg_params(p, p->d_lin1, n_frames, nb, db_dst);
    // long batches: the chunked scan of the complex path (one thread per bin walking 2000 frames took 284 us)
    if (n_frames > 128) {
      TRY(grow_carry(p, size_t(avg_scan_chunks(p->max_frames))));
      TRY(avg_use_ranges(p, ap, n_frames, p->stream));
    }
    HIPCHK(launch_avg_scan(ap, p->stream, n_frames > 128 ? p->d_carry : nullptr));
    avg_advance(p, n_frames);
  } else {
    HIPCHK(launch_lin_to_db(p->d_lin1, size_t(rows) * nb, m.log_floor, m.cal_offset_db, db_dst, p->stream));
  }
  if (!direct) HIPCHK(hipMemcpyAsync(out_db_host, p->d_db1, out_bytes, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  if (direct) std::memcpy(out_db_host, p->h_out_pin, out_bytes);
  return TDSA_OK;
}

}  // extern "C"
