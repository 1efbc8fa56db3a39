/*
 * tdsa_hip.h - C-ABI of libtdsa_hip.so, the MI355X (gfx950) IQ -> spectrum engine.
 *
 * This is the drop-in boundary for the reference's "sample method" hot path
 * (CWNE88/topdogspectrumanalyser).  The reference is pure Python and reaches native code only
 * through numpy.fft / scipy.fft; a maintainer binds this library with ctypes.
 * Every entry point names the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns int: 0 = TDSA_OK, negative = error; tdsa_last_error_string() gives text
 *   - no C++ exception and no torch/numpy type crosses this ABI: plain pointers and sizes only
 *   - the caller owns every host buffer; a plan owns its device buffers, HIP stream and events
 *   - one plan is used by one host thread at a time (the reference serialises the path under
 *     HackrfSamplesDataSource._lock, datasources/hackrf_samples.py:50,341)
 *   - "samples" always counts complex samples (one I,Q pair)
 *   - spectra are returned fftshift-ed (DC at index N/2) exactly as
 *     np.fft.fftshift(np.fft.fft(x)) orders them (datasources/hackrf_samples.py:370)
 */
#ifndef TDSA_HIP_H
#define TDSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDSA_OK 0
#define TDSA_ERR_ARG (-1)      /* bad argument (size, mode, null pointer) */
#define TDSA_ERR_HIP (-2)      /* a HIP runtime call failed               */
#define TDSA_ERR_STATE (-3)    /* call sequence error (no window set ...) */
#define TDSA_ERR_NOMEM (-4)

#define TDSA_VERSION 100

typedef struct tdsa_plan_s* tdsa_plan;

/* input sample formats (the unpack pyhackrf / pyrtlsdr do on the host) */
#define TDSA_IN_I8 0   /* interleaved int8  I,Q ; x = (I + jQ)/128          (HackRF / build contract) */
#define TDSA_IN_U8 1   /* interleaved uint8 I,Q ; x = (u/127.5 - 1) pairs   (pyrtlsdr convention)     */
#define TDSA_IN_C64 2  /* interleaved float32 re,im (numpy complex64)                               */

/* dB conversion (utils/constants.py:152-155 floors are passed in tdsa_mode.log_floor) */
#define TDSA_DB_MAG 0  /* 20*log10(|X| + floor)            datasources/hackrf_samples.py:382-383 */
#define TDSA_DB_POW 1  /* 10*log10(|X|^2 * scale + floor)  hackrf_samples.py:374-381, rtl_samples.py:175-184 */

/* trace averaging (utils/signal_processing.py:5-73) */
#define TDSA_AVG_OFF 0
#define TDSA_AVG_EXP 1
#define TDSA_AVG_LIN 2

/* hold_flags / reset bits */
#define TDSA_HOLD_MAX 1u
#define TDSA_HOLD_MIN 2u
#define TDSA_RESET_AVG 1u
#define TDSA_RESET_HOLD_MAX 2u
#define TDSA_RESET_HOLD_MIN 4u
#define TDSA_RESET_DC 8u
#define TDSA_RESET_TARE 16u
#define TDSA_RESET_ALL 31u

typedef struct tdsa_mode {
  int32_t db_mode;       /* TDSA_DB_MAG | TDSA_DB_POW                                                */
  float power_scale;     /* POW only: 1 or 1/(fs*N) for PSD (hackrf_samples.py:375, rtl_samples.py:177) */
  float log_floor;       /* 1e-12 (LOG_FLOOR) or 1e-10 (POWER_LOG_FLOOR)                               */
  int32_t avg_mode;      /* TDSA_AVG_*  ; a CHANGE of avg_mode / avg_n restarts the average (see below) */
  int32_t avg_n;         /* clamped to >= 1; n <= 1 means pass-through                                 */
  float dc_alpha;        /* < 0: no DC removal (RTL branch); 1: per-frame mean removal; (0,1): tracker
                            dc <- (1-a)*dc + a*mean(x)  (hackrf_samples.py:360-365, :32, :654-657)     */
  float cal_offset_db;   /* added to every dB value (core/display_data_processor.py:317-327)           */
  uint32_t hold_flags;   /* TDSA_HOLD_MAX | TDSA_HOLD_MIN (display_data_processor.py:371-395)          */
} tdsa_mode;

typedef struct tdsa_info {
  int32_t nfft, max_frames, device_id;
  int32_t grid, block, frames_per_block, lds_bytes; /* launch geometry of the frame kernel          */
  int32_t num_cu;
  int64_t frames_held_max, frames_held_min;          /* frames folded into the hold traces           */
  int32_t avg_count;                                 /* TraceAverager._count                          */
  int32_t version;
} tdsa_info;

/* ---- library / device --------------------------------------------------------------------- */
const char* tdsa_last_error_string(void);
int tdsa_version(void);
int tdsa_device_count(int* count);

/* ---- plan lifetime ------------------------------------------------------------------------ */
/* One plan = (device, FFT size, batch capacity).  Replaces _allocate_fft_resources
 * (datasources/hackrf_samples.py:311-324) + the per-source TraceAverager (datasources/base.py:59)
 * + the hold buffers mw.max_power_levels / mw.min_power_levels (main.py:70-105).
 * nfft: ANY size from 2 to 2^20 (HackrfSamplesDataSource.set_num_samples
 * is unbounded and np.fft.fft takes any N, hackrf_samples.py:392-405, :370): powers of two 64 .. 16384 run as ONE
 * LDS-resident kernel; 2^15 .. 2^20 as N1 x 16384 in two passes (in-register column DFT kernel + a 16384-point
 * row pass); sizes 2^a 3^b 5^c as a mixed-radix transform of exactly nfft points (tdsa_smooth.hip: in LDS up to 10 000 points,
 * two passes above);
 * every other size as a chirp-z convolution on the power-of-two kernels, M = 2^ceil(log2(2 nfft - 1))
 * (tdsa_chirp.hip: same modes, state and outputs, one row per frame; M <= 16384 - sizes up to 8192 - as ONE kernel per
 * call, about 5x the time of a native size; larger M through the long-frame kernels; sizes above 2^19 as four half-length
 * sub-convolutions of 2^20 points; fftshift by nfft / 2 as np.fft.fftshift does for odd sizes).  A plan of
 * 2^15 .. 2^20 points (a power of two: "long-frame plan") takes one
 * frame per call, or - with avg_mode lin and avg_n >= the frames seen since the last reset - a batch of K
 * segments whose Welch average comes back as ONE dB row. */
int tdsa_create(int device_id, int nfft, int max_frames, tdsa_plan* out);
int tdsa_destroy(tdsa_plan p);
int tdsa_get_info(tdsa_plan p, tdsa_info* out);

/* Window table, n == nfft float32 values built by the host exactly as the reference builds them
 * (np.hanning(N).astype(f32) / sqrt(mean(w^2)) for HackRF, raw np.hanning/np.hamming/np.ones for RTL;
 * hackrf_samples.py:314-316, rtl_samples.py:199-206).  Applied as x*w before the FFT (:368 / :169). */
int tdsa_set_window(tdsa_plan p, const float* w_host, int n);

/* Replaces set_psd_mode / set_averaging / set_dc_alpha / CalibrationManager.get_offset / hold toggles
 * (datasources/base.py:148-165, hackrf_samples.py:654-657, core/calibration_manager.py:29-31).
 * Changing avg_mode/avg_n resets the averager (TraceAverager.set_mode :19-28); setting the same values again does
 * not (the whole mode is one struct: a new calibration offset must not restart an average) - callers that want the
 * reference's unconditional restart follow up with tdsa_reset_state(TDSA_RESET_AVG), as the Python sources do. */
int tdsa_set_mode(tdsa_plan p, const tdsa_mode* m);

/* reset_averaging (base.py:167), hold clears (core/display_manager.py:139-185), _flush_buffers DC
 * reset (hackrf_samples.py:444-445), _clear_tare. */
int tdsa_reset_state(tdsa_plan p, uint32_t what);

/* Tare baseline in dB (core/display_data_processor.py:329-369): NULL disables.  While set, every
 * dB value has baseline[k] subtracted after the calibration offset and before the hold update. */
int tdsa_set_tare_baseline(tdsa_plan p, const float* baseline_db_host, int n);

/* ---- the hot path -------------------------------------------------------------------------- */
/* Batched get_power_levels(): frame k = iq[k*hop : k*hop + nfft],
 * n_frames frames, each: unpack -> DC removal -> window -> FFT -> fftshift -> |X| / |X|^2 ->
 * (PSD scale) -> (TraceAverager) -> dB(+floor) -> +cal offset -> -tare -> max/min hold.
 * Replaces hackrf_samples.py:357-386 / rtl_samples.py:167-188 per frame and
 * display_data_processor.py:177-181 per frame.
 * Host-pointer variants copy in/out synchronously (out_db_host may be NULL: hold/avg only).  They may be called
 * with ordinary (pageable) memory: calls of up to 256 KiB in + out - one displayed frame - are staged through pinned,
 * device-visible buffers of the plan that the kernels read and write in place (no DMA operation: 20 us per call at
 * 1024 points, 35 us at 16384), calls of up to 1 MiB each way bounce through the same buffers with DMA copies.
 * n_samples >= (n_frames-1)*hop + nfft. */
int tdsa_process_i8(tdsa_plan p, const int8_t* iq_host, size_t n_samples, int hop, int n_frames,
                    float* out_db_host);
int tdsa_process_u8(tdsa_plan p, const uint8_t* iq_host, size_t n_samples, int hop, int n_frames,
                    float* out_db_host);
int tdsa_process_c64(tdsa_plan p, const float* iq_host, size_t n_samples, int hop, int n_frames,
                     float* out_db_host);

/* Device-resident variant: iq_dev / out_db_dev are device pointers on the plan's device; the work
 * is enqueued on the plan's stream and the call returns immediately (tdsa_synchronize to wait).
 * This is what bench.py times (inputs resident in HBM).  out_db_dev may be NULL: the plan's state (hold traces,
 * averager) is still updated; with averaging on and both holds off the call then costs the transforms and a short
 * chain only (the averaged spectrum of a capture - Welch at a native size - without its rows: tdsa_get_avg). */
int tdsa_process_dev(tdsa_plan p, int in_format, const void* iq_dev, size_t n_samples, int hop,
                     int n_frames, float* out_db_dev);

/* Several captures ("segments") of one shape in ONE call - what a host loop over queued chunks of the reader
 * thread (datasources/hackrf_samples.py:254-305 drains its queue chunk by chunk, one get_power_levels() each,
 * :339-386) or over recorded seconds does with tdsa_process_dev, handed over at once: capture s starts at
 * iq_dev + s*seg_stride_bytes (n_samples_per_seg samples, frames_per_seg frames at `hop`, framed on its own -
 * no frame straddles two captures) and its dB rows go to out_db_dev + s*out_seg_stride_floats.
 * Results and plan state (hold traces, DC, averager) are exactly those of n_segments consecutive
 * tdsa_process_dev calls.  Where the captures do not depend on each other (no averaging, no tracked DC
 * remover, LDS-resident frame length) all of them leave as ONE persistent launch, which pays the per-launch
 * costs - cold fetch of window and twiddles, hold merge, the ragged last round of frames over the CUs - once
 * per call instead of once per capture; every other mode runs the captures one after the other inside the
 * call.  frames_per_seg <= max_frames; out_db_dev may be NULL; out_seg_stride_floats = 0 means "captures back to back"
 * (frames_per_seg * nfft), a smaller non-zero stride - rows of different captures would overlap - is TDSA_ERR_ARG. */
int tdsa_process_dev_batch(tdsa_plan p, int in_format, const void* iq_dev, size_t seg_stride_bytes,
                           int n_segments, size_t n_samples_per_seg, int hop, int frames_per_seg,
                           float* out_db_dev, size_t out_seg_stride_floats);

/* Real-input path of MicrophoneSamplesDataSource (datasources/audio_samples.py:121-184): frames of
 * stereo float32 samples [L0,R0,L1,R1,...]; every real signal of a frame (the mono mix, left, right - both for
 * stereo) is transformed on its own as signal + 0i, so a loud channel leaves nothing in a quiet one, as in the
 * reference.  Per frame: mean removal, window, N-point FFT, one-sided power with the
 * non-DC / non-Nyquist bins doubled (:131), PSD scale, TraceAverager, 10*log10(. + floor).
 * channel: TDSA_CH_MONO ((L+R)/2), _LEFT, _RIGHT -> out [n_frames][N/2+1];
 *          TDSA_CH_STEREO -> out [n_frames][2][N/2+1] (left averaged, right not, as :158-171).
 * Uses the plan's window, power_scale, log_floor and averager settings (db_mode must be TDSA_DB_POW).
 * Frame lengths: any size up to 16384, and sizes that are not a power of two up to 2^19 = 524288 points; the
 * native long-frame plans (2^15 ... 2^20) and the split chirp-z plans above 2^19 return TDSA_ERR_ARG before any work
 * is queued (tdsa_real_input_supported tells beforehand). */
#define TDSA_CH_MONO 0
#define TDSA_CH_LEFT 1
#define TDSA_CH_RIGHT 2
#define TDSA_CH_STEREO 3
int tdsa_real_input_supported(int nfft);     /* 1 / 0: has tdsa_process_real2 a path for frames of nfft points */
int tdsa_process_real2(tdsa_plan p, const float* lr_host, size_t n_samples, int hop, int n_frames,
                       int channel, float* out_db_host);

/* Hold traces (mw.max_power_levels / mw.min_power_levels); either pointer may be NULL.
 * *frames_held = number of frames folded in (0: trace is empty, buffer left untouched). */
int tdsa_get_hold(tdsa_plan p, float* max_host, float* min_host, int64_t* frames_held);

/* TraceAverager._buffer (float64 linear power, fftshift-ed) and ._count; used by the host to
 * combine per-GPU Welch partials. */
int tdsa_get_avg(tdsa_plan p, double* avg_linear_host, int* count);

/* ---- Welch partials across GPUs ----------------------------------------------------------------
 * One capture whose K segments are averaged on W GPUs (one plan each, avg lin with avg_n >= K): every plan hands out
 * its running mean of linear power - TraceAverager._buffer after `count` frames, utils/signal_processing.py:56-59 -
 * and ONE plan reassembles the overall mean on its device: mean = sum_r count_r mean_r / sum_r count_r in float64, in
 * rank order (reproducible), which becomes that plan's averager state (count = the total) exactly as if it had seen
 * every segment itself, and the dB row 10*log10(mean*scale + floor) + cal offset - tare (+ hold traces) that
 * get_power_levels + _apply_cal_offset would return (core/display_data_processor.py:317-327).  No collective: the
 * partials travel through host memory the caller owns (bench.py: a POSIX shared-memory slab every rank maps). */
/* Pin a range of caller memory (e.g. a shared-memory mapping) so that copies from / to it are plain DMA. */
int tdsa_host_register(void* host, size_t bytes);
int tdsa_host_unregister(void* host);
/* mean_host receives nfft values, float32 (as_f32 != 0: 4 MiB instead of 8 at 2^20 points; the combined dB row moves by
 * < 1e-6 dB) or float64 (exact); *count = frames behind it (0: nothing averaged, buffer untouched).  Synchronous. */
int tdsa_welch_export(tdsa_plan p, void* mean_host, int as_f32, int* count);
/* parts_host: n_parts (<= 64) partial means as tdsa_welch_export wrote them, part_stride_bytes apart; counts[r] = 0
 * skips part r.  The plan must be in avg lin mode with avg_n >= the total.  The dB row goes to out_db_dev (device
 * pointer, asynchronous) and / or out_db_host (then the call synchronises); either may be NULL. */
int tdsa_welch_combine(tdsa_plan p, const void* parts_host, size_t part_stride_bytes, const int32_t* counts, int n_parts,
                       int as_f32, float* out_db_dev, float* out_db_host);
/* The same exchange without the detour through host memory, for ranks on GPUs of one node: every rank keeps its partial
 * mean in a device buffer the other processes can map (HIP IPC: tdsa_peer_alloc hands out the 64-byte handle, which
 * travels through any host channel; tdsa_peer_open maps it on the combining rank's device, refusing devices without peer
 * access), tdsa_welch_export_dev writes the running mean there (synchronous: the values have landed when it returns) and
 * tdsa_welch_combine_dev reads all partials IN PLACE - its own from HBM, the others' over xGMI, each over its own link -
 * with the arithmetic, state and outputs of tdsa_welch_combine.  Still no collective and no RCCL: one kernel on one
 * device loading through mapped peer pointers.  owner_device_id < 0 skips the peer-access check. */
#define TDSA_PEER_HANDLE_BYTES 64
int tdsa_peer_alloc(int device_id, size_t bytes, void** dev_ptr, unsigned char* handle64);
int tdsa_peer_free(int device_id, void* dev_ptr);
/* hipDeviceCanAccessPeer(device_id -> peer_device_id): what tdsa_peer_open checks, for a launcher that wants to report the
 * node's peer matrix before it picks the exchange */
int tdsa_peer_can_access(int device_id, int peer_device_id, int* can_access);
int tdsa_peer_open(int device_id, const unsigned char* handle64, int owner_device_id, void** dev_ptr);
int tdsa_peer_close(int device_id, void* dev_ptr);
int tdsa_welch_export_dev(tdsa_plan p, void* mean_dev, int as_f32, int* count);
int tdsa_welch_combine_dev(tdsa_plan p, const void* const* parts_dev, const int32_t* counts, int n_parts, int as_f32,
                           float* out_db_dev, float* out_db_host);

/* Saturated VALU rate of the SIMDs right now - independent v_add_f32 chains, four waves per SIMD on every CU, about a
 * millisecond, timed with events on the plan's stream: *ns_per_valu = ns per wave-instruction per SIMD,
 * *shader_mhz = 2 clocks / that (a gfx950 SIMD retires one fp32 wave-instruction per 2 clocks).  bench.py reports it
 * next to the frame kernel's time: the kernel is VALU-issue bound, so kernel time x clock is what compares across boxes. */
int tdsa_shader_clock(tdsa_plan p, float* shader_mhz, float* ns_per_valu);

/* HackrfSamplesDataSource._dc_estimate (complex, units of x). */
int tdsa_get_dc(tdsa_plan p, float* re, float* im);
/* ... and its assignment: the estimate belongs to the source, not to an FFT size - the reference keeps it across
 * set_num_samples (datasources/hackrf_samples.py:392-405), which is a new plan here. */
int tdsa_set_dc(tdsa_plan p, float re, float im);

int tdsa_synchronize(tdsa_plan p);

/* Let consecutive tdsa_process_dev calls overlap on up to n_streams (1..4) HIP streams owned by the plan.
 * A persistent launch ends ragged (2440 frames over 256 CUs = 9 or 10 frames per workgroup); with more
 * than one stream the next call's workgroups start on the CUs that finish first and the inter-kernel
 * gap disappears.  With n_streams >= 3 the overlapped launches are sized for half the CUs, so that two run side by
 * side and the third queues behind them: a workgroup's fixed costs are spread over twice the frames (C3: 76.4 ->
 * 74.3 us per step; strictly serial launches keep the whole chip).  Only calls whose results do not depend on
 * execution order rotate over the extra streams: no averaging, dc_alpha < 0 or >= 1 (hold traces are
 * merged with atomics and stay exact).  Every other entry point first orders the plan's main stream
 * after the work in flight, so the API stays sequentially consistent; with overlap on, tdsa_get_dc
 * reports the last frame of whichever call finished last.  n_streams = 1 (default) restores strictly
 * serial execution.  No counterpart in the reference (its path is one frame per 20 ms timer tick,
 * core/ui_setup.py:60-61); this is the batch front end of SURVEY.md 8(a) a2. */
int tdsa_set_overlap(tdsa_plan p, int n_streams);

/* ---- trace objects: DataProcessor / TraceAverager arithmetic on host-provided rows ------------- */
/* -------- trace analytics on device-resident rows --------------------------
 * rows_dev: [n_rows][n_bins] float32 dB rows on the plan's device, e.g. what tdsa_process_dev wrote;
 * the calls are ordered after everything the plan has in flight and return with the results on the host.
 *
 * tdsa_rows_stats      per row: np.max (DutyCycleAnalyser.update_from_power, core/duty_cycle.py:36),
 *                      np.argmax (marker snap fallback, core/marker_manager.py:97; first index of equal
 *                      maxima, NaN wins like numpy) and MarkerManager._band_power over the inclusive bin
 *                      range [band_lo, band_hi] (core/marker_manager.py:308-319: 10 log10(max(sum(10^(dB/10))
 *                      * bin_width, 1e-30)); NaN when band_lo > band_hi = "no bin in the band" -> None).
 *                      Any output pointer may be NULL.
 * tdsa_rows_top_peaks  DataProcessor._find_top_peaks (core/display_data_processor.py:432-471): up to
 *                      n_peaks (<= 8) strongest strict local maxima that are >= min_sep_bins apart and
 *                      separated by a valley min_excursion_db below both; bins [n_rows][n_peaks] padded
 *                      with -1 (dB padded with NaN).  n_bins <= 16384 (the row lives in LDS).  Equal-valued
 *                      candidates are visited larger index first (the reference's order for ties is that
 *                      of np.argsort's unstable sort).
 *                      min_excursion_db IS a float32: the contract is the reference called with that float32 value
 *                      (float(np.float32(x))), in its first, float32 comparison and in its second, float64 one - a
 *                      caller's 6.3 means 6.30000019...; NaN is TDSA_ERR_ARG.  min_sep_bins < 1 means "no separation
 *                      rule" (the reference's `abs(a - b) < min_sep_bins` then never holds), the same as 1; any value
 *                      from n_bins up means the same as n_bins.  A NaN between two peaks never rejects (the
 *                      reference's np.min of the valley is NaN and both of its comparisons are false); a NaN is no
 *                      candidate and takes its two neighbours out of the candidates.  n_peaks outside [1, 8] and
 *                      n_bins outside [1, 16384] are TDSA_ERR_ARG; peak_db_host may be NULL; n_rows = 0 returns
 *                      TDSA_OK and writes nothing.
 * tdsa_rows_marker_peaks  MarkerManager.snap_to_peak / snap_to_next_peak (core/marker_manager.py:74-127): per row
 *                      scipy.signal.find_peaks(levels, height=, prominence=, distance=) - local maxima (a flat top
 *                      counts once, at its middle; never the first / last sample), height >= `height`, from the
 *                      highest peak down every peak closer than `distance` bins to a kept one is removed, then
 *                      prominence >= `prominence` (float64, the walk scipy does with wlen = None) - and what the
 *                      two methods take from it: snap_bin = the highest peak (first of equals), or np.argmax of
 *                      the row when no peak qualifies (:93-97); next_bin = the first peak right of current_idx
 *                      (= np.searchsorted(bins, marker position)), wrapping to the first peak, -1 when there is
 *                      none (:120-126: the marker stays).  The reference calls it with height = peak_threshold
 *                      (default -200), prominence = peak_excursion (default 6), distance = 3.  Optionally the
 *                      first max_list peaks in bin order (padded with -1) and their prominences (NaN).  Any
 *                      output pointer may be NULL.  n_bins <= 16384.  Two EQUAL peaks closer than `distance`:
 *                      the larger bin is kept (scipy orders them by np.argsort, whose default sort is not stable:
 *                      the reference's choice between them depends on the CPU's sorting network).  `distance` from
 *                      n_bins up means the same as n_bins.
 *                      rows_dev of both calls must be aligned to a float (4 bytes; TDSA_ERR_ARG otherwise) and to no
 *                      more: the marker search takes 16-byte loads only where n_bins % 4 == 0 AND rows_dev is 16-byte
 *                      aligned, float loads otherwise, with the same results. */
int tdsa_rows_stats(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, int band_lo, int band_hi,
                    double bin_width, float* peak_db_host, int32_t* peak_bin_host, double* band_db_host);
int tdsa_rows_top_peaks(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, int n_peaks, int min_sep_bins,
                        float min_excursion_db, int32_t* peak_bins_host, float* peak_db_host);
/* Per-frame scalars as a by-product of the spectra ("fused as optional epilogues so only scalars
 * return to the host").  With enable != 0 every tdsa_process_* call also leaves, per frame, what tdsa_rows_stats would
 * report for its dB row: peak_db = np.max (DutyCycleAnalyser.update_from_power, core/duty_cycle.py:36), peak_bin =
 * np.argmax (marker snap fallback, core/marker_manager.py:97; first of equals, a NaN first) and band_lin = the sum of
 * 10^(dB / 10) over the inclusive display-bin range [band_lo, band_hi] (MarkerManager._band_power,
 * core/marker_manager.py:308-319, before `* bin_width` and the log; band_lo > band_hi: no band, zeros).
 * Frames of 1024 ... 16384 points in the plain dB modes (no averaging, no tare, hold none / max): the frame kernel's
 * waves form them from the bins in their registers: a wave leaves its maximum, its band sum and the sixteen dB values of
 * the one lane that holds the maximum (80 bytes per wave and frame; ties between lanes and NaNs are resolved in the
 * kernel); tdsa_get_frame_stats folds a frame's waves when it is called.  No second pass over the rows, which need not
 * even be written (out_db_dev = NULL).  band_lin is summed from the linear power the kernel holds (float32 per wave,
 * float64 across waves; within 1e-5 relative of the sum over the rounded dB values, one
 * float32 unit of a dB value near -110 being 2e-6 of the power).  Every other plan / mode: rows_stats_kernel runs on
 * the rows the call wrote (a call without rows then has no statistics).  Not for plans above 16384 x 2^k points that
 * return one row per call.  The results of the last four calls are kept: calls_back = 0 is the latest call, 1 the one
 * before ... - tdsa_get_frame_stats waits for that call only, so overlapped calls (tdsa_set_overlap) stay in flight.
 * Any output pointer may be NULL; *n_frames = frames of that call (batched captures: all of them, capture after
 * capture). */
int tdsa_set_frame_stats(tdsa_plan p, int enable, int band_lo, int band_hi);
int tdsa_get_frame_stats(tdsa_plan p, int calls_back, int capacity, int* n_frames, float* peak_db_host,
                         int32_t* peak_bin_host, double* band_lin_host);
int tdsa_rows_marker_peaks(tdsa_plan p, const float* rows_dev, int n_rows, int n_bins, double height, double prominence,
                           int distance, int current_idx, int max_list, int32_t* n_peaks_host, int32_t* snap_bin_host,
                           int32_t* next_bin_host, int32_t* peak_bins_host, double* peak_prom_host);

/* -------- display accumulators kept on the device ---------------------------
 * tdsa_density: DensityDisplay._hist (displays/density_display.py:300-320): float32 [n_bins][512]
 * amplitude histogram over -200..+100 dB; every row first multiplies the histogram by `decay` (when
 * decay < 1) and then adds 1 at int32((dB + 200) / 300 * 512) (truncation toward zero; NaN and out of
 * range dropped), rows applied in order with float32 arithmetic.  _update_dev takes rows already on the
 * device (p = the plan that produced them, or NULL), _update one host row (the per-tick call: returns
 * when the row is staged in pinned memory and its update queued - every other entry point is ordered
 * behind it and _read waits), _read copies the histogram or log1p(histogram) (what setImage receives).
 * tdsa_waterfall: Waterfall._buf (displays/waterfall.py:163-180), a circular row buffer initialised to
 * min_db; a row that equals the previous pushed row (np.array_equal) is skipped (:330-336), a new one
 * is written at ptr = (ptr - 1) % H; _view returns what the reference's buf[ptr : ptr + H] holds (newest
 * first).  The reference doubles the buffer ([2H][n_bins], every row at ptr and ptr + H) so that the view
 * is one slice; the device ring keeps every line once and _view copies its two runs.  These keep C4's 2 GiB of rows on the GPU: only the image leaves. */
typedef struct tdsa_density_s* tdsa_density;
int tdsa_density_create(int device_id, int n_bins, float decay, tdsa_density* out);
int tdsa_density_destroy(tdsa_density d);
int tdsa_density_set_decay(tdsa_density d, float decay);
int tdsa_density_reset(tdsa_density d);
int tdsa_density_update_dev(tdsa_density d, tdsa_plan p, const float* rows_dev, int n_rows);
int tdsa_density_update(tdsa_density d, const float* row_host, int n);
int tdsa_density_read(tdsa_density d, float* hist_host, int as_log1p);
/* The image as the display takes it - what ImageItem.setImage(np.log1p(hist), autoLevels=True) feeds its colour table
 * (displays/density_display.py:318): uint8 [n_bins][512], float32 (v - lo) / (hi - lo) * 255 clipped and truncated with
 * lo / hi = the image's minimum / maximum (returned in levels2, may be NULL; pyqtgraph samples a large image for its auto
 * levels, here they are those of the whole image).  One byte per pixel over PCIe instead of four. */
int tdsa_density_read_u8(tdsa_density d, uint8_t* img_host, float* levels2);

/* -------- constellation analysis (displays/constellation_2d.py:104-160) ---------------------
 * What Constellation2D.update_iq_data computes for one block of complex IQ (TDSA_IN_I8 / _U8 / _C64; real input - the
 * reference's Hilbert path - is TDSA_ERR_ARG), bit for bit: rms = sqrt(mean(|iq|^2)) in float32 with numpy's summation
 * order, the AGC iq / rms when rms > float32(1e-10), EVM = sqrt(mean(min over the reference points |iq - p|^2)) in the
 * table's dtype, and np.histogram2d(i, q, bins, [[-range, range], [-range, range]]) laid out as the image
 * ([q_bin][i_bin], uint32 counts; the image is log1p of them).
 * _set_refs: n_points (<= 64) x {x, y} interleaved, float32 (is_f64 = 0) or float64; 0 points = no EVM (the
 * reference's None for an unknown modulation); a NaN or infinite point is refused.
 * _set_density: 1 <= bins <= 128, range > 0 and finite.
 * _process: one host block of n <= max_host_samples samples (one host wait): rms, evm (has_evm = 0 <=> None), counts
 * [bins][bins], and the last n_tail normalised points as float32 i[n_tail] then q[n_tail] (n_tail is clamped to n);
 * any output may be NULL.
 * _process_dev: a capture already on the device (aligned to one sample), n_seg segments of seg_len samples every hop
 * samples, each exactly what _process gives for that slice alone: rms / EVM per segment to the host (either may be
 * NULL; EVM NaN without a table), counts [n_seg][bins][bins] to a device buffer (or NULL); p = the plan whose stream
 * produced the capture (ordered after it), or NULL. */
typedef struct tdsa_constellation_s* tdsa_constellation;
int tdsa_constellation_create(int device_id, size_t max_host_samples, tdsa_constellation* out);
int tdsa_constellation_destroy(tdsa_constellation c);
int tdsa_constellation_set_refs(tdsa_constellation c, const void* xy, int n_points, int is_f64);
int tdsa_constellation_set_density(tdsa_constellation c, double range, int bins);
int tdsa_constellation_process(tdsa_constellation c, int in_format, const void* iq_host, size_t n, int n_tail,
                               float* rms, double* evm, int* has_evm, uint32_t* counts, float* tail_iq);
int tdsa_constellation_process_dev(tdsa_constellation c, tdsa_plan p, int in_format, const void* iq_dev,
                                   size_t seg_len, size_t hop, int n_seg, float* rms_host, double* evm_host,
                                   uint32_t* counts_dev);

/* -------- zoom front end: digital down-conversion ------------------------------------------
 * Inputs are counted from the last reset, across calls: n = 0, 1, ...  x[n] is the unpacked sample (TDSA_IN_I8:
 * (I + jQ)/128; _U8: float32 of u/127.5 - 1 in float64; _C64 as is), p[n] = p_b + (n - n_b) * phase_step mod 2^32
 * with (p_b, n_b) the phase and the input index at the last set_nco (a reset: p = 0 at n = 0),
 * v[n] = x[n] exp(-2 pi j p[n] / 2^32) (v[n] = 0 for n < 0), and y[m] = sum_{k < T} h[k] v[mD - k], complex64.
 * Output m is emitted by the call that delivers input m D: after n_total inputs there are ceil(n_total / D) outputs.
 * Any split of the input into calls gives the same bits.  2 <= D <= 4096, 1 <= T <= max_taps <= 64 D.
 * _set_taps: float32 taps (finite), also resets history and phase.  _set_nco: the phase stays continuous.
 * _reset: history and phase to zero (the step is kept); returns when every earlier call of the handle has finished.
 * _process: one host block of n_in <= max_host_samples samples (one copy in, one copy back, one host wait); out_host
 * holds up to n_in / D + 1 complex64 values.  _process_dev: input and output in device memory; on plan p's stream
 * (ordered after its work, and its later work after this), or on the handle's own stream for p = NULL; no host wait.
 * Both set *n_out from host-side counts.  Argument errors are reported before any HIP call. */
typedef struct tdsa_ddc_s* tdsa_ddc;
int tdsa_ddc_create(int device_id, int decimation, int max_taps, size_t max_host_samples, tdsa_ddc* out);
int tdsa_ddc_destroy(tdsa_ddc d);
int tdsa_ddc_set_taps(tdsa_ddc d, const float* taps_host, int n_taps);
int tdsa_ddc_set_nco(tdsa_ddc d, uint32_t phase_step);
int tdsa_ddc_reset(tdsa_ddc d);
int tdsa_ddc_process(tdsa_ddc d, int in_format, const void* iq_host, size_t n_in, float* out_host, size_t* n_out);
int tdsa_ddc_process_dev(tdsa_ddc d, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                         size_t* n_out);
/* A copy on plan p's stream, in order with its work (device to device, or device to host); wait = 1 waits for the
 * stream afterwards.  ZoomSpectrum moves its unframed decimated samples and reads its rows with it. */
int tdsa_plan_copy(tdsa_plan p, void* dst, const void* src, size_t bytes, int wait);

/* -------- polyphase channelizer: every fs / M channel of a capture in one pass ------------
 * M channels (a power of two, 4 .. 256), oversampling os = 1 or 2, decimation D = M / os, a prototype of T float32
 * taps (1 <= T <= max_taps <= 40 M), x[n] the unpack of the down-converter above, counted from the last reset:
 *   y_c[m] = sum_{k < T} h[k] x[mD - k] exp(-2 pi j c (mD - k) / M), c = 0 .. M - 1, complex64
 * - the down-converter at phase step c 2^32 / M, decimation D and the same taps.  Channel c is centred at c fs / M for
 * c < M / 2 and at (c - M) fs / M from there on.  Output m of every channel is emitted by the call that delivers input
 * m D; any split of the input into calls gives the same bits.  Evaluated as branch sums w_m[r] = sum_q h[qM + r]
 * x[mD - qM - r] (one fma chain over q), placed at p = (r - mD) mod M, and an unnormalised radix-2 inverse DFT over p.
 * The outputs of a call are stored channel-major: y_c[m_first + i] at out + c * out_stride + i (complex64 units),
 * i < n_out <= out_stride.  flags: TDSA_CHAN_BRANCHES stores the shifted branch sums W_m[p] at row p instead of y_c[m].
 * _set_taps: finite taps, also resets the history.  _reset: history and input count to zero; returns when every earlier
 * call of the handle has finished.  _process: one host block of n_in <= max_host_samples samples (one copy in, one
 * copy back, one host wait).  _process_dev: input and output in device memory; on plan p's stream (ordered after its
 * work, and its later work after this), or on the handle's own stream for p = NULL; no host wait.  Both set *n_out
 * (per channel) from host-side counts.  Argument errors are reported before any HIP call. */
#define TDSA_CHAN_BRANCHES 1u
typedef struct tdsa_chan_s* tdsa_chan;
int tdsa_chan_create(int device_id, int channels, int oversample, int max_taps, size_t max_host_samples,
                     tdsa_chan* out);
int tdsa_chan_destroy(tdsa_chan c);
int tdsa_chan_set_taps(tdsa_chan c, const float* taps_host, int n_taps);
int tdsa_chan_reset(tdsa_chan c);
int tdsa_chan_process(tdsa_chan c, int in_format, const void* iq_host, size_t n_in, float* out_host,
                      size_t out_stride, unsigned flags, size_t* n_out);
int tdsa_chan_process_dev(tdsa_chan c, tdsa_plan p, int in_format, const void* iq_dev, size_t n_in, void* out_dev,
                          size_t out_stride, unsigned flags, size_t* n_out);

/* -------- analog demodulation: AM / FM audio, deviation, depth ----------------------------
 * C channels (1 .. 256) of complex64, channel c's samples of a call at in + c * in_stride (complex64 units), counted
 * from the last reset across calls, x[-1] = 0.  Per channel:
 *   d[n] = arg(x[n] conj x[n-1]) / pi in (-1, 1] (TDSA_DEMOD_FM; one unit is f_i / 2 Hz; 0 where the product is 0, +1
 *          where it is negative real) or |x[n]| (TDSA_DEMOD_AM)
 *   a[m] = sum_{k < T} g[k] d[mR - k], d = 0 before sample 0; decimation R = 1 .. 64, T float32 taps, 1 <= T <= 64 R
 *   y[m] = c y[m-1] + (1 - c) a[m], y[-1] = 0, 0 <= c < 1
 *   out[m] = s a[m] (TDSA_DEMOD_POLE_OFF), s y[m] (_LOWPASS: de-emphasis) or s (a[m] - y[m]) (_HIGHPASS: carrier removal)
 * Output m comes out of the call that delivers input mR; any split of the input into calls gives the same bits.  The
 * outputs of a call are contiguous float32 at out + c * out_stride (float32 units), n_out <= out_stride per channel.
 * Measurements per channel over a[m] since _reset_meas: count, max, min (exact), sum and sum of squares (float64).
 * _set_taps and _set_pole also reset the handle; _reset zeroes the history, the pole state, the sample count and the
 * measurements and returns when every earlier call has finished.  _process: host memory through pinned staging (one
 * copy in, one copy out, one host wait), at most max_host_samples / channels samples per channel and call.
 * _process_dev: device memory, on plan p's stream (ordered after its work, and its later work after this) or on the
 * handle's own for p = NULL; no host wait.  _read_meas: five arrays of `channels` entries.  Argument errors are reported
 * before any HIP call. */
#define TDSA_DEMOD_FM 0
#define TDSA_DEMOD_AM 1
#define TDSA_DEMOD_POLE_OFF 0
#define TDSA_DEMOD_POLE_LOWPASS 1
#define TDSA_DEMOD_POLE_HIGHPASS 2
typedef struct tdsa_demod_s* tdsa_demod;
int tdsa_demod_create(int device_id, int mode, int channels, int decimation, int max_taps, size_t max_host_samples,
                      tdsa_demod* out);
int tdsa_demod_destroy(tdsa_demod d);
int tdsa_demod_set_taps(tdsa_demod d, const float* taps_host, int n_taps);
int tdsa_demod_set_pole(tdsa_demod d, int pole_mode, double c, float scale);
int tdsa_demod_reset(tdsa_demod d);
int tdsa_demod_process(tdsa_demod d, const void* in_host, size_t n_in, size_t in_stride, float* out_host,
                       size_t out_stride, size_t* n_out);
int tdsa_demod_process_dev(tdsa_demod d, tdsa_plan p, const void* in_dev, size_t n_in, size_t in_stride, void* out_dev,
                           size_t out_stride, size_t* n_out);
int tdsa_demod_read_meas(tdsa_demod d, int64_t* count, float* max_f32, float* min_f32, double* sum_f64,
                         double* sumsq_f64);
int tdsa_demod_reset_meas(tdsa_demod d);
int tdsa_demod_timer_begin(tdsa_demod d);
int tdsa_demod_timer_end(tdsa_demod d, float* elapsed_ms);

/* -------- symbol recovery for EVM: timing, carrier, one sample per symbol ------------------
 * Feed-forward and per segment: segment s is x[s * hop + j], j < seg_len, complex64, analysed on its own; the handle
 * keeps no state between calls.  Positions are 32.32 fixed point: step = round(sps 2^32) (4 <= sps <= 64), nu =
 * round(2^32 / sps) the symbol clock's phase step per sample.
 *   1 timing    P = sum |x_j|^2, C = sum |x_j|^2 exp(-2 pi i (j nu mod 2^32) / 2^32); a = arg C / pi ((0, 0): 0),
 *               t = -a / 2 (+ 1 if negative), delta_fx = floor(t step), + step if below 2^32.  TDSA_SYMSYNC_FIXED: the
 *               caller's delta_fx instead, 2^32 <= delta_fx < step + 2^32.
 *   2 resample  K = floor((seg_len - 4) 2^32 / step) - 1 symbols (2 .. 4096); pos = delta_fx + k step, i = pos >> 32,
 *               mu = the top 24 bits of the fraction; y_k = the cubic Lagrange interpolation of x[i-1 .. i+2] at mu.
 *   3 carrier   (order M = 2, 4, 8) z = y^M, Z = DFT_G of z zero padded, G = 2 * 2^ceil(log2 K); g = the lowest index of
 *               the largest |Z|^2; f = g / G (less 1 from G / 2 up) + arg(S2 conj S1) / (2 pi H), S1, S2 the sums over
 *               the first and second H = K / 2 of z_k exp(-2 pi i k g / G); step_f = round(f / M 2^32) mod 2^32;
 *               theta_fx = round((arg sum z_k exp(-2 pi i k M step_f / 2^32) - ref_arg) / (2 pi M) 2^32) mod 2^32.
 *   4 derotate  sym_k = y_k exp(-2 pi i ((theta_fx + k step_f) mod 2^32) / 2^32); order 0: sym = y.
 * Symbols: complex64, segment s at sym + s * out_stride, the first K of each row are written.  raw (or NULL): the same
 * shape, y.  One record per segment.  A segment whose P or C is not finite has TDSA_SYMSYNC_NONFINITE set, NaN symbols
 * and an otherwise zero record; no other segment is touched.  TDSA_SYMSYNC_NO_CARRIER: the transform's power is not
 * finite, step_f = theta_fx = 0.  A segment's results depend on its samples alone: not on n_seg, its place or the entry
 * point.  _process: host memory through pinned staging, n_samples and n_seg * seg_len <= max_host_samples; a hop that
 * takes a segment beyond the block is refused whatever its size.
 * _process_dev: device memory, on plan p's stream (ordered after its work, and its later work after this) or on the
 * handle's own for p = NULL; returns when the records are in records_host.  _symbols_per_segment needs no device.
 * Argument errors are reported before any HIP call. */
#define TDSA_SYMSYNC_AUTO 0
#define TDSA_SYMSYNC_FIXED 1
#define TDSA_SYMSYNC_NONFINITE 1u
#define TDSA_SYMSYNC_NO_CARRIER 2u
typedef struct tdsa_symsync_record {
  uint64_t delta_fx;           /* the first symbol's position in the segment, 32.32 samples */
  float c_re, c_im, p;         /* the symbol-rate line of |x|^2 and the segment's energy */
  int32_t g;                   /* the carrier transform's peak bin, 0 .. G - 1 */
  uint32_t step_f, theta_fx;   /* carrier per symbol and phase, in turns / 2^32 */
  float peak, mean;            /* |Z_g|^2 and the mean of |Z|^2: the carrier lock's quality */
  uint32_t flags, reserved;
} tdsa_symsync_record;
typedef struct tdsa_symsync_s* tdsa_symsync;
int tdsa_symsync_create(int device_id, size_t max_host_samples, tdsa_symsync* out);
int tdsa_symsync_destroy(tdsa_symsync h);
int tdsa_symsync_configure(tdsa_symsync h, uint64_t step, uint32_t nu, int order, double ref_arg, int timing_mode,
                           uint64_t delta_fx);
int tdsa_symsync_process(tdsa_symsync h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                         void* sym_host, size_t out_stride, void* raw_host, tdsa_symsync_record* records_host);
int tdsa_symsync_process_dev(tdsa_symsync h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                             void* sym_dev, size_t out_stride, void* raw_dev, tdsa_symsync_record* records_host);
int tdsa_symsync_symbols_per_segment(uint64_t step, size_t seg_len, int* K);
int tdsa_symsync_timer_begin(tdsa_symsync h);
int tdsa_symsync_timer_end(tdsa_symsync h, float* elapsed_ms);

/* -------- FSK analysis: symbol clock, deviation, symbols, FSK error --------------------------
 * Feed-forward and per segment like the symbol recovery above, whose 32.32 positions, step, nu and resampler it shares:
 * segment s is in[s * hop + j], j < seg_len, analysed on its own; the handle keeps no state between calls.  Input:
 * TDSA_FSK_IQ complex64, or TDSA_FSK_FREQ float32 that is a frequency already.  levels M = 2, 4 or 8; a level is an odd
 * integer l = 2 i - (M - 1), i = 0 .. M - 1.
 *   0 discriminate  (IQ) d_j = arg(x[j+1] conj x[j]) / pi in half turns per sample, j < n_d = seg_len - 1; not unwrapped:
 *                   the signal is taken to stay inside +-fs/2.  (FREQ) d_j = in_j, n_d = seg_len.
 *   1 boxcar        b_j = (((d_j + d_j+1) + ...) + d_j+B-1) * float32(1 / B), float32 adds in ascending order,
 *                   j < n_b = n_d - B + 1, B = 1 .. 64; B = 1 leaves d bit for bit.
 *   2 timing        e_j = (b_j+L - b_j)^2, j < n_b - L, L = 1 .. 64 (none: P = C = 0); P = sum e_j, C = sum e_j
 *                   exp(-2 pi i (j nu mod 2^32) / 2^32); a = arg C / pi ((0, 0): 0), t = -a / 2 (+ 1 if negative), taken to
 *                   32 fractional bits; delta_fx = (floor(t step) + L 2^31 + (step >> 1)) mod step, + step if below 2^32:
 *                   the transitions of e lie L / 2 samples past their phase, the symbol centres half a symbol later.
 *                   TDSA_FSK_FIXED: the caller's delta_fx instead, 2^32 <= delta_fx < step + 2^32.
 *   3 resample      K = floor((n_b - 4) 2^32 / step) - 1 symbols (2 .. 4096); v_k = the cubic Lagrange interpolation of
 *                   b[i-1 .. i+2] at pos = delta_fx + k step, as the symbol recovery forms it.
 *   4 levels        lo = min v, hi = max v, o = (hi + lo) / 2, g = (hi - lo) float32(1 / (2 (M - 1))); then twice:
 *                   i_k = clamp(floor((v_k - o) / (g + g) + M / 2), 0, M - 1) in float32 (a NaN: 0), l_k = 2 i_k - (M - 1),
 *                   D = K sum l^2 - (sum l)^2 in integers; D != 0: g = (K sum l v - sum l sum v) / D, o = (sum v - g
 *                   sum l) / K in float64, rounded to float32; D = 0 (one level, also hi = lo): o, g stay,
 *                   TDSA_FSK_ONE_LEVEL.  The indices are those of the second round.
 *   5 errors        err_k = v_k - fmaf(g, l_k, o); err_sumsq = sum err_k^2 in float64; err_peak = the largest |err_k|,
 *                   err_peak_k its lowest k.
 * Levels: float32, segment s at out + s * out_stride, the first K of each row are written; idx (or NULL): uint8 of the
 * same shape, i_k.  One 64-byte record per segment.  A segment whose P, C or any v_k is not finite has
 * TDSA_FSK_NONFINITE set, NaN levels, zero indices and an otherwise zero record; no other segment is touched.  Every sum is one fixed tree per (seg_len, B, L, K), so a segment's results depend on its samples
 * alone: not on n_seg, its place or the entry point.  _process: host memory through pinned staging, n_samples and
 * n_seg * seg_len <= max_host_samples.  _process_dev: device memory, on plan p's stream (ordered after its work, and its
 * later work after this) or on the handle's own for p = NULL; returns when the records are in records_host.
 * _symbols_per_segment needs no device.  Argument errors are reported before any HIP call. */
#define TDSA_FSK_IQ 0
#define TDSA_FSK_FREQ 1
#define TDSA_FSK_AUTO 0
#define TDSA_FSK_FIXED 1
#define TDSA_FSK_NONFINITE 1u
#define TDSA_FSK_ONE_LEVEL 2u
typedef struct tdsa_fsk_record {
  uint64_t delta_fx;           /* the first symbol's position among the b_j, 32.32 samples */
  float c_re, c_im, p;         /* the symbol-rate line of e and its sum */
  float offset, dev;           /* o and g: the centre of the levels and half the spacing of adjacent ones */
  float lo, hi;                /* the smallest and the largest v_k */
  float err_peak;
  double err_sumsq;
  int32_t err_peak_k;
  int32_t sum_l;               /* sum of l_k of the second round */
  uint32_t flags, reserved;
} tdsa_fsk_record;
typedef struct tdsa_fsk_s* tdsa_fsk;
int tdsa_fsk_create(int device_id, size_t max_host_samples, tdsa_fsk* out);
int tdsa_fsk_destroy(tdsa_fsk h);
int tdsa_fsk_configure(tdsa_fsk h, uint64_t step, uint32_t nu, int levels, int input_kind, int boxcar, int lag,
                       int timing_mode, uint64_t delta_fx);
int tdsa_fsk_process(tdsa_fsk h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                     float* out_host, size_t out_stride, uint8_t* idx_host, tdsa_fsk_record* records_host);
int tdsa_fsk_process_dev(tdsa_fsk h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                         void* out_dev, size_t out_stride, void* idx_dev, tdsa_fsk_record* records_host);
int tdsa_fsk_symbols_per_segment(uint64_t step, size_t seg_len, int input_kind, int boxcar, int* K);
int tdsa_fsk_timer_begin(tdsa_fsk h);
int tdsa_fsk_timer_end(tdsa_fsk h, float* elapsed_ms);

/* -------- eye diagrams: I / Q and FSK eyes on a recovered symbol clock ------------------------
 * Folds segments of a stream on one symbol clock per segment - the one the symbol recovery or the FSK analysis has just
 * put into its record, or the caller's - into a density image of P columns over one symbol by H rows over [lo, hi),
 * kept as integers on the device across calls until _reset or _configure.  Segment s is in[s * hop + j], j < seg_len.
 * step = round(sps 2^32), 4 .. 64 samples per symbol; P = 4, 8, 16, 32 or 64; H = 8 .. 256; P H <= 8192; lo < hi, finite.
 *   series   TDSA_EYE_IQ    x itself, complex64, n = seg_len; two eyes: 0 = I, 1 = Q.
 *            TDSA_EYE_FM    complex64: d_j = the FSK analysis' discriminator, b = its boxcar over B = 1 .. 64 (its stages
 *                           0 and 1, bit for bit), n = seg_len - B; one eye.
 *            TDSA_EYE_REAL  float32 through the same boxcar (B = 1: as it is), n = seg_len - B + 1; one eye.
 *   K        the producer's: tdsa_symsync_symbols_per_segment (IQ), tdsa_fsk_symbols_per_segment with TDSA_FSK_IQ (FM)
 *            or _FREQ (REAL) and B; 3 <= K <= 4096.
 *   clock    tdsa_eye_clock per segment.  delta_fx = 0: the segment is counted as skipped and contributes nothing; else
 *            2^32 <= delta_fx < step + 2^32.  step_f and theta_fx are read for IQ only.
 *   points   k = 1 .. K - 2, c = 0 .. P - 1: pos = delta_fx + k step + floor((c - P / 2) step / P) (the floor of the
 *            signed product: an arithmetic shift), i = pos >> 32, mu = the top 24 bits of the fraction; the value is the
 *            symbol recovery's cubic Lagrange interpolation of series[i-1 .. i+2], per part for IQ.  Every tap lies inside
 *            the series.  IQ: v = y exp(-2 pi i phi / 2^32), phi = theta_fx + k step_f + floor((c - P / 2) int32(step_f)
 *            / P) mod 2^32, the symbol recovery's rotation and product; step_f = theta_fx = 0 leaves finite values as
 *            they are.  Column P / 2 is the symbol recovery's symbols [1 .. K - 2], or the FSK analysis' levels
 *            [1 .. K - 2], bit for bit.
 *   rows     scale = float32(double(H) / (double(hi) - double(lo))); t = (v - lo) * scale in float32, two roundings.  NaN:
 *            n_nan; t < 0: n_under; t >= H (+inf too): n_over; else row int(t), row 0 the lowest.
 * State: counts[eyes][H][P] uint64; totals[10] uint64 = per eye {n_points, n_under, n_over, n_nan} (eye 1 zero for FM and
 * REAL), then {segments, skipped}.  Sums of integers: the same bits for any split of the segments over calls, any n_seg,
 * either entry point.  sum counts + n_under + n_over + n_nan = n_points = (segments - skipped) (K - 2) P per eye.
 * traces (or NULL): [n_seg][K - 2][P] float32 (FM, REAL) or complex64 (IQ); a skipped segment's are left untouched.
 * _process: host memory through pinned staging, n_samples <= max_host_samples; returns when the staging is free.
 * _process_dev: device samples (and traces), host clocks (copied before the call returns), on plan p's stream or the
 * handle's own for p = NULL; does not wait.  _read waits and copies eyes H P counts and the 10 totals.
 * _symbols_per_segment needs no device.  Argument errors are reported before any HIP call. */
#define TDSA_EYE_IQ 0
#define TDSA_EYE_FM 1
#define TDSA_EYE_REAL 2
#define TDSA_EYE_MAX_BINS 8192
#define TDSA_EYE_TOTALS 10
typedef struct tdsa_eye_clock {
  uint64_t delta_fx;           /* the first symbol's position in the series, 32.32 samples; 0 = skip the segment */
  uint32_t step_f, theta_fx;   /* IQ: the carrier's phase step per symbol and its phase at symbol 0, turns / 2^32 */
} tdsa_eye_clock;
typedef struct tdsa_eye_s* tdsa_eye;
int tdsa_eye_create(int device_id, size_t max_host_samples, int max_segments, tdsa_eye* out);
int tdsa_eye_destroy(tdsa_eye h);
int tdsa_eye_configure(tdsa_eye h, uint64_t step, int kind, int boxcar, int points, int rows, float lo, float hi);
int tdsa_eye_symbols_per_segment(uint64_t step, size_t seg_len, int kind, int boxcar, int* K);
int tdsa_eye_process(tdsa_eye h, const void* in_host, size_t n_samples, size_t seg_len, size_t hop, int n_seg,
                     const tdsa_eye_clock* clocks_host, void* traces_host);
int tdsa_eye_process_dev(tdsa_eye h, tdsa_plan p, const void* in_dev, size_t seg_len, size_t hop, int n_seg,
                         const tdsa_eye_clock* clocks_host, void* traces_dev);
int tdsa_eye_read(tdsa_eye h, uint64_t* counts_host, uint64_t* totals_host);
int tdsa_eye_reset(tdsa_eye h);
int tdsa_eye_timer_begin(tdsa_eye h);
int tdsa_eye_timer_end(tdsa_eye h, float* elapsed_ms);

/* -------- modulation quality: decisions, gain / phase / offset fit, error vector -------------
 * The last stage of the chain for linear modulations (BPSK .. 64QAM, any table of up to 64 points): rows of symbols as
 * the symbol recovery leaves them, segment s = y[s * in_stride + k], k < K, complex64, 2 <= K <= 4096, in_stride >= 1
 * (rows may overlap).  _set_points takes T = 1 .. 64 finite float32 pairs r_i, not all zero, and uploads beside them
 * r_abs[i] = sqrtf(fl(fl(re^2) + fl(im^2))) and inv_rho = float32(1 / sqrt(sum |r_i|^2 / T)), formed in float64.
 * Float32 and float64 arithmetic is written operation by operation, nothing is fused; a product of two float32 values
 * is exact in float64; a complex product is four products, one difference and one sum.  Every sum over k is one fixed
 * tree per K: thread t of 256 folds k = t, t + 256, ... in order from 0.0, the 64 partial sums of a wave fold by the
 * xor butterfly (v = v + the value of lane ^ o, o = 32 .. 1), the four wave sums as (W0 + W1) + (W2 + W3).
 *   0 first guess  S_y = sum y, S_yy = sum (re^2 + im^2) in float64.  c0 = float32(S_y / K) per part; v = S_yy / K -
 *                  (Re(S_y / K)^2 + Im(S_y / K)^2); a0 = (sqrtf(float32(max(v, 0))) inv_rho, 0).  S_y or S_yy not finite:
 *                  TDSA_MODQ_NONFINITE, zero indices, NaN error vectors, an otherwise zero record; no other segment is
 *                  touched.  a0 = 0: TDSA_MODQ_DEGENERATE, zero indices, a = 0, c = c0, error vectors y - c0 and
 *                  err_sumsq, err_peak, err_peak_k from them; the other sums, s_ry, s_cy and changed are zero.
 *   1 decide       q = conj(a) / (a_re^2 + a_im^2) in float64, each part rounded to float32 once; t = y - c; w = t q;
 *                  d_i = fl(fl((w_re - r_re)^2) + fl((w_im - r_im)^2)); the index is the lowest i of the smallest d_i
 *                  (compared with <; a NaN never wins; every d_i NaN: 0).
 *   2 fit          n_i = the symbols decided for point i.  In float64 and in index order S_r = sum n_i r_i, S_rr =
 *                  sum n_i (re^2 + im^2); tree sums S_ry = sum conj(r_k) y_k, S_cy = sum r_k y_k.  D = K S_rr - |S_r|^2;
 *                  a = (K S_ry - conj(S_r) S_y) / D, c = (S_y - a S_r) / K with the unrounded a, each part rounded to
 *                  float32 once.  Every symbol on one index, or D <= 0: a and c stay, TDSA_MODQ_ONE_POINT.
 *   3 two rounds   round 1 decides with (a0, c0) and fits, round 2 decides with that fit and fits again; `changed` counts
 *                  the k whose index differs between the rounds.
 *   4 errors       against round 2's indices with the final (a, c): w as in 1, eps_k = w_k - r_k, e2_k = fl(fl(eps_re^2) +
 *                  fl(eps_im^2)), m_k = sqrtf(fl(fl(w_re^2) + fl(w_im^2))) - r_abs, p_k = the demodulator's atan2 / pi of
 *                  w_k conj(r_k) in half turns (0 where r_k = 0).  Tree sums of e2, m^2, p^2 in float64; ref_sumsq is
 *                  round 2's S_rr.  err_peak is the largest e2 with the lowest k, compared with > from 0 at k = 0.
 * Outputs: one record per segment, the indices as uint8 [n_seg][out_stride] and, unless err is NULL, eps as complex64 of
 * the same shape (the error vector over time); the gaps of out_stride > K are not touched.  Given y, the record, the
 * indices and eps are this text's bit for bit, phase_sumsq within the arctangent's bound.  A segment's bits do not
 * depend on n_seg, its place or the entry point.
 * _process: a host block of n_symbols <= max_host_symbols through pinned staging.  _process_dev: device pointers
 * (symbols and error vectors aligned to 8 bytes), on plan p's stream (ordered after its work, and its later work after
 * this) or the handle's own for p = NULL.  Both return when the records are in host memory.  Argument errors are
 * reported before any HIP call. */
#define TDSA_MODQ_MAX_POINTS 64
#define TDSA_MODQ_MAX_SYMBOLS 4096
#define TDSA_MODQ_NONFINITE 1u
#define TDSA_MODQ_DEGENERATE 2u
#define TDSA_MODQ_ONE_POINT 4u
typedef struct tdsa_modq_record {
  float a_re, a_im, c_re, c_im;          /* y ~ a r + c */
  double s_y[2], s_yy, s_ry[2], s_cy[2]; /* S_y, S_yy, and round 2's S_ry, S_cy */
  double err_sumsq, ref_sumsq, mag_sumsq, phase_sumsq;
  float err_peak;                        /* the largest e2 ... */
  uint32_t err_peak_k;                   /* ... and its lowest k */
  uint32_t changed, flags;
  uint32_t reserved[2];
} tdsa_modq_record;
typedef struct tdsa_modq_s* tdsa_modq;
int tdsa_modq_create(int device_id, size_t max_host_symbols, tdsa_modq* out);
int tdsa_modq_destroy(tdsa_modq h);
int tdsa_modq_set_points(tdsa_modq h, const float* points, int n_points);   /* points: n_points (re, im) pairs */
int tdsa_modq_process(tdsa_modq h, const void* in_host, size_t n_symbols, int K, size_t in_stride, int n_seg,
                      uint8_t* idx_host, size_t out_stride, void* err_host, tdsa_modq_record* records_host);
int tdsa_modq_process_dev(tdsa_modq h, tdsa_plan p, const void* in_dev, int K, size_t in_stride, int n_seg, void* idx_dev,
                          size_t out_stride, void* err_dev, tdsa_modq_record* records_host);
int tdsa_modq_timer_begin(tdsa_modq h);
int tdsa_modq_timer_end(tdsa_modq h, float* elapsed_ms);

/* -------- signal detection: noise floor, emissions, occupancy ----------------------------
 * Rows are [n_rows][n_bins] float32 dB rows, 1 <= n_bins <= 16384, the input of tdsa_rows_top_peaks.  Per row, with
 * seg = row[bin_lo .. bin_hi] (inclusive) and n_eff its length:
 *   floor      np.sort(seg)[rank]: NaNs sort last, -inf and +inf take their places; compared by value (+0 / -0).  A NaN
 *              floor flags the row (TDSA_DETECT_NAN_FLOOR): thr is NaN, n_over = n_found = 0, no occupancy.
 *   threshold  thr = floor + margin_db, one float32 addition; a bin is set when row[i] > thr (a NaN never is); n_over
 *              counts the set bins.
 *   runs       consecutive set bins more than max_gap + 1 apart end one run and begin the next (gaps of up to max_gap
 *              bins are bridged); then runs with stop - start + 1 < min_width are dropped.  n_found counts the runs
 *              kept and may exceed max_signals; the first max_signals in bin order get records, the rest of a row's
 *              records are start = stop = peak_bin = x_lo = x_hi = -1, peak_db = NaN, power = moment = 0.
 *   signal     peak_bin = the first bin holding the run's largest non-NaN value, peak_db that value; x_lo / x_hi = the
 *              first / last bin of the run with row[i] >= peak_db - xdb (float32); power = sum p_i, moment =
 *              sum (i - start) p_i over the run's non-NaN bins, p_i = 10^(row[i] / 10) in float32 (tdsa_rows_stats'
 *              expression) summed in float64 - one fixed tree given (start, stop), so a row's records do not depend
 *              on n_rows, its place, the entry point or its alignment.
 *   occupancy  uint32 [n_bins] on the handle: every unflagged row adds its set bins; rows_seen and rows_flagged count
 *              the rows of all calls since the last _reset (or create).
 * _configure fixes the parameters: 0 <= bin_lo <= bin_hi < n_bins, 0 <= rank < n_eff, margin_db finite, 1 <= min_width
 * <= n_bins, 0 <= max_gap <= n_bins, xdb finite and >= 0, 1 <= max_signals <= 64.  _process: host rows through pinned
 * staging, n_rows <= max_host_rows.  _process_dev: rows in device memory (aligned to 4 bytes; 16-byte loads where
 * n_bins % 4 == 0 and rows_dev is 16-byte aligned, float loads otherwise, with the same results), on plan p's stream
 * (ordered after its work, and its later work after this) or on the handle's own for p = NULL.  Both write n_rows row
 * records and n_rows * max_signals signal records and return when they are in host memory; n_rows = 0 returns TDSA_OK
 * and writes nothing.  _read_occupancy: any of the three destinations may be NULL, not all.  Argument errors are
 * reported before any HIP call. */
#define TDSA_DETECT_NAN_FLOOR 1
typedef struct tdsa_detect_row {
  float floor, thr;
  int32_t n_found, n_over, flags;
  int32_t reserved[3];
} tdsa_detect_row;
typedef struct tdsa_detect_signal {
  int32_t start, stop, peak_bin, x_lo, x_hi;   /* bins of the row, inclusive */
  float peak_db;
  double power, moment;                        /* linear; centroid = start + moment / power */
} tdsa_detect_signal;
typedef struct tdsa_detect_s* tdsa_detect;
int tdsa_detect_create(int device_id, int n_bins, size_t max_host_rows, tdsa_detect* out);
int tdsa_detect_destroy(tdsa_detect h);
int tdsa_detect_configure(tdsa_detect h, int bin_lo, int bin_hi, int rank, float margin_db, int min_width, int max_gap,
                          float xdb, int max_signals);
int tdsa_detect_process(tdsa_detect h, const float* rows_host, size_t n_rows, tdsa_detect_row* row_records_host,
                        tdsa_detect_signal* signal_records_host);
int tdsa_detect_process_dev(tdsa_detect h, tdsa_plan p, const float* rows_dev, size_t n_rows,
                            tdsa_detect_row* row_records_host, tdsa_detect_signal* signal_records_host);
int tdsa_detect_read_occupancy(tdsa_detect h, uint32_t* counts_host, uint64_t* rows_seen, uint64_t* rows_flagged);
int tdsa_detect_reset(tdsa_detect h);
int tdsa_detect_timer_begin(tdsa_detect h);
int tdsa_detect_timer_end(tdsa_detect h, float* elapsed_ms);

/* -------- channel measurements: power, ACPR, occupied bandwidth, x-dB width, limit mask ----
 * Rows are [n_rows][n_bins] float32 dB rows, 1 <= n_bins <= 16384, the input of tdsa_detect_*.  Throughout, p_i =
 * 10^(row[i] / 10) in float32 (tdsa_rows_stats' expression) widened to float64; a NaN bin contributes 0.  Per row:
 *   channels   C inclusive bin ranges lo_c <= hi_c (1 <= C <= 16, they may overlap; channel 0 is the main channel).  Per
 *              channel: power = sum p_i over the range in float64, by the tree of tdsa_detect_signal.power - a channel
 *              set to a detector record's [start, stop] has that record's power bits; peak_bin = the first bin holding
 *              the range's largest non-NaN value and peak_db that value (-1 and NaN if there is none); n_nan.
 *   obw        over [obw_lo, obw_hi]: S[k] = the inclusive prefix sum of p, T = its last value (obw_total), t_lo =
 *              T (1 - f) / 2, t_hi = T (1 + f) / 2; k_lo / k_hi = the first k with S[k] >= t_lo / t_hi; with a bin
 *              spanning [k - 1/2, k + 1/2], x = k - 1/2 + (t - S[k - 1]) / p_k, S[obw_lo - 1] = 0.  T not > 0 sets
 *              TDSA_MEAS_EMPTY, T = +inf TDSA_MEAS_INF: then k = -1 and x = NaN.  The order of the sums behind S depends
 *              on the bins and the configuration alone.  n_nan counts the range's NaNs.
 *   x-dB       peak_db / peak_bin of the same range as above; xdb_lo / xdb_hi = the first / last bin of the range with
 *              row[i] >= peak_db - xdb (float32); -1 where there is no peak.
 *   limit      with a limit line (tdsa_meas_set_limit; float32 [n_bins], a NaN entry = bin not tested): lim_i =
 *              limit[i] (absolute) or limit[i] + ref in float32 (relative; ref = channel 0's peak_db, a NaN ref tests
 *              nothing).  A bin fails when row[i] > lim_i (a NaN never does): n_fail, first_fail, last_fail.  margin_i
 *              = row[i] - lim_i in float32, NaN margins skipped: worst_margin = the largest, worst_bin = its first
 *              bin.  Nothing tested: the bins are -1, worst_margin NaN.  n_fail > 0 sets TDSA_MEAS_MASK_FAIL.
 * A row's records are the same bits whatever n_rows is, wherever the row sits, and whichever entry point or load path
 * ran it.  _configure fixes the parameters (a live handle may be configured again): 1 <= n_channels <= 16, every range
 * inside the row, 0 < fraction < 1, xdb finite and >= 0.  _set_limit uploads n = n_bins values (NULL removes the line)
 * and returns when limit_host may be released.  _process: host rows through pinned staging, n_rows <= max_host_rows.
 * _process_dev: rows in device memory (aligned to 4 bytes; 16-byte loads where n_bins % 4 == 0 and rows_dev is 16-byte
 * aligned, float loads otherwise, with the same results), on plan p's stream (ordered after its work, and its later
 * work after this) or on the handle's own for p = NULL.  Both write n_rows row records and n_rows * n_channels channel
 * records and return when they are in host memory; n_rows = 0 returns TDSA_OK and writes nothing.  The handle counts
 * the rows of all calls and those with TDSA_MEAS_MASK_FAIL since the last _reset (or create): _read_totals, either
 * destination may be NULL, not both.  Argument errors are reported before any HIP call. */
#define TDSA_MEAS_EMPTY 1
#define TDSA_MEAS_INF 2
#define TDSA_MEAS_MASK_FAIL 4
#define TDSA_MEAS_MAX_CHANNELS 16
typedef struct tdsa_meas_row {
  double obw_total, x_lo, x_hi;                 /* linear power; positions in bins */
  int32_t k_lo, k_hi, xdb_lo, xdb_hi, peak_bin, n_nan, n_fail, worst_bin, first_fail, last_fail, flags;
  float peak_db, worst_margin;
  int32_t reserved;
} tdsa_meas_row;
typedef struct tdsa_meas_channel {
  double power;                                 /* linear */
  float peak_db;
  int32_t peak_bin, n_nan, reserved;
} tdsa_meas_channel;
typedef struct tdsa_meas_s* tdsa_meas;
int tdsa_meas_create(int device_id, int n_bins, size_t max_host_rows, tdsa_meas* out);
int tdsa_meas_destroy(tdsa_meas h);
int tdsa_meas_configure(tdsa_meas h, int n_channels, const int* lo, const int* hi, int obw_lo, int obw_hi,
                        double fraction, float xdb);
int tdsa_meas_set_limit(tdsa_meas h, const float* limit_host, int n, int relative);
int tdsa_meas_process(tdsa_meas h, const float* rows_host, size_t n_rows, tdsa_meas_row* row_records_host,
                      tdsa_meas_channel* channel_records_host);
int tdsa_meas_process_dev(tdsa_meas h, tdsa_plan p, const float* rows_dev, size_t n_rows,
                          tdsa_meas_row* row_records_host, tdsa_meas_channel* channel_records_host);
int tdsa_meas_read_totals(tdsa_meas h, uint64_t* rows_seen, uint64_t* rows_failed);
int tdsa_meas_reset(tdsa_meas h);
int tdsa_meas_timer_begin(tdsa_meas h);
int tdsa_meas_timer_end(tdsa_meas h, float* elapsed_ms);

/* -------- power statistics of IQ streams: CCDF, PAPR, APD ---------------------------------
 * The statistics of the INSTANTANEOUS power of the samples, which no averaged or held trace carries.  A handle has C
 * streams, 1 <= C <= 256; stream c's samples of a call lie at in + c * in_stride, counted in samples of the call's
 * format (TDSA_IN_I8 / _U8 / _C64, unpacked as the down-converter does: I8 (I + jQ) / 128, U8 by the float32 of
 * float64(u) / 127.5 - 1).  Per sample p = fl(fl(re re) + fl(im im)) in float32: two products and one sum, each rounded
 * once, no fused multiply-add, denormals kept.  u = the 32 bits of p, E = u >> 23, F = u & 0x7fffff.
 * _configure(exp_lo, gate): -126 <= exp_lo <= 64 (default -40), gate a finite float32 >= 0 (0 = off, default).
 * Per stream, accumulated over all calls since the last _reset / _configure / _create, integers only.  A sample falls in
 * exactly one class, tested in this order:
 *   1  p is NaN                         n_nan
 *   2  p < gate (float32 compare)       n_gated   (a zero sample is gated whenever gate > 0)
 *   3  p = +inf                         n_inf     (also finite samples whose square overflows)
 *   4  p = 0                            n_zero
 *   5  b = (u >> 18) - ((exp_lo + 127) << 5):  b < 0 n_under, b >= 2048 n_over, else hist[b] += 1
 * hist: 2048 uint64 bins, 64 octaves of 32; bin b covers [edge_b, edge_(b+1)), edge_b = 2^(exp_lo + b / 32) * (1 +
 * (b % 32) / 32), every edge an exact float32, widths 0.068 .. 0.134 dB.  n_total = the samples seen = the sum of the six
 * counts and of hist.  msum: 256 uint64 words; every sample of class 5, inside the window or not, adds its mantissa (F |
 * 2^23 for E >= 1, F for E = 0) to msum[E], so the total power of the finite samples is exactly (msum[0] + sum over E >=
 * 1 of msum[E] 2^(E - 1)) 2^-149; a word holds 2^40 samples of one octave.  max_bits: the largest u among the samples of
 * classes 4 and 5 (finite, not gated), 0 if none; min_bits: the smallest u of class 5, 0xffffffff if none.  Integer adds,
 * max and min commute: the state is the same bits for any split of the input into calls, either entry point, any load
 * path.
 * _process: host samples through pinned staging, C * n_in <= max_host_samples; returns when they are consumed.
 * _process_dev: samples in device memory (aligned to one sample; a stream whose first sample lies on 16 bytes is read
 * with 16-byte loads, any other by elements), on plan p's stream (ordered after its work, and its later work after this)
 * or on the handle's own for p = NULL; it does NOT wait - the state stays on the device.  in_stride >= n_in when C > 1
 * (ignored for C = 1); n_in = 0 returns TDSA_OK and does nothing.  _read goes behind the last launch, waits, and copies
 * n_streams records from first_stream on, and where the pointers are not NULL their msum ([n_streams][256]) and hist
 * ([n_streams][2048]).  _reset zeroes the state and returns when earlier calls have finished; _configure does the same
 * and sets the parameters.  Argument errors are reported before any HIP call. */
#define TDSA_PSTAT_MAX_STREAMS 256
#define TDSA_PSTAT_BINS 2048
#define TDSA_PSTAT_BINS_PER_OCTAVE 32
#define TDSA_PSTAT_EXPONENTS 256
#define TDSA_PSTAT_EXP_LO_MIN (-126)
#define TDSA_PSTAT_EXP_LO_MAX 64
typedef struct tdsa_pstat_record {
  uint64_t n_total, n_nan, n_gated, n_inf, n_zero, n_under, n_over;
  uint32_t max_bits, min_bits;                  /* float32 bits */
  uint32_t reserved[2];
} tdsa_pstat_record;                            /* 72 bytes */
typedef struct tdsa_pstat_s* tdsa_pstat;
int tdsa_pstat_create(int device_id, int streams, size_t max_host_samples, tdsa_pstat* out);
int tdsa_pstat_destroy(tdsa_pstat h);
int tdsa_pstat_configure(tdsa_pstat h, int exp_lo, float gate);
int tdsa_pstat_reset(tdsa_pstat h);
int tdsa_pstat_process(tdsa_pstat h, int in_format, const void* in_host, size_t n_in, size_t in_stride);
int tdsa_pstat_process_dev(tdsa_pstat h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride);
int tdsa_pstat_read(tdsa_pstat h, int first_stream, int n_streams, tdsa_pstat_record* records_host, uint64_t* msum_host,
                    uint64_t* hist_host);
int tdsa_pstat_timer_begin(tdsa_pstat h);
int tdsa_pstat_timer_end(tdsa_pstat h, float* elapsed_ms);

/* -------- pulse analysis of IQ streams: one descriptor per pulse -----------------------------
 * The time-domain measurement of pulsed signals: per pulse its time of arrival, width, peak, energy and the lag-one
 * product that gives the carrier inside it; PRI / PRF, duty cycle and the rest follow on the host from the records.
 * Streams and samples.  A handle has C streams, 1 <= C <= 256; stream c's samples of a call lie at in + c * in_stride,
 *   counted in samples of the call's format (TDSA_IN_I8 / _U8 / _C64, unpacked as the power statistics do).  The
 *   samples of a stream count from the last _reset / _configure / _create across calls: n = 0, 1, ... (int64).
 * Power.  p = fl(fl(re re) + fl(im im)) in float32, no fused multiply-add, denormals kept: the power statistics' value
 *   bit for bit.
 * Class.  With float32 levels 0 < off_level <= on_level < inf:  A: p >= on_level.  B: p < off_level, or p is NaN.
 *   C: anything else.  A NaN also counts in n_nan.
 * State.  A stream is off after a reset.  A sets it on, B sets it off, C leaves it as it is: the state at n is the class
 *   of the last sample <= n that is not C.  The state survives between calls.
 * Pulse.  A maximal run of on samples: toa is its first index, width its length.  It is complete when a B sample
 *   follows it; a pulse still on at the end of a call stays open in the handle and completes in a later call.
 * Fields.  peak_bits: the largest float32 bits of p in the run (p >= off_level > 0 there, so bits order as values).
 *   peak_index: the first n that attains it.  energy: the float64 sum of p, each converted to float64 first.  acc_re,
 *   acc_im: the float64 sum over n = toa + 1 .. toa + width - 1 of x[n] conj(x[n-1]), per term re = fl64(re_n re_(n-1) +
 *   im_n im_(n-1)), im = fl64(im_n re_(n-1) - re_n im_(n-1)) with the products formed in float64, where they are exact;
 *   the pair (n-1, n) crosses tiles and calls like any other - the handle keeps each stream's last sample.  flags bit 0:
 *   the run holds a sample with p = +inf; then energy is +inf and acc_* is unspecified.
 * Filter and storage.  A complete pulse with width < min_width is dropped and counted in n_short.  Kept pulses get
 *   ordinals 0, 1, ... per stream in time order; ordinal k < capacity is stored at slot k, later ones are counted in
 *   n_lost; nothing is overwritten.
 * Summary, per stream: n_total; n_on, the samples in the on state before the width filter (duty cycle = n_on /
 *   n_total); n_pulses, the kept pulses, the lost ones included; n_short; n_lost; n_nan; open, open_toa, open_width of the
 *   pulse not yet complete (0 when the stream is off).
 * Split invariance.  toa, width, peak_index, peak_bits, flags, the summary and which pulses are stored are the same
 *   bits for any split of a stream into calls, any grid and any load path.  energy, acc_re and acc_im are float64 sums
 *   whose order of addition follows the split and the tiles (TDSA_PULSE_TILE samples, TDSA_PULSE_SAMPLES_PER_THREAD per
 *   thread): they agree with any other order within the rounding of width additions - |d energy| <= width 2^-52
 *   energy, |d acc| <= width 2^-50 energy - and no closer.
 * _create: 1 <= capacity, streams * capacity <= 2^22 records.  _configure(on_level, off_level, min_width), 1 <= min_width
 * < 2^31 (after _create: 1.0, 1.0, 1), zeroes the state and returns when earlier calls have finished, as _reset does.
 * _process: host samples through pinned staging, C * n_in <= max_host_samples; returns when they are consumed.
 * _process_dev: samples in device memory (aligned to one sample; a stream whose first sample lies on 16 bytes is read
 * with 16-byte loads, any other by elements), on plan p's stream (ordered after its work, and its later work after this)
 * or on the handle's own for p = NULL; it does NOT wait.  in_stride >= n_in when C > 1 (ignored for C = 1); n_in = 0
 * returns TDSA_OK and does nothing; a call of any length is cut into launches.  _read and _read_pulses go behind the
 * last launch and wait: _read copies n_streams summaries from first_stream on; _read_pulses copies the stored records
 * first .. first + count - 1 of one stream, as many as there are (*n_out).  _debug_limits is for the tests and
 * tools/pulsebench.py: fewer tiles (one workgroup each) per launch, so that small inputs take several, and a mask
 * of the three kernels to launch (7 = all; anything else leaves the state meaningless until the next _reset).
 * Argument errors are reported before any HIP call. */
#define TDSA_PULSE_MAX_STREAMS 256
#define TDSA_PULSE_MAX_RECORDS 4194304
#define TDSA_PULSE_TILE 4096
#define TDSA_PULSE_SAMPLES_PER_THREAD 16
#define TDSA_PULSE_FLAG_INF 1u
typedef struct tdsa_pulse_record {
  int64_t toa, width, peak_index;
  uint32_t peak_bits, flags;                    /* float32 bits; TDSA_PULSE_FLAG_* */
  double energy, acc_re, acc_im;
  uint64_t reserved;
} tdsa_pulse_record;                            /* 64 bytes */
typedef struct tdsa_pulse_summary {
  uint64_t n_total, n_on, n_pulses, n_short, n_lost, n_nan;
  int64_t open_toa, open_width;
  int32_t open, reserved;
} tdsa_pulse_summary;                           /* 72 bytes */
typedef struct tdsa_pulse_s* tdsa_pulse;
int tdsa_pulse_create(int device_id, int streams, int capacity, size_t max_host_samples, tdsa_pulse* out);
int tdsa_pulse_destroy(tdsa_pulse h);
int tdsa_pulse_configure(tdsa_pulse h, float on_level, float off_level, int64_t min_width);
int tdsa_pulse_reset(tdsa_pulse h);
int tdsa_pulse_process(tdsa_pulse h, int in_format, const void* in_host, size_t n_in, size_t in_stride);
int tdsa_pulse_process_dev(tdsa_pulse h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride);
int tdsa_pulse_read(tdsa_pulse h, int first_stream, int n_streams, tdsa_pulse_summary* summaries_host);
int tdsa_pulse_read_pulses(tdsa_pulse h, int stream, int first, int count, tdsa_pulse_record* records_host, int* n_out);
int tdsa_pulse_debug_limits(tdsa_pulse h, int max_launch_tiles, int passes);
int tdsa_pulse_timer_begin(tdsa_pulse h);
int tdsa_pulse_timer_end(tdsa_pulse h, float* elapsed_ms);

/* -------- correlation search of IQ streams: where a known sequence starts -------------------
 * A sliding, normalised cross-correlation of every stream against one reference r - a preamble, a sync word, a
 * Zadoff-Chu or Barker code, a radar's transmit pulse - and a peak search over it: one record per match.
 * Streams and samples.  A handle has C streams, 1 <= C <= 256; stream c's samples of a call lie at in + c * in_stride,
 *   counted in samples of the call's format (TDSA_IN_I8 / _U8 / _C64, unpacked as the power statistics and the pulse
 *   analysis do; the format may change from call to call).  The samples of a stream count from the last reset across
 *   calls: n = 0, 1, ... (int64).
 * Reference.  r[0 .. L-1] complex64, 2 <= L <= 1024, every component finite, E_r = sum |r[k]|^2 > 0 formed in float64
 *   and rounded once to float32 (it must stay finite and above 0).  H = floor(L / 2).  _set_reference resets the streams.
 * Window.  Window n is complete once sample n + L - 1 has arrived.  For every complete window, all in float32:
 *     c1[n] = sum_{k <  H} x[n+k] conj(r[k])        c2[n] = sum_{k >= H} x[n+k] conj(r[k])        c[n] = fl(c1 + c2)
 *     e[n]  = sum_k |x[n+k]|^2                       m[n] = fl(fl(fl(c_re^2) + fl(c_im^2)) / fl(E_r e[n]))
 *   If e[n] = 0, or a component of c1 or c2, or e, is not finite: m[n] = 0 and the window counts in n_bad.  An m that
 *   comes out as NaN (inf / inf, 0 / 0 after an overflow or underflow) is stored as the quiet NaN 0x7fc00000.
 * Order of the sums: ONE fixed order per window, wherever it lies in a tile, a launch, a call or a stride and whichever
 *   load path read it.  Every sum is a chain of fused multiply-adds from +0 in ascending k.  re(c1), re(c2): per k
 *   fma(x_re, r_re, .) then fma(x_im, r_im, .).  im(c1), im(c2): per k fma(x_im, r_re, .) then fma(x_re, -r_im, .).
 *   e = fl(a + b), a the chain of fma(x_re, x_re, .), b the chain of fma(x_im, x_im, .), each over all L samples.
 * Match.  With a float32 threshold, 0 < threshold <= 1, and min_distance W, 1 <= W <= 65536, window n is a match when
 *   m[n] >= threshold, m[n] > m[j] for every j in [max(0, n-W), n) and m[n] >= m[j] for every j in (n, n+W]: the first
 *   of equal maxima wins.  m is never negative, so the two comparisons with m[j] are those of the float32 bits as
 *   unsigned integers, in which a NaN ranks above +inf; a NaN window is never a match (m[n] >= threshold is false).
 *   The decision on n needs m up to n + W: the last W complete windows of a stream stay undecided in the handle,
 *   together with the L - 1 samples of history, until a later call brings their neighbours.
 * Flush.  _flush decides the undecided windows with the right-hand range clipped at the last complete window.  After
 *   it the streams take no samples until a reset: a process call returns TDSA_ERR_ARG with a text that says so.
 * Records, 32 bytes per match: index (= n), metric (= m[n]), energy (= e[n]), c1_re, c1_im, c2_re, c2_im.  Matches get
 *   ordinals 0, 1, ... in time order per stream; ordinal k < capacity is stored at slot k, the rest are counted in
 *   n_lost; nothing is overwritten.
 * Summary per stream: n_total samples, n_windows complete windows, n_decided of them decided, n_matches (the lost ones
 *   included), n_lost, n_bad, flushed.
 * Metric trace.  With trace = K > 0 at _create the handle keeps m and c of the most recent K complete windows of each
 *   stream on the device (K is lowered to 2^28 / (24 C) if above: the trace of all streams stays within 256 MiB).
 *   _read_trace(h, stream, first, count, m_out, c_out) copies windows first .. first + count - 1 to host memory
 *   (c_out: count complex64, may be NULL); a range that reaches outside [max(0, n_windows - K), n_windows) is
 *   TDSA_ERR_ARG.
 * Split invariance.  Every bit of the records, the summaries and the trace is the same for any split of the input into
 *   calls (empty calls included), either entry point, any launch cut, any stride and any alignment of the base.
 * Accuracy against exact arithmetic: a component of c1 or c2 within 2 (L + 1) 2^-24 A, A the sum of the absolute
 *   values of its real products; e within 2 (2 L + 1) 2^-24 e; m within what follows from the two plus 8 2^-24 m
 *   (tests/corr_contract.py derives it).  Twice the first-order bound for so many terms; the header promises no more.
 * _create(device, streams, capacity, trace, max_host_samples, ref, L, &h): 1 <= capacity, streams * capacity <= 2^22.
 * After it threshold = 1 and min_distance = L.  _configure(threshold, min_distance) and _set_reference reset the
 * streams and return when earlier calls have finished, as _reset does; the device memory of a handle grows with
 * min_distance: 24 bytes times the next power of two above 2 W + 2^21 / C + trace, per stream.
 * _process: host samples through pinned staging, C * n_in <= max_host_samples; returns when they are consumed.
 * _process_dev: samples in device memory, aligned to one sample, on plan p's stream (ordered after its work, and its
 * later work after this) or on the handle's own for p = NULL; it does NOT wait.  in_stride >= n_in when C > 1; n_in = 0
 * returns TDSA_OK and does nothing; a call of any length is cut into launches.  _read goes behind the last launch and
 * waits: n_streams summaries from first_stream on, and for each of them its `capacity` record slots (records_host:
 * n_streams * capacity records, may be NULL), of which the first min(n_matches, capacity) are valid.  _debug_limits is
 * for the tests and tools/corrbench.py: fewer tiles of TDSA_CORR_TILE windows per launch (at least `streams`), a mask
 * of the passes to launch (1 correlate, 2 block maxima and count, 4 scan, 8 emit; anything but 15 leaves the state
 * meaningless until the next reset) and a variant of the correlate pass (0 as shipped: 4 for L <= 128, else 6; 1 .. 5: 4,
 * 8, 16 windows per thread, then 4, 8 with packed fused multiply-adds, the reference through scalar loads; 6, 7: 8, then
 * 8 packed, the reference read from LDS: the same bits from all of them).  A process call that returns TDSA_ERR_HIP may
 * have enqueued some of its launches: the streams are then undefined until the next reset.  Argument errors are reported before any HIP call. */
#define TDSA_CORR_MAX_STREAMS 256
#define TDSA_CORR_MAX_RECORDS 4194304
#define TDSA_CORR_MIN_REF 2
#define TDSA_CORR_MAX_REF 1024
#define TDSA_CORR_MAX_DISTANCE 65536
#define TDSA_CORR_TILE 2048
#define TDSA_CORR_WINDOWS_PER_THREAD 8
#define TDSA_CORR_MAX_LAUNCH_TILES 1024
typedef struct tdsa_corr_record {
  int64_t index;
  float metric, energy;
  float c1_re, c1_im, c2_re, c2_im;
} tdsa_corr_record;                             /* 32 bytes */
typedef struct tdsa_corr_summary {
  uint64_t n_total, n_windows, n_decided, n_matches, n_lost, n_bad;
  int32_t flushed, reserved;
} tdsa_corr_summary;                            /* 56 bytes */
typedef struct tdsa_corr_s* tdsa_corr;
int tdsa_corr_create(int device_id, int streams, int capacity, int64_t trace, size_t max_host_samples, const void* ref_c64,
                     int ref_len, tdsa_corr* out);
int tdsa_corr_destroy(tdsa_corr h);
int tdsa_corr_set_reference(tdsa_corr h, const void* ref_c64, int ref_len);
int tdsa_corr_configure(tdsa_corr h, float threshold, int min_distance);
int tdsa_corr_reset(tdsa_corr h);
int tdsa_corr_process(tdsa_corr h, int in_format, const void* in_host, size_t n_in, size_t in_stride);
int tdsa_corr_process_dev(tdsa_corr h, tdsa_plan p, int in_format, const void* in_dev, size_t n_in, size_t in_stride);
int tdsa_corr_flush(tdsa_corr h);
int tdsa_corr_read(tdsa_corr h, int first_stream, int n_streams, tdsa_corr_record* records_host, tdsa_corr_summary* summaries_host);
int tdsa_corr_read_trace(tdsa_corr h, int stream, int64_t first, int64_t count, float* m_out, void* c_out_c64);
int tdsa_corr_debug_limits(tdsa_corr h, int max_launch_tiles, int passes, int variant);
int tdsa_corr_timer_begin(tdsa_corr h);
int tdsa_corr_timer_end(tdsa_corr h, float* elapsed_ms);

/* -------- stepped sweeps: one capture per tuning step, stitched into one trace --------------
 * What hackrf_sweep / rtl_power do per tuning step - capture, window, FFT, keep the clean middle, lay the steps side by
 * side - and what HackRFSweepDataSource._parse does with their output (datasources/hackrf_sweep.py:135-166: sort by
 * frequency, np.interp onto the fixed grid of _create_frequency_grid, :32-40), with the rows never leaving the device.
 * Geometry: n_steps centres c_s (float64 Hz, strictly ascending), one frame length nfft, one bin width bin_hz, one
 * kept range [k0, k1) of the fftshift-ed row (K = k1 - k0).  Kept bin k of step s lies at x = c_s + (k - nfft/2) *
 * bin_hz, one float64 multiply then one float64 add (with bin_hz = 1.0 / (nfft * (1.0 / fs)) that is
 * np.fft.fftshift(np.fft.fftfreq(nfft, 1 / fs)) + c_s bit for bit).  The concatenation xp of the steps' frequencies
 * must be strictly increasing - x_last(s) < x_first(s + 1), checked with that expression, TDSA_ERR_ARG otherwise; gaps
 * between steps are allowed and interpolated across.  _set_geometry also takes the grid (n_grid finite float64 values),
 * waits for the handle's work in flight and clears the steps.
 * Detector: the F dB rows of a step become T[s][k - k0] (float32): _SAMPLE the last frame, _MAX / _MIN np.max / np.min
 * over the frames (a NaN stays), _AVG 10 log10(max(mean_f(10^(d_f / 10)), 1e-30)) with the sum in float64 in frame
 * order (display_data_processor.py:400-402; -inf counts as no power, a NaN stays; rows within +-300 dB; exp2 / log2
 * in float32, within 1e-3 dB of the float64 formula).
 * _update_dev: rows of steps [first_step, first_step + n_steps) already on the device, step i at rows_dev + i *
 * step_stride_floats (0: back to back, frames_per_step * nfft), its frames nfft apart; those steps become present.
 * On plan p's stream, after its work (p = NULL: the handle's own stream); no host wait.
 * _run_dev: the same from raw IQ: tdsa_process_dev_batch of plan p (one capture per step, step i at iq_dev + i *
 * step_stride_bytes) into a row scratch the handle owns, then the detector, chunk of steps by chunk of steps so that
 * the scratch stays within the bound of _set_chunk_bytes (default 256 MiB, at least one step); no host wait.  Any
 * split into calls and any bound give the same bits.
 * _read: stitches the steps present onto the grid, float64 [n_grid], to out_f64_dev and / or out_f64_host (either may
 * be NULL; with a host pointer the call waits, otherwise the next _read with one, _get_steps or _timer_end does).
 * TDSA_SWEEP_INTERP: np.interp(grid, xp, fp) bit for bit, fp = T as float64.  TDSA_SWEEP_PEAK, for grids coarser than
 * the bins: with h = grid[1] - grid[0] (> 0), out[i] = the maximum of fp over the bins with grid[i] - 0.5 h <= xp <
 * grid[i] + 0.5 h (a NaN stays; one lane walks one cell), an empty cell takes the INTERP value.  With no step present
 * every output is NaN (the reference before its first sweep).  _reset: no step is present.  _get_steps: T [n_steps][K]
 * and one byte per step (1 = present) to the host, for tests and tools.  _timer_begin / _end: HIP events on the
 * handle's own stream (where _read runs); both first put that stream behind the handle's last launch, so updates that
 * went on a plan's stream before _timer_end are inside the interval, as with the zero span and history timers.
 * Limits: n_steps <= 4096, 2 <= nfft <= 2^20, 1 <= K <= nfft, 2 <= n_grid <= 2^24, frames_per_step >= 1.  Argument
 * errors are reported before any HIP call. */
#define TDSA_SWEEP_DET_SAMPLE 0
#define TDSA_SWEEP_DET_MAX 1
#define TDSA_SWEEP_DET_MIN 2
#define TDSA_SWEEP_DET_AVG 3
#define TDSA_SWEEP_INTERP 0
#define TDSA_SWEEP_PEAK 1
typedef struct tdsa_sweep_s* tdsa_sweep;
int tdsa_sweep_create(int device_id, int nfft, int n_steps, int n_grid, tdsa_sweep* out);
int tdsa_sweep_destroy(tdsa_sweep w);
int tdsa_sweep_set_geometry(tdsa_sweep w, const double* centres_hz, double bin_hz, int k0, int k1,
                            const double* grid_hz_host);
int tdsa_sweep_reset(tdsa_sweep w);
int tdsa_sweep_set_chunk_bytes(tdsa_sweep w, size_t bytes);
int tdsa_sweep_update_dev(tdsa_sweep w, tdsa_plan p, int first_step, int n_steps, const float* rows_dev,
                          int frames_per_step, size_t step_stride_floats, int detector);
int tdsa_sweep_run_dev(tdsa_sweep w, tdsa_plan p, int in_format, const void* iq_dev, size_t step_stride_bytes,
                       int first_step, int n_steps, size_t n_samples_per_step, int hop, int frames_per_step,
                       int detector);
int tdsa_sweep_read(tdsa_sweep w, int mode, double* out_f64_host, double* out_f64_dev);
int tdsa_sweep_get_steps(tdsa_sweep w, float* T_host, unsigned char* valid_host);
int tdsa_sweep_timer_begin(tdsa_sweep w);
int tdsa_sweep_timer_end(tdsa_sweep w, float* elapsed_ms);

/* -------- zero span: detector ring, trigger search, trace view ---------------------------
 * Amplitude against time.  Samples count from the last reset, n = 0, 1, ...; x[n] is the unpacked sample (TDSA_IN_I8:
 * (I + jQ) / 128; _U8: (float(u) - 127.5f) * (1.0f / 127.5f) per component, the frame kernels' unpack; _C64 as is;
 * TDSA_IN_F32R, real float32, is accepted by tdsa_zspan_push* alone).  The detector gives one float32 e[n] per sample:
 * _DET_REAL e = Re x (F32R passes through); _DET_MAG e = sqrt(re * re + im * im), every operation rounded to float32,
 * the root correctly; _DET_DB e = log2(re * re + im * im + log_floor) * float32(10 / log2(10)) + offset_db, within
 * 1e-3 dB of the float64 formula.
 * Ring: the last `capacity` values of e.  With `total` samples pushed, held = min(total, capacity), base = total -
 * held; a push of more than `capacity` samples only processes its last `capacity`; any split of a stream into pushes
 * gives the same ring.
 * _create: capacity is int(2.0 * rate) for the reference's _ZS_BUFFER_SECONDS (core/display_data_processor.py:275,
 * :277-282 - the np.concatenate and the [-max_buf:] slice of every tick).  _set_detector resets (the ring holds
 * detected values); _reset empties the ring (DisplayManager._set_zero_span / _exit_zero_span writing None, core/display_manager.py:541, :553).
 * _push: one host block through pinned staging in chunks of max_host_samples; it returns when the block has left the
 * caller's memory, not when the ring is written (:264-272: read_samples_only, stereo mean and .real stay with the
 * caller; the history append is this call).  _push_dev: samples already on the device; on plan p's stream after its
 * work (p = NULL: the handle's own stream); no host wait.
 * _view (:284-311): level is rounded to float32 first, since the reference compares a float32 array with a Python
 * float and numpy does that in float32.  held < n_display: the chunk is everything held, untriggered.  _FREE_RUN:
 * start = total - n_display.  _RISE / _FALL: se = held - n_display, ss = max(0, se - 8 * n_display); over the
 * ring-relative pairs (i, i + 1), ss <= i <= se - 2, a rise is e[i] < level && e[i + 1] >= level, a fall e[i] >= level
 * && e[i + 1] < level (a NaN never matches); the last hit gives start = base + i + 1, triggered = 1; no hit or an
 * empty range gives the free-run start, triggered = 0.  The chunk is e[start : start + length].  n_points = 0: the
 * chunk itself, float32 [length].  Otherwise P = min(n_points, length) columns; column c covers chunk indices
 * [floor(c L / P), floor((c + 1) L / P)): _COL_MINMAX two rows [2][P], np.min then np.max of the cell (a NaN stays -
 * what the widget's peak-downsampled curve draws, displays/zero_span.py:55); _COL_SAMPLE the cell's first value;
 * _COL_MEAN its float64 sum divided by its length, rounded once.  The output goes to out_dev and / or out_host (either
 * may be NULL; room for max(n_display, 1) floats with n_points = 0, for 2 * n_points otherwise).  Every view fills
 * *info and waits once for the device.  Statistics are over the chunk: min / max as np.min / np.max, mean from a
 * float64 sum, n_at_or_above counts e >= level (duty cycle = that / length), n_rise / n_fall the crossings inside the
 * chunk (pulse count, PRF).  An empty chunk has NaN min / max / mean.
 * _timer_begin / _end: HIP events on the handle's own stream (where _view runs, behind the pushes).
 * Limits: 4 <= capacity <= 2^28, 1 <= n_display <= 2^28, 0 <= n_points <= 16384.  Argument errors are reported before
 * any HIP call. */
#define TDSA_IN_F32R 3
#define TDSA_ZS_DET_REAL 0
#define TDSA_ZS_DET_MAG 1
#define TDSA_ZS_DET_DB 2
#define TDSA_ZS_FREE_RUN 0
#define TDSA_ZS_RISE 1
#define TDSA_ZS_FALL 2
#define TDSA_ZS_COL_MINMAX 0
#define TDSA_ZS_COL_SAMPLE 1
#define TDSA_ZS_COL_MEAN 2
typedef struct tdsa_zspan_info {
  int64_t start, total;      /* absolute index of the chunk's first sample; samples pushed since the last reset */
  int32_t length, triggered, n_columns;
  float min, max;
  double mean;
  int64_t n_at_or_above;
  int32_t n_rise, n_fall;
} tdsa_zspan_info;
typedef struct tdsa_zspan_s* tdsa_zspan;
int tdsa_zspan_create(int device_id, size_t capacity, size_t max_host_samples, tdsa_zspan* out);
int tdsa_zspan_destroy(tdsa_zspan z);
int tdsa_zspan_set_detector(tdsa_zspan z, int detector, float log_floor, float offset_db);
int tdsa_zspan_reset(tdsa_zspan z);
int tdsa_zspan_push(tdsa_zspan z, int in_format, const void* samples_host, size_t n);
int tdsa_zspan_push_dev(tdsa_zspan z, tdsa_plan p, int in_format, const void* samples_dev, size_t n);
int tdsa_zspan_view(tdsa_zspan z, int mode, double level, size_t n_display, int n_points, int col_detector,
                    tdsa_zspan_info* info, float* out_host, float* out_dev);
int tdsa_zspan_timer_begin(tdsa_zspan z);
int tdsa_zspan_timer_end(tdsa_zspan z, float* elapsed_ms);

/* -------- 3-D history views: trace ring, ribbon / line-stack / surface passes -------------
 * The device side of the reference's ThreeD, RibbonWidget and Surface displays (displays/three_dimension.py, ribbon.py,
 * surface.py): a ring [depth][n_bins] of the last rows, a running hold row, and view passes that return what the three
 * widgets hand their GL items, newest row first.  kind TDSA_HIST_HEIGHTS stores z = clip((dB - (ref - range)) / range
 * * 8, 0, 8), every operation in float32 with the amplitude in force at the push (rows already held keep their z);
 * TDSA_HIST_LEVELS stores the rows as pushed and normalises at view time.  Rows never pushed are 0.  Rows are float32
 * without NaN (+-inf are fine); n_bins >= 2, depth * n_bins <= 2^28, range_db > 0 for heights.
 *
 * push: one host row, optionally with the max trace the hold follows (hold = maximum(hold, z(max)); without it the
 * hold follows the row itself) and the min trace (kept as z(min) until the next push); update_hold = 0 leaves the hold
 * alone.  push_dev: n_rows device rows in order, on the plan's stream (NULL: the handle's own), the same as n_rows
 * single pushes.  Each push also keeps the row's maximum and the index of its first occurrence (np.argmax).
 *
 * Views.  columns = 0: every bin; columns = P: column c covers bins [(c n) / P, ((c + 1) n) / P) and yields the cell's
 * maximum and the bin of its first maximum (out->bins, [rows][P]); colours follow the reduced value.  Destinations
 * (tdsa_history_out) are all host or all device pointers (on_device; device ones aligned to 16 bytes); NULL = not
 * wanted.  Every view waits for its results.
 *   ribbon   rows 0 .. min(30, depth) - 1; primary = vertices float32 [rows][2 n][3] (x from x_host[n_bins], gathered
 *            through the bins of a reduced view), colours = RGBA float32 [rows][2 n][4]  (Ribbon._row_verts_colors)
 *   lines    lines first .. first + count - 1; primary = z float32 [count][n]; colours = uint8 [count][n], int32(8 - z)
 *            % 11, 255 for a line no row has reached (TDSA_HIST_COLOUR_INDEX), or float32 [count][n][4] through
 *            palette_host [11][4] (TDSA_HIST_COLOUR_RGBA; 255 -> 0); hold, min_row: float32 [n] (+ hold_bins, min_bins
 *            when reduced); info: live and hold peak
 *   surface  all depth rows; primary = float32(clip((level - zmin) / (zmax - zmin), 0, 1)) evaluated in float64, 0.5
 *            when zmax == zmin; colours = float32 [depth][n][3] = (t, 0, 1 - t); info: live peak and live_norm */
#define TDSA_HIST_HEIGHTS 0
#define TDSA_HIST_LEVELS 1
#define TDSA_HIST_COLOUR_INDEX 0
#define TDSA_HIST_COLOUR_RGBA 1
typedef struct tdsa_history_info {
  long long pushed;        /* rows since the last reset */
  int rows, cols;          /* rows and columns of the arrays written */
  int valid_rows, has_min; /* rows of the view a push has reached; 1: min_row was written */
  int live_bin;            /* first maximum of the newest row (full-width bin) ... */
  float live_value;        /* ... and its z / level */
  int hold_bin;            /* lines: first maximum of the hold row */
  float hold_value;
  double live_norm;        /* surface: normalised z of the live peak, evaluated in float32 as the widget's marker is */
} tdsa_history_info;
typedef struct tdsa_history_out {
  int on_device, reserved;
  void* primary;
  void* colours;
  int* bins;
  float* hold;
  int* hold_bins;
  float* min_row;
  int* min_bins;
} tdsa_history_out;
typedef struct tdsa_history_s* tdsa_history;
int tdsa_history_create(int device_id, int depth, int n_bins, int kind, tdsa_history* out);
int tdsa_history_destroy(tdsa_history h);
int tdsa_history_set_amplitude(tdsa_history h, double ref_level, double range_db);
int tdsa_history_reset(tdsa_history h);
int tdsa_history_reset_hold(tdsa_history h);
int tdsa_history_push(tdsa_history h, const float* live_host, const float* max_host, const float* min_host,
                      int update_hold);
int tdsa_history_push_dev(tdsa_history h, tdsa_plan p, const float* rows_dev, int n_rows);
int tdsa_history_ribbon(tdsa_history h, const float* x_host, int columns, const tdsa_history_out* out,
                        tdsa_history_info* info);
int tdsa_history_lines(tdsa_history h, int first, int count, int colour_mode, const float* palette_host, int columns,
                       const tdsa_history_out* out, tdsa_history_info* info);
int tdsa_history_surface(tdsa_history h, int columns, const tdsa_history_out* out, tdsa_history_info* info);
int tdsa_history_timer_begin(tdsa_history h);
int tdsa_history_timer_end(tdsa_history h, float* elapsed_ms);

typedef struct tdsa_waterfall_s* tdsa_waterfall;
int tdsa_waterfall_create(int device_id, int history_lines, int n_bins, float min_db, tdsa_waterfall* out);
int tdsa_waterfall_destroy(tdsa_waterfall w);
int tdsa_waterfall_push_dev(tdsa_waterfall w, tdsa_plan p, const float* rows_dev, int n_rows, int* n_new);
int tdsa_waterfall_push(tdsa_waterfall w, const float* row_host, int n, int* is_new);
int tdsa_waterfall_view(tdsa_waterfall w, float* view_host, int* ptr);
/* _display_view() as ImageItem.setImage(img, autoLevels=False, levels=(wf_min_db, wf_max_db)) quantises it
 * (displays/waterfall.py:353-356): uint8 [history][n_bins], np.clip((view - min_db) / (max_db - min_db) * 255, 0, 255)
 * truncated, float32 arithmetic; a NaN pixel -> 0. */
int tdsa_waterfall_view_u8(tdsa_waterfall w, float min_db, float max_db, uint8_t* view_host);

/* -------- host pipeline: pinned ring + asynchronous copy / compute / read-back legs -------------
 * Batch counterpart of the reader-thread -> queue.Queue(4) -> get_power_levels() front end
 * (datasources/hackrf_samples.py:54,102-107,191-305).  The producer writes IQ
 * straight into a pinned slot (tdsa_pipe_acquire), tdsa_pipe_submit enqueues H2D -> frame kernel ->
 * D2H on three streams and returns at once, tdsa_pipe_collect waits for the OLDEST submitted slot and
 * hands back its dB rows (pinned, valid until that slot is acquired again).  Slots complete in
 * submission order; plan state (hold traces, averager, DC tracker) advances exactly as if
 * tdsa_process_i8 had been called per slot.  want_rows: 0 keeps only the plan state (hold / Welch
 * traces); 1 reads the dB rows back into pinned host memory (tdsa_pipe_collect); 2 keeps them in the
 * slot's device buffer for the analytics / accumulators below (tdsa_pipe_collect_dev hands out the device
 * pointer, valid until that slot is acquired again) and skips the read-back leg; 3 reads them back as
 * uint8 [n_frames][nfft] - what ImageItem.setImage(rows, levels=(min_db, max_db)) makes of them before the
 * colour table (displays/waterfall.py:353-356: float32 (v - lo) / (hi - lo) * 255, clipped, truncated; NaN -> 0;
 * levels from tdsa_pipe_set_levels, (-120, 0) until it is called, applied to slots submitted afterwards):
 * a quarter of the bytes over PCIe, which is what bounds a pipe that returns rows (tdsa_pipe_collect_u8; the
 * float32 rows of the slot stay on the device, tdsa_pipe_collect_dev hands them out as well).  One thread
 * drives a pipe; destroy it before its plan. */
typedef struct tdsa_pipe_s* tdsa_pipe;
int tdsa_pipe_create(tdsa_plan p, int in_format, size_t slot_samples, int n_slots, int want_rows, tdsa_pipe* out);
int tdsa_pipe_destroy(tdsa_pipe q);
int tdsa_pipe_acquire(tdsa_pipe q, void** host_slot);
int tdsa_pipe_submit(tdsa_pipe q, size_t n_samples, int hop, int n_frames);
int tdsa_pipe_collect(tdsa_pipe q, const float** rows_host, int* n_frames);
int tdsa_pipe_collect_dev(tdsa_pipe q, const float** rows_dev, int* n_frames);
int tdsa_pipe_collect_u8(tdsa_pipe q, const uint8_t** rows_host, int* n_frames);
int tdsa_pipe_set_levels(tdsa_pipe q, float min_db, float max_db);
int tdsa_pipe_pending(tdsa_pipe q, int* pending);

/* A trace object owns the per-bin state the reference keeps in numpy arrays on MainWindow /
 * DisplayManager / TraceAverager for ONE displayed trace of n bins (any n >= 1, not tied to an FFT
 * plan): hold traces (mw.max_power_levels / mw.min_power_levels, main.py:70-105), the tare
 * accumulator + baseline (core/tare_state.py:9-13, mw.baseline_power_levels) and a TraceAverager
 * buffer (utils/signal_processing.py:16-17). */
typedef struct tdsa_trace_s* tdsa_trace;
int tdsa_trace_create(int device_id, int n, tdsa_trace* out);
int tdsa_trace_destroy(tdsa_trace t);
int tdsa_trace_reset(tdsa_trace t, uint32_t what); /* TDSA_RESET_* bits */

/* One displayed frame: db_in (n float32 dB values from ANY SampleDataSource) -> +cal offset ->
 * tare (collect / subtract) -> live; max/min hold updated.  Replaces _apply_cal_offset (:317-327),
 * _apply_tare (:329-369), _update_max_hold (:371-382), _update_min_hold (:384-395) of
 * core/display_data_processor.py in one launch.
 * tare_collect != 0: this frame is accumulated into the tare buffer (10^(dB/10)); when
 * tare_total frames have been collected the baseline becomes active (reported in *tare_done) and
 * is subtracted from this very frame, as the reference does.  tare_subtract != 0: subtract the
 * active baseline.  live_out/max_out/min_out may be NULL. */
int tdsa_trace_update(tdsa_trace t, const float* db_in_host, int n, float cal_offset_db,
                      int tare_collect, int tare_total, int tare_subtract, uint32_t hold_flags,
                      float* live_out, float* max_out, float* min_out, int* tare_done);
int tdsa_trace_get_tare_baseline(tdsa_trace t, float* baseline_db_host, int* active);
int tdsa_trace_set_tare_baseline(tdsa_trace t, const float* baseline_db_host, int n);

/* TraceAverager on host rows of linear power (utils/signal_processing.py:19-61); also used for the
 * sweep averager DataProcessor owns (display_data_processor.py:41,217-221).  set_mode resets. */
int tdsa_trace_avg_set_mode(tdsa_trace t, int avg_mode, int avg_n);
int tdsa_trace_avg_process(tdsa_trace t, const double* linear_in_host, int n, double* avg_out_host,
                           int* count_out);

/* ---- helpers for callers without their own device allocator -------------------------------- */
int tdsa_dev_alloc(int device_id, size_t bytes, void** out_dev);
int tdsa_dev_free(int device_id, void* dev);
int tdsa_memcpy_h2d(int device_id, void* dst_dev, const void* src_host, size_t bytes);
int tdsa_memcpy_d2h(int device_id, void* dst_host, const void* src_dev, size_t bytes);

/* HIP-event timer on the plan's stream (bench.py: kernel time on the stream the kernels run on). */
int tdsa_timer_begin(tdsa_plan p);
int tdsa_timer_end(tdsa_plan p, float* elapsed_ms); /* records, synchronises, returns elapsed */

/* Per-launch HIP-event bracketing of the frame kernel alone (the dominant kernel bench.py prices
 * against the HBM roofline).  enable != 0 starts collecting; read synchronises the stream and returns
 * the number of frame-kernel launches and the sum of their durations since the last read. */
int tdsa_profile_enable(tdsa_plan p, int enable);
int tdsa_profile_read(tdsa_plan p, int* launches, float* total_ms);

/* ---- developer section (no reference counterpart; used by tools/ and tests/ only) ---------------------- */
/* Plan parameters the tools and tests move to reach code paths that otherwise need other hardware or very long
 * batches (the library reads nothing from the environment): "num_cu" (persistent grids sized for fewer CUs),
 * "avg_wg_min" (batches of more frames take the workgroup-chunk averager scan), "avg_f64_chunks" (1: always the scan
 * over fixed 64-frame chunks with float64 aggregates), "overlap_share" (percent of the CUs an overlapped launch is
 * sized for), "big_group" (long-frame plans: segments per column / row round, 1 .. 64), "chirp_single" (chirp-z plans:
 * 0 = the passes of the convolution as separate kernels instead of one launch), "smooth" (frame lengths 2^a 3^b 5^c: 0 = as a chirp-z convolution like every other size that is not a
 * power of two, instead of the mixed-radix transform), "smooth_n1" (such sizes above 10 000 points: the column pass's length of the two-pass transform, a divisor with both factors
 * <= 10 000), "chirp_fuse_big" (chirp-z plans with
 * M > 16384: 0 = the unpack / window / chirp and the power / dB passes as kernels of their own), "big_fuse_gather"
 * (long-frame Welch captures of one round: 1 = row pass + gather + finish as ONE launch with a dependency-counted ticket
 * queue instead of two launches - same bits, measured slower, profiles/r06_c5_fused_gather.txt; default 0) and
 * "big_queue_gave_up" (reads: an error if a workgroup of such a launch ever gave up waiting); a library built with
 * -DTDSA_DEV also knows "big_pre_wgs" (empty workgroups ahead of every column pass: tools/c5_xcd_phase.py) and "cu_mask"
 * (the plan's stream confined to a set of CUs: tools/c5_two_plans.py).
 * Unknown names are an error. */
int tdsa_debug_knob(tdsa_plan p, const char* name, int value);
/* Phase timeline of workgroup 0 of the frame kernel: allocates the plan's stamp buffer on first call;
 * host_out_2048 != NULL copies 2048 s_memtime stamps back.  Stamps are only written by a library built
 * with -DTDSA_TIMELINE (tools/timeline.py); a production build leaves them zero. */
int tdsa_debug_timeline(tdsa_plan p, unsigned long long* host_out_2048);

#ifdef __cplusplus
}
#endif
#endif /* TDSA_HIP_H */
