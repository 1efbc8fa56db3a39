// tdsa_capi_chirp.cpp - plans whose frame length is not a power of two: chirp-z convolutions (tdsa_chirp.hip) and the
// mixed-radix transforms of the sizes made of 2, 3, 5 (tdsa_smooth.hip) - their tables and their processing path.
#include "tdsa_capi_internal.hpp"

using namespace tdsa;

namespace tdsa {

// n = 2^a 3^b 5^c: the radices of its stages (4 while it divides, then 2, 3, 5); 0 stages: other factors
int smooth_radices(int n, int* radix) {
  int r = n, st = 0;
  while (r % 4 == 0 && st < kSmoothMaxStages) { radix[st++] = 4; r /= 4; }
  for (const int f : {2, 3, 5})
    while (r % f == 0 && st < kSmoothMaxStages) { radix[st++] = f; r /= f; }
  return r == 1 ? st : 0;
}
static void smooth_plan(tdsa_plan p) {
  if (p->nfft <= kSmoothMaxN) {
    p->smooth_stages = smooth_radices(p->nfft, p->smooth_radix);
    return;
  }
  // two passes, both factors within the LDS limit; the column pass's length n1 near 128 measured best (N = 10^6: 309 us
  // per ten frames at 125 x 8000 against 389 at 1000 x 1000; N = 20 000: 185 at 125 x 160 against 254 at 2 x 10 000 -
  // short columns let a workgroup take sixteen adjacent ones, whose raw samples then sit side by side)
  int best = 0;
  double best_d = 1e30;
  for (int d = 2; d <= kSmoothMaxN && d <= p->nfft / 2; ++d)
    if (p->nfft % d == 0 && p->nfft / d <= kSmoothMaxN) {
      const double dist = std::fabs(std::log(double(d) / 128.0));
      if (dist < best_d) { best_d = dist; best = d; }
    }
  if (best == 0) return;
  p->smooth_n1 = best;
  p->smooth_n2 = p->nfft / best;
  p->smooth_stages = smooth_radices(p->smooth_n1, p->smooth_radix);
  p->smooth_stages2 = smooth_radices(p->smooth_n2, p->smooth_radix2);
  if (p->smooth_stages == 0 || p->smooth_stages2 == 0) p->smooth_stages = p->smooth_stages2 = p->smooth_n1 = p->smooth_n2 = 0;
}

// plan_init's part for these plans: the chirp a[n], the filter spectra, the mixed-radix stages, the seeds of the long
// transforms
int chirp_plan_init(tdsa_plan p) {
  const int nfft = p->nfft;
  // a[n] = exp(-i pi n^2 / N): the phase from n^2 mod 2N in integers, so that it is exact for every n;
  // B = FFT_M(b), b[n] = b[M - n] = conj(a[n]) for n < N, 0 elsewhere - in double (plain radix-2), rounded once
  const int M = p->m_fft;
  std::vector<double> ar(nfft), ai(nfft), br(M, 0.0), bi(M, 0.0);
  for (int n = 0; n < nfft; ++n) {
    const long long q = ((long long)n * n) % (2ll * nfft);
    const double ang = -M_PI * double(q) / double(nfft);
    ar[n] = std::cos(ang);
    ai[n] = std::sin(ang);
  }
  std::vector<double> twc(M / 2), tws(M / 2);      // exp(-2 pi i k / M), k < M / 2: one table for every stage
  for (int k = 0; k < M / 2; ++k) {
    const double ang = -2.0 * M_PI * double(k) / double(M);
    twc[k] = std::cos(ang);
    tws[k] = std::sin(ang);
  }
  // FFT_M, in double, of the filter segment  h[m mod M] = b[m + shift] = conj(a[|m + shift|])  for lo <= m <= hi, 0 elsewhere
  const auto filter_spectrum = [&](int shift, int lo, int hi) {
    std::fill(br.begin(), br.end(), 0.0);
    std::fill(bi.begin(), bi.end(), 0.0);
    for (int mm = lo; mm <= hi; ++mm) {
      const int idx = mm + shift < 0 ? -(mm + shift) : mm + shift;
      const int pos = mm < 0 ? M + mm : mm;
      br[pos] = ar[idx];
      bi[pos] = -ai[idx];
    }
    for (int i = 1, j = 0; i < M; ++i) {        // bit reversal
      int bit = M >> 1;
      for (; j & bit; bit >>= 1) j ^= bit;
      j ^= bit;
      if (i < j) { std::swap(br[i], br[j]); std::swap(bi[i], bi[j]); }
    }
    for (int len = 2; len <= M; len <<= 1) {
      const int step = M / len;
      for (int i = 0; i < M; i += len) {
        for (int k = 0; k < len / 2; ++k) {
          const double wr = twc[k * step], wi = tws[k * step];
          const double xr = br[i + k + len / 2] * wr - bi[i + k + len / 2] * wi;
          const double xi = br[i + k + len / 2] * wi + bi[i + k + len / 2] * wr;
          br[i + k + len / 2] = br[i + k] - xr;
          bi[i + k + len / 2] = bi[i + k] - xi;
          br[i + k] += xr;
          bi[i + k] += xi;
        }
      }
    }
  };
  // ... rounded once, in the order the first transform leaves its bins in ([k1][k2] on the long-frame kernels)
  const auto upload_spectrum = [&](Dev<float2>& dst) -> int {
    std::vector<float2> b32(M);
    if (p->chirp_big) {
      const int n1 = M >> kMaxLog2N, n2 = 1 << kMaxLog2N;
      for (int k1 = 0; k1 < n1; ++k1)
        for (int k2 = 0; k2 < n2; ++k2) b32[size_t(k1) * n2 + k2] = float2{float(br[k1 + n1 * k2]), float(bi[k1 + n1 * k2])};
    } else {
      for (int k = 0; k < M; ++k) b32[k] = float2{float(br[k]), float(bi[k])};
    }
    return upload(b32, dst);
  };
  const int H = p->chirp_split;
  if (H == 0) {
    filter_spectrum(0, -(nfft - 1), nfft - 1);           // b[n] = b[M - n] = conj(a[n]) for n < N
    TRY(upload_spectrum(p->d_chirp_b));
  } else {                                               // (tdsa_chirp.hip: the three segments of the split convolution)
    filter_spectrum(0, -(H - 1), H - 1);
    TRY(upload_spectrum(p->d_chirp_b));
    filter_spectrum(-H, -(nfft - H - 1), H - 1);         // b[m - H], m = k - n' in (-(N - H), H)
    TRY(upload_spectrum(p->d_chirp_bm));
    filter_spectrum(H, -(H - 1), nfft - H - 1);          // b[m + H], m = k' - n in (-H, N - H)
    TRY(upload_spectrum(p->d_chirp_bp));
  }
  std::vector<float2> a32(nfft);
  for (int n = 0; n < nfft; ++n) a32[n] = float2{float(ar[n]), float(ai[n])};
  TRY(upload(a32, p->d_chirp_a));
  TRY(upload(std::vector<float>(M, 1.0f), p->d_ones));
  {   // 2^a 3^b 5^c up to 10 000 points: the stages of its mixed-radix transform and W_N^k
    int r = nfft;
    for (const int f : {2, 3, 5}) while (r % f == 0) r /= f;
    if (r == 1 && nfft >= 4) {
      smooth_plan(p);
      p->smooth = p->smooth_stages > 0;
    }
    if (p->smooth) TRY(upload(unit_circle(nfft), p->d_smooth_tw));
  }
  // the M-point transforms' column-pass seeds (as for a native long frame of M points)
  if (p->chirp_big) TRY(upload(seed_table(M, p->log2m), p->d_tw_seed));
  return TDSA_OK;
}

// Chirp-z core of a plan whose frame length is not a power of two: frames at `in` (stride bytes apart) ->
// p->d_u0[f][k] = M * conj(convolution), k < nfft (tdsa_chirp.hip steps 1-3), on the main stream.
// the transforms can carry the element-wise passes: M <= 16384 and frames made of whole waves (the fused instantiations
// address their rows through wave-uniform descriptors)
// (M > 16384: the column passes of tdsa_big.hip carry them instead, BigChirpPre / BigChirpPost)
#ifdef TDSA_DEV
constexpr bool kChirpTwoLaunches = true;    // spectrum_kernel<L, true, 0, 1 | 2>: each transform carries one element-wise pass
#else
constexpr bool kChirpTwoLaunches = false;   // shipped: one launch, or (tdsa_debug_knob chirp_single 0) the passes as kernels of their own
#endif
static bool chirp_fusable(tdsa_plan p) {
  if (!p->chirp || p->log2m < 10) return false;
  return p->chirp_big ? p->chirp_fuse_big != 0 : (p->chirp_single != 0 || kChirpTwoLaunches);
}

// post (fusable plans only): what the second transform's stores turn the bins into - the dB / power rows and hold traces
// of tdsa_chirp.hip's step 4 - instead of leaving complex rows in d_u0 for chirp_post_kernel; null: complex rows
struct ChirpPost {
  int first_frame_index, db_mode;
  float pscale, log_floor, cal_db;
  const float* tare;
  float* out_db;
  float* out_lin;
  float* hold_max;
  float* hold_min;
};
int chirp_transform(tdsa_plan p, const void* in, int in_format, long long stride, int n_frames, const float2* dc_sub,
                    unsigned xor_mask, float in_off, const ChirpPost* post) {
  const int N = p->nfft, M = p->m_fft;
  hipStream_t s = p->stream;
  const bool fused = chirp_fusable(p) && post != nullptr;  // both element-wise passes ride the transforms
  const bool bfused = fused && p->chirp_big;
  const int H = p->chirp_split;                            // > 0: two half-length rows per frame
  const size_t rows_max = size_t(p->max_frames) * (H ? 2 : 1);
  const int n_rows = n_frames * (H ? 2 : 1);
  if (!p->d_u0 && !fused) HIPCHK(p->d_u0.alloc(rows_max * M));
  if (!p->d_u1 && !(fused && p->chirp_single && !p->chirp_big)) HIPCHK(p->d_u1.alloc(rows_max * M));
  if (!fused)
    HIPCHK(launch_chirp_pre(in, in_format == TDSA_IN_C64, stride, N, M, n_frames, p->d_window[in_format], p->d_chirp_a, dc_sub,
                            xor_mask, in_off, p->d_u0, s, H));
  if (p->chirp_big) {
    // M = N1 x 16384: first transform as for a native long frame (column pass -> rows through the frame kernel, which
    // stores conj(X B) in its own [k1][k2] order); second transform transposed (rows first, then the per-column N1-point
    // DFT that leaves natural order): tdsa_big.hip
    const int n1 = M >> kMaxLog2N;
    const long long rowb = (long long)(1 << kMaxLog2N) * sizeof(float2), segb = (long long)M * sizeof(float2);
    if (!p->d_z) HIPCHK(p->d_z.alloc(rows_max * M));
    BigWindow flat{};                   // the rows are windowed already (chirp_pre): one for every sample
    flat.mode = 2;
    flat.table = p->d_ones;
    flat.flat = 1.0f;
    if (bfused) {                       // ... or are never stored: the raw frames are unpacked by the column pass itself
      const BigChirpPre pre{p->d_chirp_aw[in_format], N, in_format == TDSA_IN_C64, H};
      HIPCHK(launch_big_cols(p->log2m, in, 1, stride, n_rows, flat, p->d_tw_seed, dc_sub, p->d_z, xor_mask, in_off, s, 0u, &pre));
    } else {
      HIPCHK(launch_big_cols(p->log2m, p->d_u0, 1, segb, n_rows, flat, p->d_tw_seed, nullptr, p->d_z, 0u, 0.0f, s,
                             unsigned(H ? H : N)));
    }
    // the last column pass turns the bins into the dB / power rows (fused plans); hold traces from the finished rows
    const BigChirpPost bpost = bfused ? BigChirpPost{N, H, 1.0f / float(M), post->db_mode, post->pscale, post->log_floor,
                                                     post->cal_db, post->tare, post->out_db, post->out_lin}
                                      : BigChirpPost{};
    const auto hold_rows = [&]() -> int {
      if (bfused && post->out_lin == nullptr && (post->hold_max || post->hold_min))
        HIPCHK(launch_chirp_hold(post->out_db, N, n_frames, post->first_frame_index, post->hold_max, post->hold_min, s));
      return TDSA_OK;
    };

    SpecParams sp{};
    sp.frame_stride = rowb;
    sp.n_frames = n_rows * n1;
    sp.first_frame_index = 1;
    sp.window = p->d_ones;
    sp.window_perm = p->d_ones;
    sp.tw = p->d_tw;
    sp.in_scale = 1.0f;
    sp.dc_mode = DC_NONE;
    sp.db_mode = TDSA_DB_POW;
    sp.pscale = 1.0f;
    const LaunchGeom g = spectrum_geometry(kMaxLog2N, sp.n_frames, p->num_cu);
    sp.in = p->d_z;
    sp.out_cplx = p->d_u1;
    sp.out_mul = H ? nullptr : p->d_chirp_b;       // [k1][k2] order, row k1 = frame mod N1
    sp.out_mul_rows = H ? 0 : n1;
    if (!H && p->chirp_single) {
      // the row pass of the first transform and the row pass of the transposed second one work on the SAME row k1 (its
      // bins k1 + N1 k2 over k2): one pass through the workgroup does both, with the filter multiply between them
      // (spectrum_kernel<14, true, 0, 4>) - the rows are written once and read once less
      sp.rows_twice = 1;
      TRY(launch_spectrum_profiled(p, 1, sp, g));
      HIPCHK(launch_big_cols_out(p->log2m, p->d_u1, segb, n_rows, p->d_tw_seed, p->d_u0, unsigned(N), s, bfused ? &bpost : nullptr));
      return hold_rows();
    }
    TRY(launch_spectrum_profiled(p, 1, sp, g));
    if (H)    // split plans: the two half-rows' spectra meet the three filter segments: conj(UA B0 + UB Bm), conj(UA Bp + UB B0)
      HIPCHK(launch_chirp_split_combine(p->d_u1, (long long)M, n_frames, p->d_chirp_b, p->d_chirp_bm, p->d_chirp_bp, s));
    sp.in = p->d_u1;
    sp.out_cplx = p->d_z;
    sp.out_mul = nullptr;
    sp.out_mul_rows = 0;
    TRY(launch_spectrum_profiled(p, 1, sp, g));

    HIPCHK(launch_big_cols_out(p->log2m, p->d_z, segb, n_rows, p->d_tw_seed, p->d_u0, unsigned(H ? H : N), s, bfused ? &bpost : nullptr));
    return hold_rows();
  }
  SpecParams sp{};
  sp.frame_stride = (long long)M * sizeof(float2);
  sp.n_frames = n_frames;
  sp.first_frame_index = 1;
  sp.window = p->d_ones;
  sp.window_perm = p->d_ones;
  sp.tw = p->d_tw;
  sp.in_scale = 1.0f;
  sp.dc_mode = DC_NONE;
  sp.db_mode = TDSA_DB_POW;
  sp.pscale = 1.0f;
  const LaunchGeom g = spectrum_geometry(p->log2m, n_frames, p->num_cu);
  sp.in = p->d_u0;
  sp.out_cplx = p->d_u1;
  sp.out_mul = p->d_chirp_b;          // the first transform stores conj(FFT_M(U) * B)
  sp.in_valid = N;                    // rows of U: N samples, the padding up to M is neither written nor read
  if (fused) {                        // ... and U itself is never stored: the raw frames are unpacked on load
    sp.in = in;
    sp.pre_raw = in;
    sp.pre_stride = stride;
    sp.pre_aw = p->d_chirp_aw[in_format];
    sp.pre_c64 = in_format == TDSA_IN_C64;
    sp.dc_sub = dc_sub;
    sp.pre_xor = xor_mask;
    sp.pre_off = in_off;
  }
  const auto set_post = [&] {         // what the second transform's stores turn the bins into
    sp.out_cplx = nullptr;
    sp.out_valid = 0;
    sp.post_n = N;
    sp.post_inv_m = 1.0f / float(M);
    sp.first_frame_index = post->first_frame_index;
    sp.db_mode = post->db_mode;
    sp.pscale = post->pscale;
    sp.log_floor = post->log_floor;
    sp.cal_db = post->cal_db;
    sp.tare = post->tare;
    sp.out_db = post->out_db;
    sp.out_lin = post->out_lin;
  };
  if (fused && p->chirp_single) {
    // the whole convolution of a frame in one pass through its workgroup (spectrum_kernel<L, true, 0, 3>): transform,
    // x B, conjugate, through LDS back into sample order, transform, dB rows - the complex64 intermediate never leaves the CU
    set_post();
    TRY(launch_spectrum_profiled(p, 1, sp, g));
    if (post->out_lin == nullptr && (post->hold_max || post->hold_min))
      HIPCHK(launch_chirp_hold(post->out_db, N, n_frames, post->first_frame_index, post->hold_max, post->hold_min, s));
    return TDSA_OK;
  }
  TRY(launch_spectrum_profiled(p, 1, sp, g));
  sp.in = p->d_u1;
  sp.pre_raw = nullptr;
  sp.dc_sub = nullptr;
  sp.out_cplx = p->d_u0;
  sp.out_mul = nullptr;
  sp.in_valid = 0;
  sp.out_valid = N;                   // only bins k < N of the convolution are needed
  if (fused) set_post();              // ... and leave as the dB / power rows themselves
  TRY(launch_spectrum_profiled(p, 1, sp, g));
  if (fused && post->out_lin == nullptr && (post->hold_max || post->hold_min))
    HIPCHK(launch_chirp_hold(post->out_db, N, n_frames, post->first_frame_index, post->hold_max, post->hold_min, s));
  return TDSA_OK;
}

// Plans whose frame length is not a power of two (tdsa_chirp.hip): same modes, same state, same outputs as the
// native sizes - every stage on the plan's main stream.
int process_chirp(tdsa_plan p, int in_format, const void* iq_dev, int hop, int n_frames, float* out_db_dev) {
  const tdsa_mode& m = p->mode;
  const bool averaging = avg_active(m);
  const int N = p->nfft, M = p->m_fft;
  const int in_c64 = in_format == TDSA_IN_C64;
  const auto [xor_mask, in_off, in_scale] = in_format_consts(in_format);
  const long long stride = (long long)hop * bytes_per_sample(in_format);
  hipStream_t s = p->stream;
  const float2* dc_sub = nullptr;
  const bool smooth = p->smooth && p->smooth_on;      // a transform of exactly N points instead of the convolution
  // ... whose kernel forms the frame means of byte samples itself when the call has few frames (a GUI tick has one: a launch
  // less, 34 -> 28 us per host call at N = 1000; in batches the frame-by-frame reductions cost more than the sums kernel)
  const bool dc_own = smooth && p->smooth_n1 == 0 && !in_c64 && m.dc_alpha >= 1.0f && n_frames <= 8;
  const int twice_zero = in_format == TDSA_IN_I8 ? 256 : (in_c64 ? 0 : 255);
  if (m.dc_alpha >= 0.0f && !dc_own) {
    // frame means as residuals (exact sums); 0 <= alpha < 1: the tracker of the native path fed with them
    // directly (n = 1, zero level 0)
    const bool tracked = m.dc_alpha < 1.0f;
    if (chirp_sum_chunks(N) > 1 && !p->d_sums64)      // long frames: several workgroups per frame leave partial sums here
      HIPCHK(p->d_sums64.alloc(size_t(p->max_frames) * chirp_sum_chunks(N) * 2));
    HIPCHK(launch_chirp_sums(iq_dev, in_c64, xor_mask, stride, N, n_frames, twice_zero, p->d_sums,
                             tracked ? nullptr : p->d_dc_state, in_scale, s, p->d_sums64));
    dc_sub = p->d_sums;                   // dc_alpha >= 1: the frame's own mean
    if (tracked) {
      HIPCHK(launch_dc_track(p->d_sums, 1, n_frames, m.dc_alpha, 0.0f, in_scale, p->d_dc_state, p->d_dc_sub, s));
      dc_sub = p->d_dc_sub;
    }
  }
  const float pscale = m.db_mode == TDSA_DB_POW ? m.power_scale : 1.0f;
  float* const tare = p->tare_active ? p->d_tare_base : nullptr;
  const int first = p->frames_seen > 0 ? 1 : 0;
  if (averaging && !p->d_lin) HIPCHK(p->d_lin.alloc(size_t(p->max_frames) * N));
  // the power / dB rows leave the second transform directly (linear rows for the averager's scan, else dB rows + hold
  // traces); frames below 1024 points (and the A/B knobs): complex rows in d_u0, chirp_post below
  const bool fusable = chirp_fusable(p) || smooth;
  const bool holding = (m.hold_flags & (TDSA_HOLD_MAX | TDSA_HOLD_MIN)) != 0;
  float* rows = out_db_dev;
  if (fusable && !averaging && rows == nullptr && holding) {   // only the hold traces are wanted: the rows go to scratch
    if (!p->d_u0) HIPCHK(p->d_u0.alloc(size_t(p->max_frames) * (p->chirp_split ? 2 : 1) * M));
    rows = p->d_u0.as<float>();
  }
  if (fusable && !averaging && rows == nullptr) {              // nothing to produce (no rows, no hold, no averaging)
    if (dc_own)                                                // (but the estimate the plan carries moves on)
      HIPCHK(launch_chirp_sums(iq_dev, in_c64, xor_mask, stride, N, n_frames, twice_zero, p->d_sums, p->d_dc_state, in_scale, s,
                               p->d_sums64));
    p->frames_seen += n_frames;
    return TDSA_OK;
  }
  const ChirpPost post{first, m.db_mode, pscale, m.log_floor, m.cal_offset_db, averaging ? nullptr : tare,
                       averaging ? nullptr : rows, averaging ? p->d_lin : nullptr,
                       (!averaging && (m.hold_flags & TDSA_HOLD_MAX)) ? p->d_hold_max : nullptr,
                       (!averaging && (m.hold_flags & TDSA_HOLD_MIN)) ? p->d_hold_min : nullptr};
  if (smooth) {
    SmoothParams sp{};
    sp.in = iq_dev;
    sp.in_c64 = in_c64;
    sp.frame_stride = stride;
    sp.n = N;
    sp.n_frames = n_frames;
    sp.n_stages = p->smooth_stages;
    for (int i = 0; i < p->smooth_stages; ++i) sp.radix[i] = p->smooth_radix[i];
    sp.tw = p->d_smooth_tw;
    sp.tw_step = 1;
    sp.window = p->d_window[in_format];
    sp.dc_sub = dc_sub;
    sp.dc_own = dc_own;
    sp.twice_zero = twice_zero;
    sp.in_scale = in_scale;
    sp.dc_state = p->d_dc_state;
    sp.xor_mask = xor_mask;
    sp.in_off = in_off;
    sp.db_mode = post.db_mode;
    sp.pscale = post.pscale;
    sp.log_floor = post.log_floor;
    sp.cal_db = post.cal_db;
    sp.tare = post.tare;
    sp.out_db = post.out_db;
    sp.out_lin = post.out_lin;
    if (p->smooth_n1 == 0) {
      HIPCHK(launch_smooth(sp, s));
    } else {
      // above the LDS limit: column pass (n1-point transforms of fpw adjacent columns, times W_N^(n2 k1)) into z, row pass
      // (n2-point transforms of adjacent rows k1) from z to the dB rows
      if (!p->d_smooth_z) HIPCHK(p->d_smooth_z.alloc(size_t(p->max_frames) * N));
      sp.n_total = N;
      sp.n1 = p->smooth_n1;
      sp.n2 = p->smooth_n2;
      sp.z = p->d_smooth_z;
      sp.n = p->smooth_n1;
      sp.tw_step = p->smooth_n2;
      HIPCHK(launch_smooth(sp, s, 1));
      sp.n = p->smooth_n2;
      sp.tw_step = p->smooth_n1;
      sp.n_stages = p->smooth_stages2;
      for (int i = 0; i < p->smooth_stages2; ++i) sp.radix[i] = p->smooth_radix2[i];
      HIPCHK(launch_smooth(sp, s, 2));
    }
    if (post.out_lin == nullptr && (post.hold_max || post.hold_min))
      HIPCHK(launch_chirp_hold(post.out_db, N, n_frames, post.first_frame_index, post.hold_max, post.hold_min, s));
  } else {
    TRY(chirp_transform(p, iq_dev, in_format, stride, n_frames, dc_sub, xor_mask, in_off, fusable ? &post : nullptr));
  }
  if (averaging) {
    if (!p->d_carry && p->max_frames > 128) HIPCHK(p->d_carry.alloc(size_t(avg_scan_chunks(p->max_frames)) * N));
    if (!fusable)
      HIPCHK(launch_chirp_post(p->d_u0, N, M, n_frames, first, m.db_mode, pscale, m.log_floor,
                               m.cal_offset_db, nullptr, nullptr, p->d_lin, nullptr, nullptr, s, p->chirp_split));
    AvgParams ap = avg_params(p, p->d_lin, n_frames, N, out_db_dev);
    ap.tare = tare;
    ap.state_max = (m.hold_flags & TDSA_HOLD_MAX) ? p->d_hold_max : nullptr;
    ap.state_min = (m.hold_flags & TDSA_HOLD_MIN) ? p->d_hold_min : nullptr;
    TRY(avg_use_ranges(p, ap, n_frames, s));
    HIPCHK(launch_avg_scan(ap, s, p->d_carry));
    avg_advance(p, n_frames);
  } else if (!fusable) {
    HIPCHK(launch_chirp_post(p->d_u0, N, M, n_frames, first, m.db_mode, pscale, m.log_floor,
                             m.cal_offset_db, tare, out_db_dev, nullptr,
                             (m.hold_flags & TDSA_HOLD_MAX) ? p->d_hold_max : nullptr,
                             (m.hold_flags & TDSA_HOLD_MIN) ? p->d_hold_min : nullptr, s, p->chirp_split));
  }
  if (m.hold_flags & TDSA_HOLD_MAX) p->held_max += n_frames;
  if (m.hold_flags & TDSA_HOLD_MIN) p->held_min += n_frames;
  p->frames_seen += n_frames;
  return TDSA_OK;
}

}  // namespace tdsa
