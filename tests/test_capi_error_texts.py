"""The texts tdsa_last_error_string returns for the argument errors of the detector, the channel measurements, the power
statistics, the pulse analysis, the symbol recovery and the FSK analysis that need no live handle, and for the
null-handle timer calls of every handle type that has a timer.  Every text is compared whole: the entry points of these handles share their checks, and a shared
check must go on naming the handle it speaks for.  No call here reaches a device."""
import ctypes as C

from topdogspectrumanalyser_amd import _native as nat

lib = nat.lib
BUF = (C.c_ubyte * 256)()
H = C.c_void_p()
N = C.c_int(0)
I8, U8, C64 = nat.IN_I8, nat.IN_U8, nat.IN_C64


def ints(*v):
    return (C.c_int * len(v))(*v)


def out():
    return C.byref(H)


DETECT_OK = (0, 63, 31, 10.0, 1, 0, 3.0, 16)          # bin_lo, bin_hi, rank, margin_db, min_width, max_gap, xdb, max_signals
MEAS_OK = (1, ints(0), ints(63), 0, 63, 0.99, 26.0)   # n_channels, lo, hi, obw_lo, obw_hi, fraction, xdb
ONE = 1 << 32                                         # one sample in 32.32: 4 samples per symbol have nu = 2^30
SYM_OK = (4 * ONE, 1 << 30, 4, 0.0, 0, 0)             # step, nu, order, ref_arg, timing_mode, delta_fx
FSK_OK = (4 * ONE, 1 << 30, 2, 0, 2, 2, 0, 0)         # step, nu, levels, input_kind, boxcar, lag, timing_mode, delta_fx
STEP_RANGE = "4 .. 64 samples per symbol in 32.32 fixed point"
DELTA_RANGE = "2^32 <= delta_fx < step + 2^32"

CASES = [
    # ---- signal detection ------------------------------------------------------------------------------------------
    ("tdsa_detect_create", (0, 64, 4, None), "null out"),
    ("tdsa_detect_create", (0, 0, 4, out()), "n_bins=0: 1 .. 16384"),
    ("tdsa_detect_create", (0, 16385, 4, out()), "n_bins=16385: 1 .. 16384"),
    ("tdsa_detect_create", (0, 64, 0, out()), "max_host_rows=0: at least 1"),
    ("tdsa_detect_configure", (None, -1, 63, 31, 10.0, 1, 0, 3.0, 16), "bins -1 .. 63: 0 <= bin_lo <= bin_hi < n_bins"),
    ("tdsa_detect_configure", (None, 5, 4, 0, 10.0, 1, 0, 3.0, 16), "bins 5 .. 4: 0 <= bin_lo <= bin_hi < n_bins"),
    ("tdsa_detect_configure", (None, 0, 16384, 0, 10.0, 1, 0, 3.0, 16), "bins 0 .. 16384: 0 <= bin_lo <= bin_hi < n_bins"),
    ("tdsa_detect_configure", (None, 0, 63, 64, 10.0, 1, 0, 3.0, 16), "rank=64: 0 .. 63, the range's bins less one"),
    ("tdsa_detect_configure", (None, 0, 63, 31, float("inf"), 1, 0, 3.0, 16), "margin_db is not finite"),
    ("tdsa_detect_configure", (None, 0, 63, 31, 10.0, 0, 0, 3.0, 16), "min_width=0: 1 .. n_bins"),
    ("tdsa_detect_configure", (None, 0, 63, 31, 10.0, 1, -1, 3.0, 16), "max_gap=-1: 0 .. n_bins"),
    ("tdsa_detect_configure", (None, 0, 63, 31, 10.0, 1, 0, -0.5, 16), "xdb=-0.5: finite and not negative"),
    ("tdsa_detect_configure", (None, 0, 63, 31, 10.0, 1, 0, 3.0, 65), "max_signals=65: 1 .. 64"),
    ("tdsa_detect_configure", (None,) + DETECT_OK, "null detector"),
    ("tdsa_detect_process", (None, BUF, 1, BUF, BUF), "null detector"),
    ("tdsa_detect_process", (None, None, 1, None, None), "null detector"),
    ("tdsa_detect_process_dev", (None, None, BUF, 1, BUF, BUF), "null detector"),
    ("tdsa_detect_process_dev", (None, None, C.c_void_p(4098), 1, BUF, BUF), "null detector"),
    ("tdsa_detect_read_occupancy", (None, None, None, None), "null detector"),
    ("tdsa_detect_reset", (None,), "null detector"),
    ("tdsa_detect_timer_begin", (None,), "null detector"),
    ("tdsa_detect_timer_end", (None, None), "null detector"),
    # ---- channel measurements --------------------------------------------------------------------------------------
    ("tdsa_meas_create", (0, 64, 4, None), "null out"),
    ("tdsa_meas_create", (0, 0, 4, out()), "n_bins=0: 1 .. 16384"),
    ("tdsa_meas_create", (0, 64, 0, out()), "max_host_rows=0: at least 1"),
    ("tdsa_meas_configure", (None, 0, ints(0), ints(63), 0, 63, 0.99, 26.0), "n_channels=0: 1 .. 16"),
    ("tdsa_meas_configure", (None, 1, None, ints(63), 0, 63, 0.99, 26.0),
     "channel bounds missing: lo and hi hold n_channels bins each"),
    ("tdsa_meas_configure", (None, 2, ints(0, 5), ints(63, 4), 0, 63, 0.99, 26.0),
     "channel 1, bins 5 .. 4: 0 <= lo <= hi < n_bins"),
    ("tdsa_meas_configure", (None, 1, ints(0), ints(63), 5, 4, 0.99, 26.0), "obw bins 5 .. 4: 0 <= obw_lo <= obw_hi < n_bins"),
    ("tdsa_meas_configure", (None, 1, ints(0), ints(63), 0, 63, 1.0, 26.0), "fraction=1: above 0 and below 1"),
    ("tdsa_meas_configure", (None, 1, ints(0), ints(63), 0, 63, 0.99, -0.5), "xdb=-0.5: finite and not negative"),
    ("tdsa_meas_configure", (None,) + MEAS_OK, "null measurement handle"),
    ("tdsa_meas_set_limit", (None, BUF, 64, 2), "relative=2: 0 (absolute) or 1 (to channel 0's peak)"),
    ("tdsa_meas_set_limit", (None, BUF, 64, 0), "null measurement handle"),
    ("tdsa_meas_process", (None, BUF, 1, BUF, BUF), "null measurement handle"),
    ("tdsa_meas_process", (None, None, 1, None, None), "null measurement handle"),
    ("tdsa_meas_process_dev", (None, None, BUF, 1, BUF, BUF), "null measurement handle"),
    ("tdsa_meas_process_dev", (None, None, C.c_void_p(4098), 1, BUF, BUF), "null measurement handle"),
    ("tdsa_meas_read_totals", (None, None, None), "null measurement handle"),
    ("tdsa_meas_reset", (None,), "null measurement handle"),
    ("tdsa_meas_timer_begin", (None,), "null measurement handle"),
    ("tdsa_meas_timer_end", (None, None), "null measurement handle"),
    # ---- power statistics ------------------------------------------------------------------------------------------
    ("tdsa_pstat_create", (0, 1, 1024, None), "null out"),
    ("tdsa_pstat_create", (0, 0, 1024, out()), "streams=0: 1 .. 256"),
    ("tdsa_pstat_create", (0, 257, 1024, out()), "streams=257: 1 .. 256"),
    ("tdsa_pstat_create", (0, 4, 3, out()), "max_host_samples=3: at least one sample per stream (4)"),
    ("tdsa_pstat_configure", (None, -127, 0.0), "exp_lo=-127: -126 .. 64"),
    ("tdsa_pstat_configure", (None, 65, 0.0), "exp_lo=65: -126 .. 64"),
    ("tdsa_pstat_configure", (None, -40, -1.0), "gate=-1: finite and not negative (0 = off)"),
    ("tdsa_pstat_configure", (None, -40, 0.0), "null power statistics handle"),
    ("tdsa_pstat_reset", (None,), "null power statistics handle"),
    ("tdsa_pstat_process", (None, 3, BUF, 4, 4),
     "in_format=3: the power statistics take complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pstat_process", (None, -1, BUF, 4, 4),
     "in_format=-1: the power statistics take complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pstat_process", (None, I8, C.c_void_p(4097), 4, 4), "null power statistics handle"),   # a host pointer aligns to nothing
    ("tdsa_pstat_process", (None, C64, None, 4, 4), "null power statistics handle"),
    ("tdsa_pstat_process_dev", (None, None, 3, BUF, 4, 4),
     "in_format=3: the power statistics take complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pstat_process_dev", (None, None, C64, C.c_void_p(4100), 4, 4), "input pointer must be aligned to one sample (8 bytes)"),
    ("tdsa_pstat_process_dev", (None, None, I8, C.c_void_p(4097), 4, 4), "input pointer must be aligned to one sample (2 bytes)"),
    ("tdsa_pstat_process_dev", (None, None, U8, C.c_void_p(4097), 4, 4), "input pointer must be aligned to one sample (2 bytes)"),
    ("tdsa_pstat_process_dev", (None, None, U8, C.c_void_p(4096), 4, 4), "null power statistics handle"),
    ("tdsa_pstat_read", (None, 0, 1, None, None, None), "null records"),
    ("tdsa_pstat_read", (None, 0, 1, BUF, None, None), "null power statistics handle"),
    ("tdsa_pstat_timer_begin", (None,), "null power statistics handle"),
    ("tdsa_pstat_timer_end", (None, None), "null power statistics handle"),
    # ---- pulse analysis --------------------------------------------------------------------------------------------
    ("tdsa_pulse_create", (0, 1, 16, 1024, None), "null out"),
    ("tdsa_pulse_create", (0, 0, 16, 1024, out()), "streams=0: 1 .. 256"),
    ("tdsa_pulse_create", (0, 1, 0, 1024, out()), "capacity=0: at least 1, streams * capacity at most 4194304"),
    ("tdsa_pulse_create", (0, 256, (1 << 14) + 1, 1024, out()), "capacity=16385: at least 1, streams * capacity at most 4194304"),
    ("tdsa_pulse_create", (0, 4, 16, 3, out()), "max_host_samples=3: at least one sample per stream (4)"),
    ("tdsa_pulse_configure", (None, 0.0, 0.5, 1), "on_level=0: a finite float32 above 0"),
    ("tdsa_pulse_configure", (None, 1.0, 1.5, 1), "off_level=1.5: above 0 and at most on_level=1"),
    ("tdsa_pulse_configure", (None, 1.0, 1.0, 0), "min_width=0: 1 .. 2^31 - 1"),
    ("tdsa_pulse_configure", (None, 1.0, 1.0, 1 << 31), "min_width=2147483648: 1 .. 2^31 - 1"),
    ("tdsa_pulse_configure", (None, 1.0, 0.5, 1), "null pulse handle"),
    ("tdsa_pulse_reset", (None,), "null pulse handle"),
    ("tdsa_pulse_process", (None, 3, BUF, 4, 4), "in_format=3: the pulse analysis takes complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pulse_process", (None, -1, BUF, 4, 4), "in_format=-1: the pulse analysis takes complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pulse_process", (None, I8, C.c_void_p(4097), 4, 4), "null pulse handle"),
    ("tdsa_pulse_process", (None, C64, None, 4, 4), "null pulse handle"),
    ("tdsa_pulse_process_dev", (None, None, 7, BUF, 4, 4), "in_format=7: the pulse analysis takes complex IQ (TDSA_IN_I8 / _U8 / _C64)"),
    ("tdsa_pulse_process_dev", (None, None, C64, C.c_void_p(4100), 4, 4), "input pointer must be aligned to one sample (8 bytes)"),
    ("tdsa_pulse_process_dev", (None, None, I8, C.c_void_p(4097), 4, 4), "input pointer must be aligned to one sample (2 bytes)"),
    ("tdsa_pulse_process_dev", (None, None, U8, C.c_void_p(4096), 4, 4), "null pulse handle"),
    ("tdsa_pulse_read", (None, 0, 1, None), "null summaries"),
    ("tdsa_pulse_read", (None, 0, 1, BUF), "null pulse handle"),
    ("tdsa_pulse_read_pulses", (None, 0, 0, 1, BUF, None), "null n_out"),
    ("tdsa_pulse_read_pulses", (None, 0, 0, 1, BUF, C.byref(N)), "null pulse handle"),
    ("tdsa_pulse_debug_limits", (None, 16, 7), "null pulse handle"),
    ("tdsa_pulse_timer_begin", (None,), "null pulse handle"),
    ("tdsa_pulse_timer_end", (None, None), "null pulse handle"),
    # ---- symbol recovery ----------------------------------------------------------------------------------------------
    ("tdsa_symsync_create", (0, 4096, None), "null out"),
    ("tdsa_symsync_create", (0, 8, out()), "max_host_samples=8: at least 16"),
    ("tdsa_symsync_configure", (None, 4 * ONE - 1) + SYM_OK[1:], f"step={4 * ONE - 1}: {STEP_RANGE}"),
    ("tdsa_symsync_configure", (None, 64 * ONE + 1, 1 << 26) + SYM_OK[2:], f"step={64 * ONE + 1}: {STEP_RANGE}"),
    ("tdsa_symsync_configure", (None, 4 * ONE, (1 << 30) + 2) + SYM_OK[2:], "nu=1073741826: the phase step of this symbol rate is 1073741824"),
    ("tdsa_symsync_configure", (None, 4 * ONE, (1 << 30) - 2) + SYM_OK[2:], "nu=1073741822: the phase step of this symbol rate is 1073741824"),
    ("tdsa_symsync_configure", (None, 4 * ONE, 1 << 30, 3, 0.0, 0, 0), "order=3: 0, 2, 4 or 8"),
    ("tdsa_symsync_configure", (None, 4 * ONE, 1 << 30, 4, float("nan"), 0, 0), "ref_arg is not finite"),
    ("tdsa_symsync_configure", (None, 4 * ONE, 1 << 30, 4, 0.0, 2, 0), "timing_mode=2: TDSA_SYMSYNC_AUTO or _FIXED"),
    ("tdsa_symsync_configure", (None, 4 * ONE, 1 << 30, 4, 0.0, 1, ONE - 1), f"delta_fx={ONE - 1}: {DELTA_RANGE}"),
    ("tdsa_symsync_configure", (None, 4 * ONE, 1 << 30, 4, 0.0, 1, 5 * ONE), f"delta_fx={5 * ONE}: {DELTA_RANGE}"),
    ("tdsa_symsync_configure", (None,) + SYM_OK, "null symbol synchroniser"),
    ("tdsa_symsync_symbols_per_segment", (4 * ONE, 100, None), "null K"),
    ("tdsa_symsync_symbols_per_segment", (4 * ONE - 1, 100, C.byref(N)), f"step={4 * ONE - 1}: {STEP_RANGE}"),
    ("tdsa_symsync_process", (None, BUF, 100, 100, 100, 1, BUF, 64, None, BUF), "null symbol synchroniser"),
    ("tdsa_symsync_process", (None, None, 100, 100, 0, 0, None, 0, None, None), "null symbol synchroniser"),
    ("tdsa_symsync_process_dev", (None, None, BUF, 100, 100, 1, BUF, 64, None, BUF), "null symbol synchroniser"),
    ("tdsa_symsync_process_dev", (None, None, C.c_void_p(4100), 100, 100, 1, BUF, 64, None, BUF), "null symbol synchroniser"),
    ("tdsa_symsync_timer_begin", (None,), "null symbol synchroniser"),
    ("tdsa_symsync_timer_end", (None, None), "null symbol synchroniser"),
    # ---- FSK analysis --------------------------------------------------------------------------------------------------
    ("tdsa_fsk_create", (0, 4096, None), "null out"),
    ("tdsa_fsk_create", (0, 8, out()), "max_host_samples=8: at least 16"),
    ("tdsa_fsk_configure", (None, 4 * ONE - 1) + FSK_OK[1:], f"step={4 * ONE - 1}: {STEP_RANGE}"),
    ("tdsa_fsk_configure", (None, 64 * ONE + 1, 1 << 26) + FSK_OK[2:], f"step={64 * ONE + 1}: {STEP_RANGE}"),
    ("tdsa_fsk_configure", (None, 4 * ONE, (1 << 30) + 2) + FSK_OK[2:], "nu=1073741826: the phase step of this symbol rate is 1073741824"),
    ("tdsa_fsk_configure", (None, 4 * ONE, (1 << 30) - 2) + FSK_OK[2:], "nu=1073741822: the phase step of this symbol rate is 1073741824"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 3, 0, 2, 2, 0, 0), "levels=3: 2, 4 or 8"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 2, 2, 2, 0, 0), "input_kind=2: TDSA_FSK_IQ or _FREQ"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 0, 2, 0, 0), "boxcar=0: 1 .. 64 samples"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 65, 2, 0, 0), "boxcar=65: 1 .. 64 samples"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 2, 0, 0, 0), "lag=0: 1 .. 64 samples"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 2, 65, 0, 0), "lag=65: 1 .. 64 samples"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 2, 2, 2, 0), "timing_mode=2: TDSA_FSK_AUTO or _FIXED"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 2, 2, 1, ONE - 1), f"delta_fx={ONE - 1}: {DELTA_RANGE}"),
    ("tdsa_fsk_configure", (None, 4 * ONE, 1 << 30, 2, 0, 2, 2, 1, 5 * ONE), f"delta_fx={5 * ONE}: {DELTA_RANGE}"),
    ("tdsa_fsk_configure", (None,) + FSK_OK, "null FSK analyser"),
    ("tdsa_fsk_symbols_per_segment", (4 * ONE, 100, 0, 2, None), "null K"),
    ("tdsa_fsk_symbols_per_segment", (64 * ONE + 1, 100, 0, 2, C.byref(N)), f"step={64 * ONE + 1}: {STEP_RANGE}"),
    ("tdsa_fsk_symbols_per_segment", (4 * ONE, 100, -1, 2, C.byref(N)), "input_kind=-1: TDSA_FSK_IQ or _FREQ"),
    ("tdsa_fsk_symbols_per_segment", (4 * ONE, 100, 1, 65, C.byref(N)), "boxcar=65: 1 .. 64 samples"),
    ("tdsa_fsk_process", (None, BUF, 100, 100, 100, 1, BUF, 64, None, BUF), "null FSK analyser"),
    ("tdsa_fsk_process", (None, None, 100, 100, 0, 0, None, 0, None, None), "null FSK analyser"),
    ("tdsa_fsk_process_dev", (None, None, BUF, 100, 100, 1, BUF, 64, None, BUF), "null FSK analyser"),
    ("tdsa_fsk_process_dev", (None, None, C.c_void_p(4098), 100, 100, 1, BUF, 64, None, BUF), "null FSK analyser"),
    ("tdsa_fsk_timer_begin", (None,), "null FSK analyser"),
    ("tdsa_fsk_timer_end", (None, None), "null FSK analyser"),
    # ---- the timers of the other handle types ------------------------------------------------------------------------
    ("tdsa_demod_timer_begin", (None,), "null demodulator"),
    ("tdsa_demod_timer_end", (None, None), "null demodulator"),
    ("tdsa_sweep_timer_begin", (None,), "null sweep"),
    ("tdsa_sweep_timer_end", (None, None), "null sweep"),
    ("tdsa_zspan_timer_begin", (None,), "null zero span"),
    ("tdsa_zspan_timer_end", (None, None), "null zero span"),
    ("tdsa_history_timer_begin", (None,), "null history"),
    ("tdsa_history_timer_end", (None, None), "null history"),
]


def test_every_error_text_is_the_recorded_one():
    wrong = []
    for name, args, text in CASES:
        H.value = None
        rc = getattr(lib, name)(*args)
        got = lib.tdsa_last_error_string().decode()
        if rc != -1 or got != text or H.value:             # a refused create leaves no handle behind
            wrong.append((name, rc, got, text))
    assert not wrong, wrong
