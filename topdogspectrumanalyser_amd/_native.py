"""ctypes binding of libtdsa_hip.so (include/tdsa_hip.h).

The HIP library IS the product path: if it is missing or fails to load this module raises
ImportError - there is deliberately no numpy fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TDSA_HIP_LIB", os.path.join(_HERE, "libtdsa_hip.so"))

TDSA_OK = 0
IN_I8, IN_U8, IN_C64 = 0, 1, 2
IN_F32R = 3                                   # real float32: tdsa_zspan_push* only
DB_MAG, DB_POW = 0, 1
AVG_OFF, AVG_EXP, AVG_LIN = 0, 1, 2
HOLD_MAX, HOLD_MIN = 1, 2
CH_MONO, CH_LEFT, CH_RIGHT, CH_STEREO = 0, 1, 2, 3
SWEEP_DET_SAMPLE, SWEEP_DET_MAX, SWEEP_DET_MIN, SWEEP_DET_AVG = 0, 1, 2, 3
SWEEP_INTERP, SWEEP_PEAK = 0, 1
CHAN_BRANCHES = 1
DEMOD_FM, DEMOD_AM = 0, 1
DEMOD_POLE_OFF, DEMOD_POLE_LOWPASS, DEMOD_POLE_HIGHPASS = 0, 1, 2
SYMSYNC_AUTO, SYMSYNC_FIXED = 0, 1
SYMSYNC_NONFINITE, SYMSYNC_NO_CARRIER = 1, 2
FSK_IQ, FSK_FREQ = 0, 1
FSK_AUTO, FSK_FIXED = 0, 1
FSK_NONFINITE, FSK_ONE_LEVEL = 1, 2
EYE_IQ, EYE_FM, EYE_REAL = 0, 1, 2
EYE_MAX_BINS, EYE_TOTALS = 8192, 10
MODQ_MAX_POINTS, MODQ_MAX_SYMBOLS = 64, 4096
MODQ_NONFINITE, MODQ_DEGENERATE, MODQ_ONE_POINT = 1, 2, 4
DETECT_NAN_FLOOR = 1
MEAS_EMPTY, MEAS_INF, MEAS_MASK_FAIL = 1, 2, 4
ZS_DET_REAL, ZS_DET_MAG, ZS_DET_DB = 0, 1, 2
ZS_FREE_RUN, ZS_RISE, ZS_FALL = 0, 1, 2
ZS_COL_MINMAX, ZS_COL_SAMPLE, ZS_COL_MEAN = 0, 1, 2
HIST_HEIGHTS, HIST_LEVELS = 0, 1
HIST_COLOUR_INDEX, HIST_COLOUR_RGBA = 0, 1
RESET_AVG, RESET_HOLD_MAX, RESET_HOLD_MIN, RESET_DC, RESET_TARE, RESET_ALL = 1, 2, 4, 8, 16, 31


class Mode(C.Structure):
    _fields_ = [("db_mode", C.c_int32), ("power_scale", C.c_float), ("log_floor", C.c_float),
                ("avg_mode", C.c_int32), ("avg_n", C.c_int32), ("dc_alpha", C.c_float),
                ("cal_offset_db", C.c_float), ("hold_flags", C.c_uint32)]


class Info(C.Structure):
    _fields_ = [("nfft", C.c_int32), ("max_frames", C.c_int32), ("device_id", C.c_int32),
                ("grid", C.c_int32), ("block", C.c_int32), ("frames_per_block", C.c_int32),
                ("lds_bytes", C.c_int32), ("num_cu", C.c_int32),
                ("frames_held_max", C.c_int64), ("frames_held_min", C.c_int64),
                ("avg_count", C.c_int32), ("version", C.c_int32)]


class ZspanInfo(C.Structure):
    _fields_ = [("start", C.c_int64), ("total", C.c_int64), ("length", C.c_int32), ("triggered", C.c_int32),
                ("n_columns", C.c_int32), ("min", C.c_float), ("max", C.c_float), ("mean", C.c_double),
                ("n_at_or_above", C.c_int64), ("n_rise", C.c_int32), ("n_fall", C.c_int32)]


class HistoryInfo(C.Structure):
    _fields_ = [("pushed", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("valid_rows", C.c_int32),
                ("has_min", C.c_int32), ("live_bin", C.c_int32), ("live_value", C.c_float), ("hold_bin", C.c_int32),
                ("hold_value", C.c_float), ("live_norm", C.c_double)]


class HistoryOut(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("reserved", C.c_int32), ("primary", C.c_void_p), ("colours", C.c_void_p),
                ("bins", C.c_void_p), ("hold", C.c_void_p), ("hold_bins", C.c_void_p), ("min_row", C.c_void_p),
                ("min_bins", C.c_void_p)]


class PstatRecord(C.Structure):
    _fields_ = [("n_total", C.c_uint64), ("n_nan", C.c_uint64), ("n_gated", C.c_uint64), ("n_inf", C.c_uint64),
                ("n_zero", C.c_uint64), ("n_under", C.c_uint64), ("n_over", C.c_uint64), ("max_bits", C.c_uint32),
                ("min_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PulseRecord(C.Structure):
    _fields_ = [("toa", C.c_int64), ("width", C.c_int64), ("peak_index", C.c_int64), ("peak_bits", C.c_uint32),
                ("flags", C.c_uint32), ("energy", C.c_double), ("acc_re", C.c_double), ("acc_im", C.c_double),
                ("reserved", C.c_uint64)]


class PulseSummary(C.Structure):
    _fields_ = [("n_total", C.c_uint64), ("n_on", C.c_uint64), ("n_pulses", C.c_uint64), ("n_short", C.c_uint64),
                ("n_lost", C.c_uint64), ("n_nan", C.c_uint64), ("open_toa", C.c_int64), ("open_width", C.c_int64),
                ("open", C.c_int32), ("reserved", C.c_int32)]


class CorrRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("metric", C.c_float), ("energy", C.c_float), ("c1_re", C.c_float),
                ("c1_im", C.c_float), ("c2_re", C.c_float), ("c2_im", C.c_float)]


class CorrSummary(C.Structure):
    _fields_ = [("n_total", C.c_uint64), ("n_windows", C.c_uint64), ("n_decided", C.c_uint64), ("n_matches", C.c_uint64),
                ("n_lost", C.c_uint64), ("n_bad", C.c_uint64), ("flushed", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/tdsa_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_SIGNATURES = {
    "tdsa_last_error_string": (C.c_char_p, []),
    "tdsa_version": (C.c_int, []),
    "tdsa_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "tdsa_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tdsa_destroy": (C.c_int, [_P]),
    "tdsa_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "tdsa_set_window": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_set_mode": (C.c_int, [_P, C.POINTER(Mode)]),
    "tdsa_reset_state": (C.c_int, [_P, C.c_uint32]),
    "tdsa_set_tare_baseline": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_process_i8": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "tdsa_process_u8": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "tdsa_process_c64": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "tdsa_process_dev": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "tdsa_process_dev_batch": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int, _P,
                                         C.c_size_t]),
    "tdsa_process_real2": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P]),
    "tdsa_real_input_supported": (C.c_int, [C.c_int]),
    "tdsa_get_hold": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int64)]),
    "tdsa_get_avg": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "tdsa_host_register": (C.c_int, [_P, C.c_size_t]),
    "tdsa_host_unregister": (C.c_int, [_P]),
    "tdsa_welch_export": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_welch_combine": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_int32), C.c_int, C.c_int, _P, _P]),
    "tdsa_peer_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P), _P]),
    "tdsa_peer_free": (C.c_int, [C.c_int, _P]),
    "tdsa_peer_open": (C.c_int, [C.c_int, _P, C.c_int, C.POINTER(_P)]),
    "tdsa_peer_can_access": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_peer_close": (C.c_int, [C.c_int, _P]),
    "tdsa_welch_export_dev": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_welch_combine_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.c_int, C.c_int, _P, _P]),
    "tdsa_shader_clock": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tdsa_get_dc": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tdsa_set_dc": (C.c_int, [_P, C.c_float, C.c_float]),
    "tdsa_synchronize": (C.c_int, [_P]),
    "tdsa_set_overlap": (C.c_int, [_P, C.c_int]),
    "tdsa_rows_stats": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    "tdsa_rows_top_peaks": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "tdsa_set_frame_stats": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "tdsa_get_frame_stats": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tdsa_rows_marker_peaks": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                         _P, _P, _P, _P, _P]),
    "tdsa_density_create": (C.c_int, [C.c_int, C.c_int, C.c_float, C.POINTER(_P)]),
    "tdsa_density_destroy": (C.c_int, [_P]),
    "tdsa_density_set_decay": (C.c_int, [_P, C.c_float]),
    "tdsa_density_reset": (C.c_int, [_P]),
    "tdsa_density_update_dev": (C.c_int, [_P, _P, _P, C.c_int]),
    "tdsa_density_update": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_density_read": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_density_read_u8": (C.c_int, [_P, _P, _P]),
    "tdsa_constellation_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_constellation_destroy": (C.c_int, [_P]),
    "tdsa_constellation_set_refs": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tdsa_constellation_set_density": (C.c_int, [_P, C.c_double, C.c_int]),
    "tdsa_constellation_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_int, C.POINTER(C.c_float),
                                             C.POINTER(C.c_double), C.POINTER(C.c_int), _P, _P]),
    "tdsa_constellation_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.c_size_t, C.c_int, _P, _P, _P]),
    "tdsa_ddc_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_ddc_destroy": (C.c_int, [_P]),
    "tdsa_ddc_set_taps": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_ddc_set_nco": (C.c_int, [_P, C.c_uint32]),
    "tdsa_ddc_reset": (C.c_int, [_P]),
    "tdsa_ddc_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P, C.POINTER(C.c_size_t)]),
    "tdsa_ddc_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, _P, C.POINTER(C.c_size_t)]),
    "tdsa_chan_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_chan_destroy": (C.c_int, [_P]),
    "tdsa_chan_set_taps": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_chan_reset": (C.c_int, [_P]),
    "tdsa_chan_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.c_uint, C.POINTER(C.c_size_t)]),
    "tdsa_chan_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.c_uint,
                                        C.POINTER(C.c_size_t)]),
    "tdsa_demod_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_demod_destroy": (C.c_int, [_P]),
    "tdsa_demod_set_taps": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_demod_set_pole": (C.c_int, [_P, C.c_int, C.c_double, C.c_float]),
    "tdsa_demod_reset": (C.c_int, [_P]),
    "tdsa_demod_process": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "tdsa_demod_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "tdsa_demod_read_meas": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "tdsa_demod_reset_meas": (C.c_int, [_P]),
    "tdsa_demod_timer_begin": (C.c_int, [_P]),
    "tdsa_demod_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_symsync_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_symsync_destroy": (C.c_int, [_P]),
    "tdsa_symsync_configure": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_int, C.c_double, C.c_int, C.c_uint64]),
    "tdsa_symsync_process": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_symsync_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_symsync_symbols_per_segment": (C.c_int, [C.c_uint64, C.c_size_t, C.POINTER(C.c_int)]),
    "tdsa_symsync_timer_begin": (C.c_int, [_P]),
    "tdsa_symsync_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_fsk_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_fsk_destroy": (C.c_int, [_P]),
    "tdsa_fsk_configure": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "tdsa_fsk_process": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_fsk_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_fsk_symbols_per_segment": (C.c_int, [C.c_uint64, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_fsk_timer_begin": (C.c_int, [_P]),
    "tdsa_fsk_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_eye_create": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.POINTER(_P)]),
    "tdsa_eye_destroy": (C.c_int, [_P]),
    "tdsa_eye_configure": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]),
    "tdsa_eye_symbols_per_segment": (C.c_int, [C.c_uint64, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_eye_process": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P, _P]),
    "tdsa_eye_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_int, _P, _P]),
    "tdsa_eye_read": (C.c_int, [_P, _P, _P]),
    "tdsa_eye_reset": (C.c_int, [_P]),
    "tdsa_eye_timer_begin": (C.c_int, [_P]),
    "tdsa_eye_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_modq_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_modq_destroy": (C.c_int, [_P]),
    "tdsa_modq_set_points": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_modq_process": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_modq_process_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_size_t, C.c_int, _P, C.c_size_t, _P, _P]),
    "tdsa_modq_timer_begin": (C.c_int, [_P]),
    "tdsa_modq_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_detect_create": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_detect_destroy": (C.c_int, [_P]),
    "tdsa_detect_configure": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int]),
    "tdsa_detect_process": (C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    "tdsa_detect_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P]),
    "tdsa_detect_read_occupancy": (C.c_int, [_P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tdsa_detect_reset": (C.c_int, [_P]),
    "tdsa_detect_timer_begin": (C.c_int, [_P]),
    "tdsa_detect_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_meas_create": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_meas_destroy": (C.c_int, [_P]),
    "tdsa_meas_configure": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_double, C.c_float]),
    "tdsa_meas_set_limit": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tdsa_meas_process": (C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    "tdsa_meas_process_dev": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P]),
    "tdsa_meas_read_totals": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tdsa_meas_reset": (C.c_int, [_P]),
    "tdsa_meas_timer_begin": (C.c_int, [_P]),
    "tdsa_meas_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_pstat_create": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_pstat_destroy": (C.c_int, [_P]),
    "tdsa_pstat_configure": (C.c_int, [_P, C.c_int, C.c_float]),
    "tdsa_pstat_reset": (C.c_int, [_P]),
    "tdsa_pstat_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_pstat_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_pstat_read": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    "tdsa_pstat_timer_begin": (C.c_int, [_P]),
    "tdsa_pstat_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_pulse_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_pulse_destroy": (C.c_int, [_P]),
    "tdsa_pulse_configure": (C.c_int, [_P, C.c_float, C.c_float, C.c_int64]),
    "tdsa_pulse_reset": (C.c_int, [_P]),
    "tdsa_pulse_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_pulse_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_pulse_read": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "tdsa_pulse_read_pulses": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int)]),
    "tdsa_pulse_debug_limits": (C.c_int, [_P, C.c_int, C.c_int]),
    "tdsa_pulse_timer_begin": (C.c_int, [_P]),
    "tdsa_pulse_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_corr_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_size_t, _P, C.c_int, C.POINTER(_P)]),
    "tdsa_corr_destroy": (C.c_int, [_P]),
    "tdsa_corr_set_reference": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_corr_configure": (C.c_int, [_P, C.c_float, C.c_int]),
    "tdsa_corr_reset": (C.c_int, [_P]),
    "tdsa_corr_process": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_corr_process_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "tdsa_corr_flush": (C.c_int, [_P]),
    "tdsa_corr_read": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "tdsa_corr_read_trace": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, _P]),
    "tdsa_corr_debug_limits": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "tdsa_corr_timer_begin": (C.c_int, [_P]),
    "tdsa_corr_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_sweep_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tdsa_sweep_destroy": (C.c_int, [_P]),
    "tdsa_sweep_set_geometry": (C.c_int, [_P, _P, C.c_double, C.c_int, C.c_int, _P]),
    "tdsa_sweep_reset": (C.c_int, [_P]),
    "tdsa_sweep_set_chunk_bytes": (C.c_int, [_P, C.c_size_t]),
    "tdsa_sweep_update_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_size_t, C.c_int]),
    "tdsa_sweep_run_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                     C.c_int]),
    "tdsa_sweep_read": (C.c_int, [_P, C.c_int, _P, _P]),
    "tdsa_sweep_get_steps": (C.c_int, [_P, _P, _P]),
    "tdsa_sweep_timer_begin": (C.c_int, [_P]),
    "tdsa_sweep_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_zspan_create": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "tdsa_zspan_destroy": (C.c_int, [_P]),
    "tdsa_zspan_set_detector": (C.c_int, [_P, C.c_int, C.c_float, C.c_float]),
    "tdsa_zspan_reset": (C.c_int, [_P]),
    "tdsa_zspan_push": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "tdsa_zspan_push_dev": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t]),
    "tdsa_zspan_view": (C.c_int, [_P, C.c_int, C.c_double, C.c_size_t, C.c_int, C.c_int, C.POINTER(ZspanInfo), _P, _P]),
    "tdsa_zspan_timer_begin": (C.c_int, [_P]),
    "tdsa_zspan_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_history_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tdsa_history_destroy": (C.c_int, [_P]),
    "tdsa_history_set_amplitude": (C.c_int, [_P, C.c_double, C.c_double]),
    "tdsa_history_reset": (C.c_int, [_P]),
    "tdsa_history_reset_hold": (C.c_int, [_P]),
    "tdsa_history_push": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "tdsa_history_push_dev": (C.c_int, [_P, _P, _P, C.c_int]),
    "tdsa_history_ribbon": (C.c_int, [_P, _P, C.c_int, C.POINTER(HistoryOut), C.POINTER(HistoryInfo)]),
    "tdsa_history_lines": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(HistoryOut),
                                     C.POINTER(HistoryInfo)]),
    "tdsa_history_surface": (C.c_int, [_P, C.c_int, C.POINTER(HistoryOut), C.POINTER(HistoryInfo)]),
    "tdsa_history_timer_begin": (C.c_int, [_P]),
    "tdsa_history_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_plan_copy": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    "tdsa_waterfall_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(_P)]),
    "tdsa_waterfall_destroy": (C.c_int, [_P]),
    "tdsa_waterfall_push_dev": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_waterfall_push": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "tdsa_waterfall_view": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "tdsa_waterfall_view_u8": (C.c_int, [_P, C.c_float, C.c_float, _P]),
    "tdsa_pipe_create": (C.c_int, [_P, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(_P)]),
    "tdsa_pipe_destroy": (C.c_int, [_P]),
    "tdsa_pipe_acquire": (C.c_int, [_P, C.POINTER(_P)]),
    "tdsa_pipe_submit": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int]),
    "tdsa_pipe_collect": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]),
    "tdsa_pipe_collect_dev": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]),
    "tdsa_pipe_collect_u8": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_int)]),
    "tdsa_pipe_set_levels": (C.c_int, [_P, C.c_float, C.c_float]),
    "tdsa_pipe_pending": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "tdsa_trace_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "tdsa_trace_destroy": (C.c_int, [_P]),
    "tdsa_trace_reset": (C.c_int, [_P, C.c_uint32]),
    "tdsa_trace_update": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                    _P, _P, _P, C.POINTER(C.c_int)]),
    "tdsa_trace_get_tare_baseline": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "tdsa_trace_set_tare_baseline": (C.c_int, [_P, _P, C.c_int]),
    "tdsa_trace_avg_set_mode": (C.c_int, [_P, C.c_int, C.c_int]),
    "tdsa_trace_avg_process": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "tdsa_dev_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_P)]),
    "tdsa_dev_free": (C.c_int, [C.c_int, _P]),
    "tdsa_memcpy_h2d": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "tdsa_memcpy_d2h": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "tdsa_profile_enable": (C.c_int, [_P, C.c_int]),
    "tdsa_profile_read": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "tdsa_timer_begin": (C.c_int, [_P]),
    "tdsa_timer_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tdsa_debug_timeline": (C.c_int, [_P, _P]),
    "tdsa_debug_knob": (C.c_int, [_P, C.c_char_p, C.c_int]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the box
        raise ImportError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class TdsaError(RuntimeError):
    pass


def check(rc: int) -> None:
    if rc != TDSA_OK:
        raise TdsaError(f"tdsa error {rc}: {lib.tdsa_last_error_string().decode()}")


class _Handle:
    """Lifetime of an object that owns device resources: close() once, from __del__ and on leaving a `with` block.  The
    plain case is one library handle in self._h, which close() hands to the library function _destroy names; a class that
    owns something else (several handles, a pipe's _q, a source's engine) overrides close() and needs neither."""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _close_all(obj, *names, wait=None) -> None:
    """The close() of a handle made of handles: waits for the stream of the engine in attribute `wait`, if it is still
    open, then closes the attributes `names` (a handle, or a list of them) that exist, in the order given.  Attributes
    a constructor did not reach are skipped, and close() of a closed handle does nothing."""
    eng = getattr(obj, wait, None) if wait else None
    if eng is not None and eng._h:
        eng.synchronize()
    for name in names:
        held = getattr(obj, name, None)
        for h in held if isinstance(held, list) else [held]:
            if h is not None:
                h.close()


class _Timer:
    """HIP-event timer of a handle: _timer names the library's (begin, end) pair."""
    _timer = ("", "")

    def timer_begin(self) -> None:
        check(getattr(lib, self._timer[0])(self._h))

    def timer_end(self) -> float:
        """Milliseconds of device time on the handle's stream since timer_begin."""
        ms = C.c_float()
        check(getattr(lib, self._timer[1])(self._h, C.byref(ms)))
        return float(ms.value)
