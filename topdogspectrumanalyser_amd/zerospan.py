"""Zero span: amplitude against time at the tuned frequency, on the device.

  view_plan   the host half of the view contract (held, base, search range, free-run start): a pure function
  ZeroSpan    a detector ring in HBM (tdsa_zspan_*): push samples, view a display window free running or aligned to
              the last rise / fall crossing of a level, as the raw chunk or reduced to a screen's worth of columns,
              with the chunk statistics (min, max, mean, duty cycle, pulse count).  With `decimation` the input first
              runs through a DownConverter (NCO, mixer, RBW filter) and the ring holds the detector of its outputs at
              fs / D: zero span as a bench analyser means it.

With detector "real", no decimation and points=None, `view` returns what the reference's DataProcessor.
_process_zero_span_data hands its widget, bit for bit (core/display_data_processor.py:261-311 there).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat
from .devmem import DeviceBuffer
from .engine import SpectrumEngine
from .zoom import DownConverter

BUFFER_SECONDS = 2.0            # the reference's _ZS_BUFFER_SECONDS
MIN_CAPACITY, MAX_CAPACITY = 4, 1 << 28
MAX_POINTS = 16384
DETECTORS = {"real": nat.ZS_DET_REAL, "mag": nat.ZS_DET_MAG, "db": nat.ZS_DET_DB}
MODES = {"free_run": nat.ZS_FREE_RUN, "rise": nat.ZS_RISE, "fall": nat.ZS_FALL}
COLUMNS = {"minmax": nat.ZS_COL_MINMAX, "sample": nat.ZS_COL_SAMPLE, "mean": nat.ZS_COL_MEAN}


def view_plan(total: int, capacity: int, n_display: int, mode: str = "free_run") -> dict:
    """What a view of `n_display` samples sees after `total` samples went into a ring of `capacity`:
    held, base (absolute index of the oldest sample held), length of the chunk, free_start (its start without a
    trigger hit) and search = (ss, se): the ring-relative pairs (i, i + 1), ss <= i <= se - 2, a trigger is looked for
    in - or None (free run, fewer samples held than shown, or an empty range)."""
    if mode not in MODES:
        raise ValueError(f"mode={mode!r}: one of {sorted(MODES)}")
    total, capacity, n_display = int(total), int(capacity), int(n_display)
    if total < 0 or capacity < 1 or n_display < 1:
        raise ValueError(f"total={total}, capacity={capacity}, n_display={n_display}")
    held = min(total, capacity)
    base = total - held
    if held < n_display:
        return dict(held=held, base=base, length=held, free_start=base, search=None)
    search = None
    if mode != "free_run":
        se = held - n_display
        ss = max(0, se - 8 * n_display)
        if se - 2 >= ss:
            search = (ss, se)
    return dict(held=held, base=base, length=n_display, free_start=total - n_display, search=search)


class ZeroSpanView:
    """One view: `.samples` (the raw chunk, points=None) or `.columns` ([2][P] min / max rows, or [P]), `.time_s`
    (np.arange(len, dtype=float32) / rate for the raw chunk as the reference builds it; the start time of each column
    otherwise), `.start` (absolute index of the first sample), `.triggered`, `.total`, `.length`, and the chunk
    statistics `.min`, `.max`, `.mean`, `.n_at_or_above`, `.n_rise`, `.n_fall`."""

    def __init__(self, info: nat.ZspanInfo, rate: float, samples, columns):
        self.samples, self.columns, self.rate = samples, columns, float(rate)
        self.start, self.total, self.length = int(info.start), int(info.total), int(info.length)
        self.triggered = bool(info.triggered)
        self.min, self.max, self.mean = np.float32(info.min), np.float32(info.max), float(info.mean)
        self.n_at_or_above, self.n_rise, self.n_fall = int(info.n_at_or_above), int(info.n_rise), int(info.n_fall)
        if samples is not None:
            self.time_s = np.arange(samples.size, dtype=np.float32) / self.rate
        else:
            P = int(info.n_columns)
            first = (np.arange(P, dtype=np.int64) * self.length) // max(P, 1)
            self.time_s = first / self.rate

    @property
    def duty_cycle(self) -> float:
        """Share of the chunk at or above the level."""
        return self.n_at_or_above / self.length if self.length else float("nan")

    @property
    def pulse_rate_hz(self) -> float:
        """Rising crossings per second of chunk."""
        return self.n_rise * self.rate / self.length if self.length else float("nan")


def _zs_input(samples):
    """(contiguous array, TDSA_IN_* format, sample count) of a host block: complex, interleaved int8 / uint8 pairs,
    real floats, or an [n, 2] stereo block (reduced with the reference's raw.mean(axis=1))."""
    a = np.asarray(samples)
    if a.dtype == np.int8 or a.dtype == np.uint8:
        a = np.ascontiguousarray(a.reshape(-1))
        if a.size % 2:
            raise ValueError("interleaved I/Q bytes of odd length")
        return a, nat.IN_I8 if a.dtype == np.int8 else nat.IN_U8, a.size // 2
    if a.ndim == 2:
        a = a.mean(axis=1)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a.reshape(-1), dtype=np.complex64)
        return a, nat.IN_C64, a.size
    a = np.ascontiguousarray(a.ravel().astype(np.float32))
    return a, nat.IN_F32R, a.size


class ZeroSpan(nat._Handle, nat._Timer):
    """Detector ring of the last `buffer_s` seconds on the device, and views of it."""
    _destroy = "tdsa_zspan_destroy"
    _timer = ("tdsa_zspan_timer_begin", "tdsa_zspan_timer_end")

    def __init__(self, sample_rate: float, window_s: float = 0.01, detector: str = "real",
                 decimation: Optional[int] = None, offset_hz: float = 0.0, taps=None, device: int = 0,
                 log_floor: float = 1e-12, offset_db: float = 0.0, buffer_s: float = BUFFER_SECONDS,
                 max_host_samples: int = 1 << 22):
        if detector not in DETECTORS:
            raise ValueError(f"detector={detector!r}: one of {sorted(DETECTORS)}")
        self.sample_rate = float(sample_rate)
        if not self.sample_rate > 0:
            raise ValueError(f"sample_rate={sample_rate}")
        self.window_s = float(window_s)
        self.device = int(device)
        self.decimation = None if decimation is None else int(decimation)
        self.max_host_samples = int(max_host_samples)
        self.rate = self.sample_rate if self.decimation is None else self.sample_rate / self.decimation
        self.capacity = int(float(buffer_s) * self.rate)
        if not MIN_CAPACITY <= self.capacity <= MAX_CAPACITY:
            raise ValueError(f"capacity={self.capacity} samples ({buffer_s} s at {self.rate} Hz): "
                             f"{MIN_CAPACITY} .. {MAX_CAPACITY}")
        self._h = C.c_void_p()
        self.ddc = self._engine = None
        self._d_in = self._d_y = None
        nat.check(nat.lib.tdsa_zspan_create(self.device, self.capacity, self.max_host_samples, C.byref(self._h)))
        self.detector = detector
        self.log_floor, self.offset_db = float(log_floor), float(offset_db)
        nat.check(nat.lib.tdsa_zspan_set_detector(self._h, DETECTORS[detector], self.log_floor, self.offset_db))
        if self.decimation is not None:
            # the tuned channel: converter, scratch and ring share one stream (a small plan lends it)
            self.ddc = DownConverter(self.decimation, self.sample_rate, offset_hz, taps, self.device, self.max_host_samples)
            self._engine = SpectrumEngine(64, max_frames=1, device=self.device)
            self._d_in = DeviceBuffer(8 * self.max_host_samples, self.device)
            self._y_cap = self.max_host_samples // self.decimation + 1
            self._d_y = DeviceBuffer(8 * self._y_cap, self.device)

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        nat._close_all(self, wait="_engine")
        super().close()                       # the ring: after the wait, before the scratch it was fed from
        nat._close_all(self, "_d_in", "_d_y", "ddc", "_engine")

    # ------------------------------------------------------------------ configuration
    @property
    def n_display(self) -> int:
        """max(int(window_s * rate), 4), as the reference."""
        return max(int(self.window_s * self.rate), 4)

    @property
    def offset_hz(self) -> float:
        return 0.0 if self.ddc is None else self.ddc.offset_hz

    def set_detector(self, detector: str, log_floor: Optional[float] = None, offset_db: Optional[float] = None) -> None:
        """Changes what the ring holds, so the history starts again."""
        if detector not in DETECTORS:
            raise ValueError(f"detector={detector!r}: one of {sorted(DETECTORS)}")
        self.log_floor = self.log_floor if log_floor is None else float(log_floor)
        self.offset_db = self.offset_db if offset_db is None else float(offset_db)
        nat.check(nat.lib.tdsa_zspan_set_detector(self._h, DETECTORS[detector], self.log_floor, self.offset_db))
        self.detector = detector
        if self.ddc is not None:
            self._engine.synchronize()
            self.ddc.reset()

    def reset(self) -> None:
        """Empty history; samples count from 0 again (and the converter's filter history and phase, if there is one)."""
        nat.check(nat.lib.tdsa_zspan_reset(self._h))
        if self.ddc is not None:
            self._engine.synchronize()
            self.ddc.reset()

    # ------------------------------------------------------------------ input
    def push(self, samples) -> int:
        """One host block.  Returns the number of values that went into the ring."""
        a, fmt, n = _zs_input(samples)
        if n == 0:
            return 0
        if self.ddc is None:
            nat.check(nat.lib.tdsa_zspan_push(self._h, fmt, a.ctypes.data_as(C.c_void_p), n))
            return n
        if fmt == nat.IN_F32R:
            raise ValueError("the tuned channel takes complex IQ (complex, or interleaved int8 / uint8 pairs)")
        bps = 8 if fmt == nat.IN_C64 else 2
        pushed = 0
        for s in range(0, n, self.max_host_samples):
            k = min(self.max_host_samples, n - s)
            part = np.ascontiguousarray(a[s:s + k] if fmt == nat.IN_C64 else a[2 * s:2 * (s + k)])
            nat.check(nat.lib.tdsa_plan_copy(self._engine._h, self._d_in.at(0, bps * k), part.ctypes.data_as(C.c_void_p),
                                             bps * k, 0))
            pushed += self._convert(self._engine, fmt, self._d_in.ptr, k)
        return pushed

    def _convert(self, engine, fmt: int, ptr: int, n: int) -> int:
        done = 0
        for s in range(0, n, self.max_host_samples):       # the scratch holds one block's outputs
            k = min(self.max_host_samples, n - s)
            bps = 8 if fmt == nat.IN_C64 else 2
            n_out = self.ddc.process_device(engine, fmt, ptr + bps * s, k, self._d_y.ptr)
            if n_out:
                nat.check(nat.lib.tdsa_zspan_push_dev(self._h, engine._h, nat.IN_C64, self._d_y.at(0, 8 * n_out), n_out))
            done += n_out
        return done

    def push_device(self, engine: Optional[SpectrumEngine], fmt: int, ptr: int, n: int) -> int:
        """Samples already in device memory, on `engine`'s stream after its work (None: the handle's own stream, or
        the tuned channel's); no host wait.  Returns the number of values that went into the ring."""
        if int(n) == 0:
            return 0
        if self.ddc is None:
            nat.check(nat.lib.tdsa_zspan_push_dev(self._h, engine._h if engine is not None else None, int(fmt),
                                                  C.c_void_p(int(ptr)), int(n)))
            return int(n)
        return self._convert(self._engine if engine is None else engine, int(fmt), int(ptr), int(n))

    # ------------------------------------------------------------------ output
    def view(self, mode: str = "free_run", level: float = 0.0, points: Optional[int] = None,
             column: str = "minmax", window_s: Optional[float] = None, n_display: Optional[int] = None) -> ZeroSpanView:
        """The display window (window_s, default the handle's; or n_display samples) free running or aligned to the
        last crossing of `level`; points=None: the raw chunk, otherwise min(points, length) columns of `column`."""
        if mode not in MODES:
            raise ValueError(f"mode={mode!r}: one of {sorted(MODES)}")
        if column not in COLUMNS:
            raise ValueError(f"column={column!r}: one of {sorted(COLUMNS)}")
        if n_display is None:
            n_display = self.n_display if window_s is None else max(int(float(window_s) * self.rate), 4)
        n_display = int(n_display)
        if not 1 <= n_display <= MAX_CAPACITY:
            raise ValueError(f"n_display={n_display}: 1 .. {MAX_CAPACITY}")
        n_points = 0 if points is None else int(points)
        if points is not None and not 1 <= n_points <= MAX_POINTS:
            raise ValueError(f"points={points}: 1 .. {MAX_POINTS}")
        rows = 2 if column == "minmax" else 1
        out = np.empty(min(n_display, self.capacity) if n_points == 0 else rows * n_points, dtype=np.float32)
        info = nat.ZspanInfo()
        nat.check(nat.lib.tdsa_zspan_view(self._h, MODES[mode], float(level), n_display, n_points, COLUMNS[column],
                                          C.byref(info), out.ctypes.data_as(C.c_void_p), None))
        if n_points == 0:
            return ZeroSpanView(info, self.rate, out[:info.length], None)
        P = int(info.n_columns)
        cols = out[:rows * P].reshape(rows, P) if rows == 2 else out[:P]
        return ZeroSpanView(info, self.rate, None, cols)
