"""Stepped sweeps: one IQ capture per tuning step, stitched into one trace on the device.

A span wider than the sample rate, the way hackrf_sweep and rtl_power make one: retune, capture a block, window and
FFT it, keep the clean middle of each step, lay the steps side by side, resample onto a fixed grid.  The frames are the
ordinary SpectrumEngine's; what this module adds is what comes after them, without the rows leaving the device:

  plan_steps         tuning centres, kept bin range and bin width that cover [start, stop] with abutting kept ranges
  SweepAssembler     step detector (sample / max / min / avg over a step's frames) and stitch (np.interp onto the grid,
                     or the peak of each grid cell) behind tdsa_sweep_*
  IqSweepDataSource  a SweepDataSource with the reference's shape (datasources/hackrf_sweep.py): `capture(centre_hz,
                     n_samples)` is its only contact with hardware - a tuner, a replay file or a synthetic scene
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from typing import Callable, Optional, Tuple

import numpy as np

from . import _native as nat
from .datasources.base import SweepDataSource
from .devmem import DeviceBuffer
from .engine import SpectrumEngine
from .utils.constants import DSPConstants
from .zoom import zoom_window

MAX_STEPS = 4096
DETECTORS = {"sample": nat.SWEEP_DET_SAMPLE, "max": nat.SWEEP_DET_MAX, "min": nat.SWEEP_DET_MIN,
             "avg": nat.SWEEP_DET_AVG}
MODES = {"interp": nat.SWEEP_INTERP, "peak": nat.SWEEP_PEAK}
_FORMATS = {"i8": nat.IN_I8, "u8": nat.IN_U8, "c64": nat.IN_C64}


def plan_steps(start_hz: float, stop_hz: float, sample_rate: float, nfft: int, keep: float = 0.75
               ) -> Tuple[np.ndarray, Tuple[int, int], float]:
    """(centres[S] float64, (k0, k1), bin_hz) of a sweep over [start_hz, stop_hz] with captures of `sample_rate`.

    bin_hz = 1.0 / (nfft * (1.0 / fs)); K = the largest even number <= keep * nfft bins are kept of every step, centred
    on bin nfft / 2 (the tuning centre); the step is K * bin_hz, so the kept ranges abut: step s holds the bins at
    start + (s K + j) bin_hz, j < K, and S = ceil((stop - start) / step) steps hold every bin below stop."""
    fs, N = float(sample_rate), int(nfft)
    start, stop = float(start_hz), float(stop_hz)
    if not (fs > 0 and N >= 2 and N % 2 == 0):
        raise ValueError(f"sample_rate={sample_rate}, nfft={nfft}: a positive rate and an even frame length")
    if not stop > start:
        raise ValueError(f"stop {stop} Hz is not above start {start} Hz")
    if not 0.0 < keep <= 1.0:
        raise ValueError(f"keep={keep}: a fraction of the frame, (0, 1]")
    bin_hz = 1.0 / (N * (1.0 / fs))
    K = max(2, int(keep * N) // 2 * 2)
    k0 = N // 2 - K // 2
    step = K * bin_hz
    S = max(1, int(np.ceil((stop - start) / step - 1e-9)))
    if S > MAX_STEPS:
        raise ValueError(f"{S} steps of {step} Hz: at most {MAX_STEPS} (raise the sample rate or narrow the span)")
    centres = start + (np.arange(S, dtype=np.float64) + 0.5) * step
    return centres, (k0, k0 + K), bin_hz


def step_frequencies(centres, k0: int, k1: int, nfft: int, bin_hz: float) -> np.ndarray:
    """xp: the frequency of every kept bin, step after step: centre + (k - nfft / 2) * bin_hz, a multiply then an add."""
    k = (np.arange(int(k0), int(k1)) - int(nfft) // 2).astype(np.float64) * float(bin_hz)
    return (np.asarray(centres, dtype=np.float64)[:, None] + k[None, :]).reshape(-1)


def check_geometry(centres, k0: int, k1: int, nfft: int, bin_hz: float) -> None:
    """What tdsa_sweep_set_geometry demands, with its expression: 0 <= k0 < k1 <= nfft, a positive bin width, finite
    centres, and the last kept bin of every step strictly below the first of the next (ValueError otherwise)."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1)
    if not (0 <= int(k0) < int(k1) <= int(nfft)):
        raise ValueError(f"kept range [{k0}, {k1}): 0 <= k0 < k1 <= nfft = {nfft}")
    if not (np.isfinite(bin_hz) and bin_hz > 0):
        raise ValueError(f"bin_hz={bin_hz}: positive and finite")
    if not 1 <= c.size <= MAX_STEPS or not np.all(np.isfinite(c)):
        raise ValueError(f"{c.size} centres: 1 .. {MAX_STEPS} finite values")
    first = c + float(int(k0) - int(nfft) // 2) * float(bin_hz)
    last = c + float(int(k1) - 1 - int(nfft) // 2) * float(bin_hz)
    bad = np.nonzero(~(last[:-1] < first[1:]))[0]
    if bad.size:
        s = int(bad[0])
        raise ValueError(f"steps {s} and {s + 1}: the last kept bin of one ({last[s]!r} Hz) is not below the first of "
                         f"the next ({first[s + 1]!r} Hz) - centres must ascend and kept ranges must not overlap")


def frequency_grid(start_hz: float, stop_hz: float, bin_size: float) -> np.ndarray:
    """The reference's fixed grid (HackRFSweepDataSource._create_frequency_grid)."""
    return np.linspace(start_hz, stop_hz, int((stop_hz - start_hz) / bin_size))


class SweepAssembler(nat._Handle, nat._Timer):
    """Detector and stitch of one sweep geometry (tdsa_sweep_*): T[steps][K] and the flags of the steps present stay on
    the device between calls."""
    _destroy = "tdsa_sweep_destroy"
    _timer = ("tdsa_sweep_timer_begin", "tdsa_sweep_timer_end")

    def __init__(self, nfft: int, centres, kept: Tuple[int, int], bin_hz: float, grid, device: int = 0):
        self.nfft = int(nfft)
        self.device = int(device)
        self.centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        self.grid = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
        self.k0, self.k1 = int(kept[0]), int(kept[1])
        self.bin_hz = float(bin_hz)
        self._h = None
        check_geometry(self.centres, self.k0, self.k1, self.nfft, self.bin_hz)
        if not (self.grid.size >= 2 and np.all(np.isfinite(self.grid))):
            raise ValueError("the grid needs at least two points, all finite")
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_sweep_create(self.device, self.nfft, int(self.centres.size), int(self.grid.size),
                                            C.byref(self._h)))
        try:
            nat.check(nat.lib.tdsa_sweep_set_geometry(self._h, self.centres.ctypes.data_as(C.c_void_p), self.bin_hz,
                                                      self.k0, self.k1, self.grid.ctypes.data_as(C.c_void_p)))
        except Exception:
            self.close()
            raise

    # ------------------------------------------------------------------ geometry
    @property
    def n_steps(self) -> int:
        return int(self.centres.size)

    @property
    def kept_bins(self) -> int:
        return self.k1 - self.k0

    def frequencies(self) -> np.ndarray:
        return step_frequencies(self.centres, self.k0, self.k1, self.nfft, self.bin_hz)

    def reset(self) -> None:
        """No step is present any more (a read gives NaN until the next update)."""
        nat.check(nat.lib.tdsa_sweep_reset(self._h))

    def set_chunk_bytes(self, nbytes: int) -> None:
        """Bound of the row scratch run_device works through (default 256 MiB; at least one step is always taken)."""
        nat.check(nat.lib.tdsa_sweep_set_chunk_bytes(self._h, int(nbytes)))

    # ------------------------------------------------------------------ processing
    def update_device(self, engine: Optional[SpectrumEngine], first_step: int, n_steps: int, rows_dev: int,
                      frames_per_step: int, detector: str = "avg", step_stride_floats: int = 0) -> None:
        """dB rows already on the device ([steps][frames][nfft] at rows_dev) into T, on `engine`'s stream (None: the
        handle's own), no host wait."""
        nat.check(nat.lib.tdsa_sweep_update_dev(self._h, engine._h if engine is not None else None, int(first_step),
                                                int(n_steps), C.c_void_p(rows_dev), int(frames_per_step),
                                                int(step_stride_floats), DETECTORS[detector]))

    def run_device(self, engine: SpectrumEngine, in_format: int, iq_dev: int, step_stride_bytes: int, first_step: int,
                   n_steps: int, n_samples_per_step: int, hop: int, frames_per_step: int,
                   detector: str = "avg") -> None:
        """Raw captures on the device, one per step: the engine's frames, then the detector; no host wait."""
        nat.check(nat.lib.tdsa_sweep_run_dev(self._h, engine._h, int(in_format), C.c_void_p(iq_dev),
                                             int(step_stride_bytes), int(first_step), int(n_steps),
                                             int(n_samples_per_step), int(hop), int(frames_per_step),
                                             DETECTORS[detector]))

    def read(self, mode: str = "interp", out_dev: Optional[int] = None, to_host: bool = True) -> Optional[np.ndarray]:
        """The stitched trace on the grid, float64 (waits); with to_host = False it only goes to out_dev, no wait."""
        out = np.empty(self.grid.size, dtype=np.float64) if to_host else None
        nat.check(nat.lib.tdsa_sweep_read(self._h, MODES[mode], out.ctypes.data_as(C.c_void_p) if to_host else None,
                                          C.c_void_p(out_dev) if out_dev else None))
        return out

    def steps(self) -> Tuple[np.ndarray, np.ndarray]:
        """(T[steps][K] float32, present[steps] bool)."""
        T = np.empty((self.n_steps, self.kept_bins), dtype=np.float32)
        valid = np.empty(self.n_steps, dtype=np.uint8)
        nat.check(nat.lib.tdsa_sweep_get_steps(self._h, T.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)))
        return T, valid.astype(bool)


class IqSweepDataSource(nat._Handle, SweepDataSource):
    """Sweeps [start_freq, stop_freq] by retuning: `capture(centre_hz, n_samples)` returns one block of IQ per step
    (complex, or interleaved int8 / uint8 pairs, as in_format says), the steps' rows are made by `.engine` (window, dB
    mode, PSD scale, calibration and DC removal are set there, as on any SpectrumEngine) and stitched onto the
    reference's grid of `bin_size` Hz.  get_data() is the last complete sweep, NaN before the first."""

    def __init__(self, start_freq: float, stop_freq: float, bin_size: float, *,
                 capture: Callable[[float, int], np.ndarray], sample_rate: float, nfft: int = 8192,
                 frames_per_step: int = 1, hop: Optional[int] = None, detector: str = "avg", keep: float = 0.75,
                 in_format="c64", device: int = 0):
        self.start_freq = int(start_freq)
        self.stop_freq = int(stop_freq)
        self.bin_size = int(bin_size)
        self.capture = capture
        self.sample_rate = float(sample_rate)
        self.nfft = int(nfft)
        self.frames_per_step = int(frames_per_step)
        self.hop = self.nfft if hop is None else int(hop)
        if self.frames_per_step < 1 or self.hop < 1:
            raise ValueError(f"frames_per_step={frames_per_step}, hop={hop}")
        if detector not in DETECTORS:
            raise ValueError(f"detector={detector!r}: one of {sorted(DETECTORS)}")
        self.detector, self.keep = detector, float(keep)
        self.mode = "interp"                           # the reference's stitch; "peak" for grids coarser than the bins
        self.in_format = _FORMATS[in_format] if isinstance(in_format, str) else int(in_format)
        self.device = int(device)
        self.n_samples_per_step = (self.frames_per_step - 1) * self.hop + self.nfft
        self.is_running = False
        self.sweep_rate = None                         # sweeps per second, measured
        self.sweep_count = 0
        self.last_data_time = 0.0
        self.lock = threading.Lock()
        self.thread: Optional[threading.Thread] = None
        self.engine = SpectrumEngine(self.nfft, max_frames=self.frames_per_step, device=self.device)
        self.engine.set_window(zoom_window(self.nfft))
        self.engine.configure(db_mode="mag", log_floor=DSPConstants.LOG_FLOOR, dc_alpha=-1.0)
        self.assembler: Optional[SweepAssembler] = None
        self._d_in = None
        self._plan()

    # ------------------------------------------------------------------ planning
    def _create_frequency_grid(self) -> None:
        self.frequency_grid = frequency_grid(self.start_freq, self.stop_freq, self.bin_size)
        self.full_power_array = np.full(self.frequency_grid.size, np.nan)

    def _plan(self) -> None:
        """Grid, steps and device buffers for the current range."""
        self._create_frequency_grid()
        self.centres, self.kept, self.bin_hz = plan_steps(self.start_freq, self.stop_freq, self.sample_rate, self.nfft,
                                                          self.keep)
        self._release()
        self.assembler = SweepAssembler(self.nfft, self.centres, self.kept, self.bin_hz, self.frequency_grid, self.device)
        S = self.centres.size
        if self.in_format == nat.IN_C64:
            self._stage = np.zeros((S, self.n_samples_per_step), dtype=np.complex64)
        else:
            self._stage = np.zeros((S, 2 * self.n_samples_per_step),
                                   dtype=np.int8 if self.in_format == nat.IN_I8 else np.uint8)
        self._d_in = DeviceBuffer(self._stage.nbytes, self.device)

    def _release(self) -> None:
        if self.assembler is not None:
            self.engine.synchronize()
        nat._close_all(self, "assembler", "_d_in")
        self.assembler = self._d_in = None

    # ------------------------------------------------------------------ SweepDataSource
    def start(self, frequency=None):
        if self.is_running:
            self.stop()
        if frequency:
            self.start_freq = int(frequency.start)
            self.stop_freq = int(frequency.stop)
            self._plan()
        self.is_running = True
        self.sweep_rate = None
        self.thread = threading.Thread(target=self._sweep_loop, name="iq-sweep", daemon=True)
        self.thread.start()

    def _sweep_loop(self) -> None:
        try:
            while self.is_running:
                self.sweep_once()
        finally:
            self.is_running = False

    def stop(self):
        self.is_running = False
        t, self.thread = self.thread, None
        if t is not None and t.is_alive() and t is not threading.current_thread():
            t.join()

    def close(self) -> None:
        self.stop()
        if getattr(self, "engine", None) is not None and self.engine._h:
            self._release()
            self.engine.close()

    def sweep_once(self) -> np.ndarray:
        """One sweep, synchronously: a capture per step into one staging buffer, one copy, one run_device, one read."""
        t0 = time.monotonic()
        for s, c in enumerate(self.centres):
            block = np.asarray(self.capture(float(c), self.n_samples_per_step)).reshape(-1)
            if block.size != self._stage.shape[1]:
                raise ValueError(f"capture returned {block.size} values for step {s}, {self._stage.shape[1]} expected")
            self._stage[s] = block
        eng, asm = self.engine, self.assembler
        nat.check(nat.lib.tdsa_plan_copy(eng._h, self._d_in.at(0, self._stage.nbytes),
                                         self._stage.ctypes.data_as(C.c_void_p), self._stage.nbytes, 0))
        asm.run_device(eng, self.in_format, self._d_in.ptr, self._stage.strides[0], 0, self.centres.size,
                       self.n_samples_per_step, self.hop, self.frames_per_step, self.detector)
        trace = asm.read(self.mode)
        dt = time.monotonic() - t0
        with self.lock:
            self.full_power_array = trace
            self.sweep_count += 1
            self.sweep_rate = 1.0 / dt if dt > 0 else None
        self.last_data_time = time.monotonic()
        return trace

    def get_data(self):
        with self.lock:
            return self.full_power_array.copy()

    def get_number_of_points(self):
        with self.lock:
            return len(self.full_power_array)
