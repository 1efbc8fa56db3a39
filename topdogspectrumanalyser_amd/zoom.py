"""Zoom spectra: digital down-conversion and decimation on the device.

A bench analyser's zoom: mix the region of interest at `offset_hz` down to 0 Hz, low-pass filter it, keep every D-th
sample, and take a short FFT of the slower stream.  The span becomes fs / D and the RBW fs / (D nfft).

  design_decimator  the default filter (Kaiser-windowed sinc, 34 taps per phase), built on the host like the windows
  DownConverter     unpack + NCO + mixer + polyphase FIR in one HIP pass (tdsa_ddc_*); history and state stay on the
                    device, so any split of the input into calls gives the same bits
  ZoomSpectrum      a DownConverter feeding a SpectrumEngine of nfft points through HBM: the existing averaging, holds,
                    calibration, tare and per-frame statistics work on the zoomed rows

The alias-free band is |f| <= 0.4 fs / D; aliases fold into the outer 20 % of the zoomed span (documented, not cropped).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat
from .analytics import _iq_input
from .devmem import DeviceBuffer
from .engine import SpectrumEngine
from .utils.constants import DSPConstants

MIN_DECIMATION, MAX_DECIMATION = 2, 4096
MAX_TAPS_PER_PHASE = 64
ALIAS_FREE_FRACTION = 0.4      # of the output rate: the passband edge of the default design
KAISER_BETA = 0.1102 * (100.0 - 8.7)


def design_decimator(decimation: int, taps_per_phase: int = 34) -> np.ndarray:
    """T = taps_per_phase * D float32 taps: sinc((i - (T-1)/2) / D) / D times a Kaiser window (beta for 100 dB),
    scaled in float64 to a sum of 1.  At 34 taps per phase: >= 100 dB beyond 0.6 fs/D, <= 0.001 dB ripple within
    0.4 fs/D for every D in 2 .. 4096."""
    D = int(decimation)
    if not MIN_DECIMATION <= D <= MAX_DECIMATION:
        raise ValueError(f"decimation={D}: {MIN_DECIMATION} .. {MAX_DECIMATION}")
    if not 1 <= int(taps_per_phase) <= MAX_TAPS_PER_PHASE:
        raise ValueError(f"taps_per_phase={taps_per_phase}: 1 .. {MAX_TAPS_PER_PHASE}")
    T = int(taps_per_phase) * D
    i = np.arange(T, dtype=np.float64)
    h = np.sinc((i - (T - 1) / 2.0) / D) / D * np.kaiser(T, KAISER_BETA)
    h /= h.sum()
    return h.astype(np.float32)


def nco_step(offset_hz: float, sample_rate: float):
    """(uint32 phase step, actual offset in Hz): step = round(f 2^32 / fs) mod 2^32, actual = round(...) fs / 2^32.
    |offset_hz| <= fs / 2."""
    fs = float(sample_rate)
    f = float(offset_hz)
    if not fs > 0:
        raise ValueError(f"sample_rate={sample_rate}")
    if not abs(f) <= fs / 2:
        raise ValueError(f"offset {f} Hz is outside +-fs/2 = +-{fs / 2} Hz")
    k = int(round(f * 2.0 ** 32 / fs))
    return k % (1 << 32), k * fs / 2.0 ** 32


def zoom_freq_bins(nfft: int, decimation: int, sample_rate: float, centre_freq: float = 0.0,
                   offset_hz: float = 0.0) -> np.ndarray:
    """fftshift(fftfreq(nfft, D / fs)) + centre_freq + offset_hz: the axis of a zoomed row."""
    return np.fft.fftshift(np.fft.fftfreq(int(nfft), int(decimation) / float(sample_rate))) + centre_freq + offset_hz


def alias_free_bins(nfft: int, decimation: int, sample_rate: float) -> slice:
    """The bins of a zoomed row within +-0.4 fs / D of the zoom centre."""
    fb = zoom_freq_bins(nfft, decimation, sample_rate)
    idx = np.nonzero(np.abs(fb) <= ALIAS_FREE_FRACTION * float(sample_rate) / int(decimation))[0]
    return slice(int(idx[0]), int(idx[-1]) + 1)


def as_taps(taps) -> np.ndarray:
    """A filter as the library takes it: contiguous float32 [T], every tap finite."""
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
    if not np.all(np.isfinite(h)):
        raise ValueError("taps must be finite")
    return h


def outputs_completed(n_total: int, n_in: int, decimation: int) -> int:
    """Outputs (per channel) a call delivering n_in inputs completes after n_total earlier ones, one output per D inputs:
    output m comes out of the call that delivers input m D."""
    D = int(decimation)
    return -(-(int(n_total) + int(n_in)) // D) - (-(-int(n_total) // D))


def check_same_device(engine_device: int, device: int) -> None:
    """A handle launches on the stream of an engine of its own device only."""
    if int(engine_device) != int(device):
        raise ValueError(f"engine on device {engine_device}, handle on device {device}")


class DownConverter(nat._Handle):
    """Mixes `offset_hz` to 0 Hz and decimates by `decimation` (complex64 out, one output per D inputs)."""
    _destroy = "tdsa_ddc_destroy"

    def __init__(self, decimation: int, sample_rate: float, offset_hz: float = 0.0, taps=None, device: int = 0,
                 max_host_samples: int = 1 << 22):
        self.decimation = int(decimation)
        self.sample_rate = float(sample_rate)
        self.device = int(device)
        self.max_host_samples = int(max_host_samples)
        self.taps = design_decimator(self.decimation) if taps is None else as_taps(taps)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_ddc_create(self.device, self.decimation, int(self.taps.size), self.max_host_samples,
                                          C.byref(self._h)))
        nat.check(nat.lib.tdsa_ddc_set_taps(self._h, self.taps.ctypes.data_as(C.c_void_p), int(self.taps.size)))
        self.phase_step = 0
        self.offset_hz = 0.0
        self.set_offset(offset_hz)

    # ------------------------------------------------------------------ configuration
    @property
    def output_rate(self) -> float:
        return self.sample_rate / self.decimation

    @property
    def alias_free_hz(self) -> float:
        return ALIAS_FREE_FRACTION * self.output_rate

    @property
    def first_full_output(self) -> int:
        """m0 = ceil((T-1) / D): the first output whose filter window lies entirely in delivered input."""
        return -(-(int(self.taps.size) - 1) // self.decimation)

    def set_offset(self, offset_hz: float) -> float:
        """Retune (the phase stays continuous); returns the actual, quantised offset."""
        step, actual = nco_step(offset_hz, self.sample_rate)
        nat.check(nat.lib.tdsa_ddc_set_nco(self._h, step))
        self.phase_step, self.offset_hz = step, actual
        return actual

    def reset(self) -> None:
        """History and phase to zero (inputs count from 0 again); the offset is kept."""
        nat.check(nat.lib.tdsa_ddc_reset(self._h))

    # ------------------------------------------------------------------ processing
    def process(self, iq) -> np.ndarray:
        """One host block (complex, or interleaved int8 / uint8 pairs): the outputs it completes, complex64."""
        a, fmt, n = _iq_input(iq, None)
        outs = []
        for s in range(0, max(n, 1), self.max_host_samples):
            k = min(self.max_host_samples, n - s)
            part = a[s:s + k] if fmt == nat.IN_C64 else a[2 * s:2 * (s + k)]
            out = np.empty(k // self.decimation + 1, dtype=np.complex64)
            n_out = C.c_size_t()
            nat.check(nat.lib.tdsa_ddc_process(self._h, fmt, part.ctypes.data_as(C.c_void_p), k,
                                               out.ctypes.data_as(C.c_void_p), C.byref(n_out)))
            outs.append(out[:n_out.value])
        return outs[0] if len(outs) == 1 else np.concatenate(outs)

    def process_device(self, engine: Optional[SpectrumEngine], fmt: int, ptr: int, n_in: int, out_ptr: int) -> int:
        """Input and output in device memory, on `engine`'s stream (None: the handle's own), no host wait.
        Returns the number of outputs written at out_ptr."""
        n_out = C.c_size_t()
        nat.check(nat.lib.tdsa_ddc_process_dev(self._h, engine._h if engine is not None else None, int(fmt),
                                               C.c_void_p(ptr), int(n_in), C.c_void_p(out_ptr) if out_ptr else None,
                                               C.byref(n_out)))
        return int(n_out.value)


def zoom_window(nfft: int) -> np.ndarray:
    """The HackRF source's window: symmetric Hann, float32, unit mean power."""
    w = np.hanning(int(nfft)).astype(np.float32)
    w /= np.sqrt(np.mean(w ** 2))
    return w


class ZoomSpectrum(nat._Handle):
    """Spectra of the band offset_hz +- fs / (2 D) at RBW fs / (D nfft).  Frame k is y[m0 + k hop : m0 + k hop + nfft]
    of the decimated stream; framing continues across calls, and decimated samples not yet framed stay on the device.

    `.engine` is the SpectrumEngine the rows come from (configure, hold, averaged, frame_stats work as usual).  DC
    removal is off: the zoomed DC is the signal at the zoom centre."""

    def __init__(self, sample_rate: float, decimation: int, nfft: int, offset_hz: float = 0.0, hop: Optional[int] = None,
                 taps=None, window=None, device: int = 0, max_host_samples: int = 1 << 22):
        self.nfft = int(nfft)
        self.hop = self.nfft if hop is None else int(hop)
        if self.hop < 1:
            raise ValueError(f"hop={hop}")
        self.device = int(device)
        self.ddc = DownConverter(decimation, sample_rate, offset_hz, taps, device, max_host_samples)
        self.max_host_samples = int(max_host_samples)
        max_out = self.max_host_samples // self.ddc.decimation + 1
        self._rows_cap = max_out // self.hop + 1          # frames one host call can complete
        self.engine = SpectrumEngine(self.nfft, max_frames=min(self._rows_cap, 256), device=self.device)
        self.engine.set_window(zoom_window(self.nfft) if window is None else window)
        self.engine.configure(db_mode="mag", log_floor=DSPConstants.LOG_FLOOR, dc_alpha=-1.0)
        self._y_cap = 0
        self._y = []
        self._restart()
        self._grow(self.nfft + max_out)
        self._d_in = DeviceBuffer(8 * self.max_host_samples, self.device)
        self._d_rows = DeviceBuffer(4 * self._rows_cap * self.nfft, self.device)

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        nat._close_all(self, "_y", "_d_in", "_d_rows", "ddc", "engine", wait="engine")

    # ------------------------------------------------------------------ axis
    @property
    def decimation(self) -> int:
        return self.ddc.decimation

    @property
    def sample_rate(self) -> float:
        return self.ddc.sample_rate

    @property
    def offset_hz(self) -> float:
        return self.ddc.offset_hz

    @property
    def output_rate(self) -> float:
        return self.ddc.output_rate

    @property
    def rbw(self) -> float:
        return self.sample_rate / (self.decimation * self.nfft)

    def freq_bins(self, centre_freq: float = 0.0) -> np.ndarray:
        return zoom_freq_bins(self.nfft, self.decimation, self.sample_rate, centre_freq, self.offset_hz)

    @property
    def alias_free(self) -> slice:
        """The bins within +-0.4 fs / D of the zoom centre."""
        return alias_free_bins(self.nfft, self.decimation, self.sample_rate)

    # ------------------------------------------------------------------ state
    def _restart(self) -> None:
        self._cur = 0
        self._base = 0                        # absolute output index of _y[_cur][0]
        self._pending = 0                     # outputs held there
        self._next = self.ddc.first_full_output   # absolute index of the next frame's first output
        self._inputs = 0                      # inputs delivered since the last reset

    def set_offset(self, offset_hz: float) -> float:
        """Retune; the phase stays continuous and framing goes on."""
        return self.ddc.set_offset(offset_hz)

    def reset(self) -> None:
        """Down-converter history, phase and framing from the start; the engine's averaging, holds and DC state too."""
        self.engine.synchronize()
        self.ddc.reset()
        self.engine.reset()
        self._restart()

    def hold(self):
        return self.engine.hold()

    def frames_completed_by(self, n_in: int) -> int:
        """Frames a call delivering n_in more inputs would complete."""
        end = -(-(self._inputs + int(n_in)) // self.decimation)
        return 0 if end - self._next < self.nfft else (end - self._next - self.nfft) // self.hop + 1

    # ------------------------------------------------------------------ processing
    def _grow(self, need: int) -> None:
        if need <= self._y_cap:
            return
        cap = max(need, 2 * self._y_cap)
        new = [DeviceBuffer(8 * cap, self.device), DeviceBuffer(8 * cap, self.device)]
        if self._y_cap:
            if self._pending:
                nat.check(nat.lib.tdsa_plan_copy(self.engine._h, new[self._cur].ptr,
                                                 self._y[self._cur].at(0, 8 * self._pending), 8 * self._pending, 0))
            self.engine.synchronize()
            for old in self._y:
                old.close()
        self._y, self._y_cap = new, cap

    def _run(self, fmt: int, ptr: int, n_in: int, rows_ptr: int) -> int:
        """DDC onto the pending outputs, frames of everything complete, the unframed tail to the other buffer."""
        D = self.decimation
        total = self._inputs + int(n_in)
        n_new = outputs_completed(self._inputs, n_in, D)
        self._grow(self._pending + n_new)
        y = self._y[self._cur]
        n_out = self.ddc.process_device(self.engine, fmt, ptr, n_in, y.at(8 * self._pending, 8 * n_new))
        self._inputs = total
        end = self._base + self._pending + n_out
        nf = 0 if end - self._next < self.nfft else (end - self._next - self.nfft) // self.hop + 1
        done = 0
        while done < nf:
            k = min(self.engine.max_frames, nf - done)
            start = self._next + done * self.hop
            n_frame = (k - 1) * self.hop + self.nfft
            self.engine.process_device(nat.IN_C64, y.at(8 * (start - self._base), 8 * n_frame), n_frame,
                                       self.hop, k, rows_ptr + 4 * done * self.nfft if rows_ptr else None)
            done += k
        self._next += nf * self.hop
        keep_from = min(self._next, end)
        keep = end - keep_from
        other = self._y[self._cur ^ 1]
        if keep:
            nat.check(nat.lib.tdsa_plan_copy(self.engine._h, other.at(0, 8 * keep),
                                             y.at(8 * (keep_from - self._base), 8 * keep), 8 * keep, 0))
        self._cur ^= 1
        self._base, self._pending = keep_from, keep
        return nf

    def process(self, iq) -> np.ndarray:
        """Host IQ in (complex, or interleaved int8 / uint8 pairs): [frames, nfft] float32 dB rows of the frames this
        call completed (one host wait per max_host_samples block)."""
        a, fmt, n = _iq_input(iq, None)
        bps = 8 if fmt == nat.IN_C64 else 2
        rows = []
        for s in range(0, n, self.max_host_samples):
            k = min(self.max_host_samples, n - s)
            part = np.ascontiguousarray(a[s:s + k] if fmt == nat.IN_C64 else a[2 * s:2 * (s + k)])
            nat.check(nat.lib.tdsa_plan_copy(self.engine._h, self._d_in.at(0, bps * k), part.ctypes.data_as(C.c_void_p),
                                             bps * k, 0))
            nf = self._run(fmt, self._d_in.ptr, k, self._d_rows.ptr)
            out = np.empty((nf, self.nfft), dtype=np.float32)
            nat.check(nat.lib.tdsa_plan_copy(self.engine._h, out.ctypes.data_as(C.c_void_p),
                                             self._d_rows.at(0, out.nbytes), out.nbytes, 1))
            rows.append(out)
        if not rows:
            return np.empty((0, self.nfft), dtype=np.float32)
        return rows[0] if len(rows) == 1 else np.concatenate(rows)

    def process_device(self, fmt: int, ptr: int, n_in: int, out_db_dev: Optional[int]) -> int:
        """Raw IQ already on the device (ptr, n_in samples): dB rows of the completed frames to out_db_dev (room for
        frames_completed_by(n_in) rows, or None), asynchronous on the engine's stream.  Returns the frame count."""
        return self._run(int(fmt), int(ptr), int(n_in), int(out_db_dev) if out_db_dev else 0)
