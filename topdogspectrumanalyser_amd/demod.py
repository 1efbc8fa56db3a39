"""Analog demodulation on the device: AM / FM audio, deviation, depth.

The consumer of the complex64 streams zoom.DownConverter and channelizer.Channelizer leave in HBM: per channel an FM
discriminator (phase step per sample, in half turns) or an AM one (the envelope), a real decimating FIR to the audio
rate, a one-pole section (FM de-emphasis as a low-pass, AM carrier removal as a high-pass) and a scale, in one HIP pass
(tdsa_demod_*).  Filter history and pole state stay on the device: any split of the input into calls gives the same
bits.  The same pass accumulates count, max, min, sum and sum of squares of the filtered discriminator per channel, from
which measure() reads FM offset and deviation or AM carrier level and depth.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as nat
from .engine import SpectrumEngine
from .zoom import as_taps, check_same_device, design_decimator, outputs_completed

MAX_CHANNELS = 256
MAX_DECIMATION = 64
MAX_TAPS_PER_PHASE = 64
MODES = {"fm": nat.DEMOD_FM, "am": nat.DEMOD_AM}


def design_audio_filter(decimation: int) -> np.ndarray:
    """The default audio filter: [1.0] at R = 1, otherwise zoom.design_decimator(R) - 34 taps per phase, sum 1, flat to
    0.4 f_i / R and >= 100 dB down beyond 0.6 f_i / R."""
    R = int(decimation)
    if not 1 <= R <= MAX_DECIMATION:
        raise ValueError(f"decimation={decimation}: 1 .. {MAX_DECIMATION}")
    return np.ones(1, dtype=np.float32) if R == 1 else design_decimator(R)


def deemphasis_pole(tau_s: float, audio_rate: float) -> float:
    """c = exp(-1 / (audio_rate tau)): the pole of an RC de-emphasis of time constant tau (75e-6 or 50e-6 s)."""
    if not (float(tau_s) > 0 and float(audio_rate) > 0):
        raise ValueError(f"tau_s={tau_s}, audio_rate={audio_rate}: both positive")
    return math.exp(-1.0 / (float(audio_rate) * float(tau_s)))


def check_parameters(mode, channels: int, decimation: int, n_taps: int, pole: float = 0.0) -> int:
    """The library's own rules, raised as ValueError before anything touches a device.  Returns the mode's number."""
    key = mode.lower() if isinstance(mode, str) else mode
    if key in MODES:
        key = MODES[key]
    if key not in (nat.DEMOD_FM, nat.DEMOD_AM):
        raise ValueError(f"mode={mode!r}: 'fm' or 'am'")
    if not 1 <= int(channels) <= MAX_CHANNELS:
        raise ValueError(f"channels={channels}: 1 .. {MAX_CHANNELS}")
    R = int(decimation)
    if not 1 <= R <= MAX_DECIMATION:
        raise ValueError(f"decimation={decimation}: 1 .. {MAX_DECIMATION}")
    if not 1 <= int(n_taps) <= MAX_TAPS_PER_PHASE * R:
        raise ValueError(f"{n_taps} taps: 1 .. {MAX_TAPS_PER_PHASE * R} ({MAX_TAPS_PER_PHASE} per phase at decimation {R})")
    if not 0.0 <= float(pole) < 1.0:
        raise ValueError(f"pole c={pole}: 0 <= c < 1")
    return int(key)


def check_call(n_in: int, in_stride: int, ptr: int, n_out: int, out_stride: int, out_ptr: int) -> None:
    """A call's placement: channel c's input at ptr + 8 c in_stride, its outputs at out_ptr + 4 c out_stride."""
    if int(n_in) < 0:
        raise ValueError(f"n_in={n_in}")
    if int(in_stride) < int(n_in):
        raise ValueError(f"in_stride={in_stride}: below the call's {n_in} samples per channel")
    if int(out_stride) < int(n_out):
        raise ValueError(f"out_stride={out_stride}: the call completes {n_out} outputs per channel")
    if int(ptr) % 8:
        raise ValueError("input pointer must be aligned to one complex64 sample (8 bytes)")
    if int(out_ptr) % 4:
        raise ValueError("output pointer must be aligned to one float32 (4 bytes)")
    if int(n_in) > 0 and not ptr:
        raise ValueError("null input pointer")
    if int(n_out) > 0 and not out_ptr:
        raise ValueError("null output pointer")


@dataclass
class Measurement:
    """Per channel, over the filtered discriminator a[m] since reset_measure(): the raw arrays and what they say.
    FM (all in Hz, a[m] scaled by f_i / 2): offset_hz = mean, peak_plus_hz = max - mean, peak_minus_hz = mean - min,
    rms_hz = deviation about the mean.  AM: carrier = mean, depth = (max - min) / (max + min).  Channels that have
    seen no output hold NaN."""
    mode: str
    count: np.ndarray
    max: np.ndarray
    min: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray
    mean: np.ndarray
    rms: np.ndarray                   # about the mean
    offset_hz: Optional[np.ndarray] = None
    peak_plus_hz: Optional[np.ndarray] = None
    peak_minus_hz: Optional[np.ndarray] = None
    rms_hz: Optional[np.ndarray] = None
    carrier: Optional[np.ndarray] = None
    depth: Optional[np.ndarray] = None


def derive(mode: str, input_rate: float, count, mx, mn, s, ss) -> Measurement:
    """The derived figures from the five raw arrays (also what the tests apply to the contract's arrays)."""
    count = np.asarray(count, dtype=np.int64)
    mx64, mn64 = np.asarray(mx, dtype=np.float64), np.asarray(mn, dtype=np.float64)
    s, ss = np.asarray(s, dtype=np.float64), np.asarray(ss, dtype=np.float64)
    with np.errstate(all="ignore"):
        n = np.where(count > 0, count, 1).astype(np.float64)
        none = count == 0
        mean = np.where(none, np.nan, s / n)
        rms = np.where(none, np.nan, np.sqrt(np.maximum(ss / n - (s / n) ** 2, 0.0)))
        m = Measurement(mode, count, np.asarray(mx), np.asarray(mn), s, ss, mean, rms)
        if mode == "fm":
            k = float(input_rate) / 2.0
            m.offset_hz = k * mean
            m.peak_plus_hz = np.where(none, np.nan, k * (mx64 - mean))
            m.peak_minus_hz = np.where(none, np.nan, k * (mean - mn64))
            m.rms_hz = k * rms
        else:
            m.carrier = mean
            m.depth = np.where(none | (mx64 + mn64 <= 0), np.nan, (mx64 - mn64) / np.where(mx64 + mn64 > 0, mx64 + mn64, 1.0))
    return m


class Demodulator(nat._Handle, nat._Timer):
    """AM / FM demodulation of `channels` complex64 streams at input_rate into float32 audio at input_rate / decimation.

    taps: the audio filter (default design_audio_filter(decimation)).  deemphasis: time constant in seconds of a
    low-pass one-pole section (FM: 75e-6 or 50e-6).  remove_carrier: a high-pass one-pole section (AM: the output is the
    envelope minus its slow mean); its time constant is `deemphasis` if given, else 10 ms.  scale: applied last."""
    _destroy = "tdsa_demod_destroy"
    _timer = ("tdsa_demod_timer_begin", "tdsa_demod_timer_end")

    def __init__(self, mode, input_rate: float, decimation: int = 1, channels: int = 1, taps=None,
                 deemphasis: Optional[float] = None, remove_carrier: bool = False, scale: float = 1.0, device: int = 0,
                 max_host_samples: int = 1 << 20):
        self.taps = None if taps is None else as_taps(taps)
        self._mode = check_parameters(mode, channels, decimation,
                                      self.taps.size if self.taps is not None else int(decimation))
        self.mode = "am" if self._mode == nat.DEMOD_AM else "fm"
        self.channels = int(channels)
        self.decimation = int(decimation)
        self.input_rate = float(input_rate)
        if not self.input_rate > 0:
            raise ValueError(f"input_rate={input_rate}")
        if self.taps is None:
            self.taps = design_audio_filter(self.decimation)
        if not np.isfinite(float(scale)):
            raise ValueError(f"scale={scale}")
        self.scale = float(scale)
        self.device = int(device)
        self.max_host_samples = int(max_host_samples)
        if self.max_host_samples < self.channels:
            raise ValueError(f"max_host_samples={max_host_samples}: at least one sample per channel")
        if remove_carrier:
            self.pole_mode = nat.DEMOD_POLE_HIGHPASS
            self.pole = deemphasis_pole(10e-3 if deemphasis is None else deemphasis, self.audio_rate)
        elif deemphasis is not None:
            self.pole_mode = nat.DEMOD_POLE_LOWPASS
            self.pole = deemphasis_pole(deemphasis, self.audio_rate)
        else:
            self.pole_mode, self.pole = nat.DEMOD_POLE_OFF, 0.0
        self._inputs = 0
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_demod_create(self.device, self._mode, self.channels, self.decimation, int(self.taps.size),
                                            self.max_host_samples, C.byref(self._h)))
        nat.check(nat.lib.tdsa_demod_set_taps(self._h, self.taps.ctypes.data_as(C.c_void_p), int(self.taps.size)))
        nat.check(nat.lib.tdsa_demod_set_pole(self._h, self.pole_mode, self.pole, self.scale))

    # ------------------------------------------------------------------ configuration
    @property
    def audio_rate(self) -> float:
        return self.input_rate / self.decimation

    @property
    def first_full_output(self) -> int:
        """The first output whose filter window lies entirely in real discriminator values: ceil((T - 1) / R) for AM,
        ceil(T / R) for FM, whose d[0] has no predecessor."""
        return -(-(int(self.taps.size) - (self.mode == "am")) // self.decimation)

    def set_pole(self, pole_mode: int, c: float, scale: Optional[float] = None) -> None:
        """The one-pole section by its coefficient; also resets the handle."""
        if pole_mode not in (nat.DEMOD_POLE_OFF, nat.DEMOD_POLE_LOWPASS, nat.DEMOD_POLE_HIGHPASS):
            raise ValueError(f"pole_mode={pole_mode}")
        check_parameters(self._mode, self.channels, self.decimation, self.taps.size, c)
        s = self.scale if scale is None else float(scale)
        nat.check(nat.lib.tdsa_demod_set_pole(self._h, int(pole_mode), float(c), s))
        self.pole_mode, self.pole, self.scale, self._inputs = int(pole_mode), float(c), s, 0

    def outputs_completed_by(self, n_in: int) -> int:
        """Outputs per channel a call delivering n_in more inputs per channel would complete."""
        return outputs_completed(self._inputs, n_in, self.decimation)

    def reset(self) -> None:
        """History, pole state and measurements to zero: inputs count from 0 again."""
        nat.check(nat.lib.tdsa_demod_reset(self._h))
        self._inputs = 0

    # ------------------------------------------------------------------ processing
    def process(self, x) -> np.ndarray:
        """Complex [C][n] (or [n] for one channel) in host memory: float32 [C][n_out], the outputs it completes."""
        a = np.asarray(x)
        if not np.iscomplexobj(a):
            raise ValueError(f"real input ({a.dtype}): the demodulator takes complex64 streams")
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.channels:
            raise ValueError(f"input of shape {np.shape(x)}: [{self.channels}][n]")
        a = np.ascontiguousarray(a, dtype=np.complex64)
        n = a.shape[1]
        per_call = self.max_host_samples // self.channels
        outs = []
        for s in range(0, max(n, 1), per_call):
            k = min(per_call, n - s)
            want = self.outputs_completed_by(k)
            out = np.empty((self.channels, max(want, 1)), dtype=np.float32)
            n_out = C.c_size_t()
            nat.check(nat.lib.tdsa_demod_process(self._h, C.c_void_p(a.ctypes.data + 8 * s), k, n,
                                                 out.ctypes.data_as(C.c_void_p), out.shape[1], C.byref(n_out)))
            self._inputs += k
            outs.append(out[:, :n_out.value])
        return outs[0] if len(outs) == 1 else np.concatenate(outs, axis=1)

    def process_device(self, engine: Optional[SpectrumEngine], ptr: int, n_in: int, in_stride: int, out_ptr: int,
                       out_stride: int) -> int:
        """Input and output in device memory, on `engine`'s stream (None: the handle's own), no host wait.  Channel c's
        n_in samples are at ptr + 8 c in_stride, its outputs go to out_ptr + 4 c out_stride.  Returns the number of
        outputs per channel."""
        check_call(n_in, in_stride, ptr or 0, self.outputs_completed_by(n_in), out_stride, out_ptr or 0)
        if engine is not None:
            check_same_device(engine.device, self.device)
        n_out = C.c_size_t()
        nat.check(nat.lib.tdsa_demod_process_dev(self._h, engine._h if engine is not None else None,
                                                 C.c_void_p(ptr) if ptr else None, int(n_in), int(in_stride),
                                                 C.c_void_p(out_ptr) if out_ptr else None, int(out_stride),
                                                 C.byref(n_out)))
        self._inputs += int(n_in)
        return int(n_out.value)

    # ------------------------------------------------------------------ measurements
    def measure(self) -> Measurement:
        """Waits for the handle's work, then reads the five per-channel accumulators."""
        cnt = np.empty(self.channels, dtype=np.int64)
        mx = np.empty(self.channels, dtype=np.float32)
        mn = np.empty(self.channels, dtype=np.float32)
        s = np.empty(self.channels, dtype=np.float64)
        ss = np.empty(self.channels, dtype=np.float64)
        nat.check(nat.lib.tdsa_demod_read_meas(self._h, *(v.ctypes.data_as(C.c_void_p) for v in (cnt, mx, mn, s, ss))))
        return derive(self.mode, self.input_rate, cnt, mx, mn, s, ss)

    def reset_measure(self) -> None:
        """The accumulators start again; the audio state is not touched."""
        nat.check(nat.lib.tdsa_demod_reset_meas(self._h))
