"""Pulse analysis of IQ streams on the device: one descriptor per pulse.

The time-domain measurement of pulsed signals - radar, TDMA bursts, keyed carriers, hoppers.  Three HIP passes
(tdsa_pulse_*) over raw int8 / uint8 captures, a DownConverter's complex64 stream or all channels of a Channelizer at
once run a two-level (hysteresis) detector on the instantaneous power and leave, per stream, a list of pulse records in
device memory: time of arrival, width, peak, energy, and the sum of x[n] conj(x[n-1]) whose angle is the carrier inside
the pulse.  A pulse that is still on when a call ends stays open in the handle and completes in a later call.
process_device does not wait; read() does, and PRI / PRF, duty cycle and the rest are numpy on a few KiB.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._inputs import _IqStreams

MAX_STREAMS = 256
MAX_RECORDS = 1 << 22
TILE, SAMPLES_PER_THREAD = 4096, 16
FLAG_INF = 1
RECORD = np.dtype([("toa", np.int64), ("width", np.int64), ("peak_index", np.int64), ("peak_bits", np.uint32),
                   ("flags", np.uint32), ("energy", np.float64), ("acc_re", np.float64), ("acc_im", np.float64),
                   ("reserved", np.uint64)])
COUNTS = ("n_total", "n_on", "n_pulses", "n_short", "n_lost", "n_nan")
SUMMARY = np.dtype([(f, np.uint64) for f in COUNTS] + [("open_toa", np.int64), ("open_width", np.int64),
                                                        ("open", np.int32), ("reserved", np.int32)])
assert RECORD.itemsize == 64 == C.sizeof(nat.PulseRecord) and SUMMARY.itemsize == 72 == C.sizeof(nat.PulseSummary)


def levels_from_db(on_db: float, hysteresis_db: float = 0.0) -> Tuple[float, float]:
    """(on_level, off_level) as linear powers, power 1.0 = 0 dB: on at on_db, off hysteresis_db below it; each level
    rounded once to float32."""
    if not hysteresis_db >= 0.0:
        raise ValueError(f"hysteresis_db={hysteresis_db}: not negative")
    with np.errstate(over="ignore"):
        on = float(np.float32(10.0 ** (float(on_db) / 10.0)))
        off = float(np.float32(10.0 ** ((float(on_db) - float(hysteresis_db)) / 10.0)))
    return on, off


def _checked(on_level, off_level, min_width) -> Tuple[float, float, int]:
    """The parameters as the library takes them; ValueError before it is called."""
    with np.errstate(over="ignore"):
        on = float(np.float32(on_level))
        off = on if off_level is None else float(np.float32(off_level))
    if not (math.isfinite(on) and on > 0.0):
        raise ValueError(f"on_level={on_level}: a finite float32 above 0")
    if not 0.0 < off <= on:
        raise ValueError(f"off_level={off_level}: above 0 and at most on_level={on}")
    try:
        w = int(min_width)
        if w != min_width:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"min_width={min_width!r}: an integer 1 .. 2^31 - 1") from None
    if not 1 <= w < 1 << 31:
        raise ValueError(f"min_width={min_width}: 1 .. 2^31 - 1")
    return on, off, w


@dataclass
class PulseTrain:
    """The pulses of one stream as read() found them.  records: [K] of RECORD, the stored pulses in time order; summary:
    one SUMMARY record.  Times are in samples since the last reset; powers are linear, in the units of |x|^2 of the
    unpacked samples (int8: (I + jQ) / 128)."""
    records: np.ndarray
    summary: np.ndarray
    stream: int = 0

    def __len__(self) -> int:
        return int(self.records.shape[0])

    def __getattr__(self, name):
        if name in RECORD.names and "records" in self.__dict__:
            return self.records[name]                  # toa, width, peak_index, peak_bits, flags, energy, acc_re, acc_im
        if name in COUNTS and "summary" in self.__dict__:
            return int(self.summary[name])
        raise AttributeError(name)

    @property
    def peak_power(self) -> np.ndarray:
        return self.records["peak_bits"].copy().view(np.float32).astype(np.float64)

    @property
    def mean_power(self) -> np.ndarray:
        return self.records["energy"] / self.records["width"]

    @property
    def freq(self) -> np.ndarray:
        """The carrier inside each pulse in cycles per sample, (-0.5, 0.5]: the angle of the sum of x[n] conj(x[n-1]);
        NaN for a pulse of one sample."""
        f = np.arctan2(self.records["acc_im"], self.records["acc_re"]) / (2.0 * np.pi)
        return np.where(self.records["width"] > 1, f, np.nan)

    def pri(self) -> np.ndarray:
        """[K - 1] pulse repetition intervals in samples."""
        return np.diff(self.records["toa"])

    def prf(self, fs: float) -> np.ndarray:
        """[K - 1] pulse repetition frequencies in Hz at sample rate fs."""
        return float(fs) / self.pri().astype(np.float64)

    def to_seconds(self, fs: float) -> Tuple[np.ndarray, np.ndarray]:
        """(toa, width) in seconds at sample rate fs."""
        return self.records["toa"] / float(fs), self.records["width"] / float(fs)

    @property
    def duty_cycle(self) -> float:
        """The share of samples in the on state, before the width filter; NaN before the first sample."""
        n = int(self.summary["n_total"])
        return int(self.summary["n_on"]) / n if n else math.nan

    @property
    def open_pulse(self) -> Optional[Tuple[int, int]]:
        """(toa, width so far) of the pulse that is not yet complete, or None."""
        if not int(self.summary["open"]):
            return None
        return int(self.summary["open_toa"]), int(self.summary["open_width"])


class PulseAnalyzer(_IqStreams, nat._Handle, nat._Timer):
    """Pulse descriptors of `streams` IQ streams (1 .. 256), up to `capacity` stored pulses each (streams * capacity
    <= 2^22).

    A sample whose power is at or above on_level switches its stream on, one below off_level (or NaN) switches it off,
    anything between leaves it as it is; a pulse is a maximal run of on samples.  Complete pulses shorter than
    min_width are dropped (n_short); those beyond capacity are counted (n_lost).  The state accumulates over all calls
    until reset() or configure()."""
    _destroy = "tdsa_pulse_destroy"
    _timer = ("tdsa_pulse_timer_begin", "tdsa_pulse_timer_end")
    _process = ("tdsa_pulse_process", "tdsa_pulse_process_dev")

    def __init__(self, streams: int = 1, capacity: int = 4096, device: int = 0, max_host_samples: Optional[int] = None):
        self.streams, self.capacity = int(streams), int(capacity)
        if not 1 <= self.streams <= MAX_STREAMS:
            raise ValueError(f"streams={streams}: 1 .. {MAX_STREAMS}")
        if self.capacity < 1 or self.streams * self.capacity > MAX_RECORDS:
            raise ValueError(f"capacity={capacity}: at least 1, streams * capacity at most {MAX_RECORDS}")
        self._stage(max_host_samples)
        self.device = int(device)
        self.on_level, self.off_level, self.min_width = 1.0, 1.0, 1
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_pulse_create(self.device, self.streams, self.capacity, self.max_host_samples, C.byref(self._h)))

    def configure(self, on_level: float, off_level: Optional[float] = None, min_width: int = 1) -> None:
        """New levels (linear power; off_level defaults to on_level: one threshold) and the shortest pulse kept.  The
        state starts again."""
        cfg = _checked(on_level, off_level, min_width)
        nat.check(nat.lib.tdsa_pulse_configure(self._h, cfg[0], cfg[1], cfg[2]))
        self.on_level, self.off_level, self.min_width = cfg

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_pulse_reset(self._h))

    def read_summaries(self) -> np.ndarray:
        """Waits for the calls so far; [streams] of SUMMARY."""
        out = np.zeros(self.streams, dtype=SUMMARY)
        nat.check(nat.lib.tdsa_pulse_read(self._h, 0, self.streams, out.ctypes.data_as(C.c_void_p)))
        return out

    def read(self, stream: int = 0) -> PulseTrain:
        """Waits for the calls so far and reads one stream's summary and its stored pulses."""
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"stream={stream}: inside the handle's {self.streams}")
        summary = np.zeros(1, dtype=SUMMARY)
        nat.check(nat.lib.tdsa_pulse_read(self._h, s, 1, summary.ctypes.data_as(C.c_void_p)))
        stored = min(int(summary[0]["n_pulses"]), self.capacity)
        rec = np.zeros(stored, dtype=RECORD)
        got = C.c_int(0)
        if stored:
            nat.check(nat.lib.tdsa_pulse_read_pulses(self._h, s, 0, stored, rec.ctypes.data_as(C.c_void_p), C.byref(got)))
        return PulseTrain(rec[:got.value], summary[0], s)

    def _debug_limits(self, max_launch_tiles: int = 16384, passes: int = 7) -> None:
        """For the tests and tools/pulsebench.py: fewer tiles per launch, a mask of the three kernels."""
        nat.check(nat.lib.tdsa_pulse_debug_limits(self._h, int(max_launch_tiles), int(passes)))
