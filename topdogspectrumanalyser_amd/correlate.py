"""Correlation search of IQ streams on the device: where a known sequence starts.

A sliding, normalised cross-correlation of every stream against one reference - a preamble, a sync word, a Zadoff-Chu or
Barker code, a radar's transmit pulse - and a peak search over it (tdsa_corr_*).  Raw int8 / uint8 captures, a
DownConverter's complex64 stream or all channels of a Channelizer at once go in; per stream a list of match records
stays in device memory: the window's index, its metric |c|^2 / (E_r e) in 0 .. 1, its energy, and the correlation of the
reference's two halves, whose phase difference is the carrier offset.  The last min_distance windows of a call stay
undecided in the handle until a later call (or flush()) brings their neighbours.  process_device does not wait; read()
does.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as nat
from ._inputs import _IqStreams

MAX_STREAMS = 256
MAX_RECORDS = 1 << 22
MIN_REF, MAX_REF = 2, 1024
MAX_DISTANCE = 65536
TILE, WINDOWS_PER_THREAD = 2048, 8
MAX_LAUNCH_TILES = 1024
TRACE_BYTES, RING_ENTRY_BYTES = 1 << 28, 24
RECORD = np.dtype([("index", np.int64), ("metric", np.float32), ("energy", np.float32), ("c1_re", np.float32),
                   ("c1_im", np.float32), ("c2_re", np.float32), ("c2_im", np.float32)])
COUNTS = ("n_total", "n_windows", "n_decided", "n_matches", "n_lost", "n_bad")
SUMMARY = np.dtype([(f, np.uint64) for f in COUNTS] + [("flushed", np.int32), ("reserved", np.int32)])
assert RECORD.itemsize == 32 == C.sizeof(nat.CorrRecord) and SUMMARY.itemsize == 56 == C.sizeof(nat.CorrSummary)


# ---- reference makers: complex64 of unit mean power --------------------------------------------------------------
def _unit_power(r) -> np.ndarray:
    r = np.asarray(r, dtype=np.complex128)
    return (r / math.sqrt(float(np.mean(np.abs(r) ** 2)))).astype(np.complex64)


def zadoff_chu(L: int, root: int = 1) -> np.ndarray:
    """The Zadoff-Chu sequence of length L and root `root` (coprime to L): constant amplitude, and for such a root a
    periodic autocorrelation that is zero off the peak."""
    L, root = int(L), int(root)
    if L < 2 or not 0 < root < L or math.gcd(root, L) != 1:
        raise ValueError(f"zadoff_chu(L={L}, root={root}): L at least 2, 0 < root < L, coprime")
    n = np.arange(L, dtype=np.int64)
    q = (root * n * (n + L % 2)) % (2 * L)                 # the phase in units of pi / L, reduced exactly
    return _unit_power(np.exp(-1j * np.pi * q / L))


_BARKER = {2: "+-", 3: "++-", 4: "++-+", 5: "+++-+", 7: "+++--+-", 11: "+++---+--+-", 13: "+++++--++-+-+"}


def barker(n: int) -> np.ndarray:
    """The Barker code of length n (2, 3, 4, 5, 7, 11 or 13) as +1 / -1."""
    if n not in _BARKER:
        raise ValueError(f"barker({n}): lengths {sorted(_BARKER)}")
    return np.array([1.0 if ch == "+" else -1.0 for ch in _BARKER[n]], dtype=np.complex64)


def from_symbols(symbols, sps: int, taps=None) -> np.ndarray:
    """The symbols at `sps` samples each: held for a symbol without taps; with taps (symbols.rrc_taps) one impulse per
    symbol shaped by them, the full convolution."""
    s = np.asarray(symbols, dtype=np.complex128).ravel()
    sps = int(sps)
    if s.size < 1 or sps < 1:
        raise ValueError(f"from_symbols: {s.size} symbols at sps={sps}")
    if taps is None:
        return _unit_power(np.repeat(s, sps))
    up = np.zeros(s.size * sps, dtype=np.complex128)
    up[::sps] = s
    return _unit_power(np.convolve(up, np.asarray(taps, dtype=np.float64)))


def _reference(ref) -> np.ndarray:
    """The reference as the library takes it; ValueError before it is called."""
    r = np.asarray(ref)
    if r.ndim != 1 or not MIN_REF <= r.size <= MAX_REF or r.dtype.kind not in "cfiu":
        raise ValueError(f"reference of shape {r.shape} and dtype {r.dtype}: {MIN_REF} .. {MAX_REF} complex samples")
    with np.errstate(over="ignore"):
        r = np.ascontiguousarray(r, dtype=np.complex64)
    if not (np.isfinite(r.real).all() and np.isfinite(r.imag).all()):
        raise ValueError("reference: every sample finite")
    with np.errstate(over="ignore"):
        e = reference_energy(r)
    if not (np.isfinite(e) and e > 0):
        raise ValueError(f"reference energy {e}: finite and above 0")
    return r


def reference_energy(ref) -> np.float32:
    """E_r: the float64 sum of |r[k]|^2 over the complex64 reference, rounded once to float32."""
    r = np.asarray(ref, dtype=np.complex64)
    return np.float32(np.sum(r.real.astype(np.float64) ** 2 + r.imag.astype(np.float64) ** 2))


def _checked(threshold, min_distance, L):
    with np.errstate(over="ignore", invalid="ignore"):
        thr = float(np.float32(threshold))
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"threshold={threshold}: above 0 and at most 1")
    if min_distance is None:
        min_distance = L
    try:
        w = int(min_distance)
        if w != min_distance:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"min_distance={min_distance!r}: an integer 1 .. {MAX_DISTANCE}") from None
    if not 1 <= w <= MAX_DISTANCE:
        raise ValueError(f"min_distance={min_distance}: 1 .. {MAX_DISTANCE}")
    return thr, w


@dataclass
class Matches:
    """The matches of one stream as read() found them.  records: [K] of RECORD, the stored matches in time order;
    summary: one SUMMARY record; L, e_ref: the reference's length and energy.  index is the first sample of the
    reference in the stream, counted from the last reset."""
    records: np.ndarray
    summary: np.ndarray
    L: int
    e_ref: float
    stream: int = 0

    def __len__(self) -> int:
        return int(self.records.shape[0])

    def __getattr__(self, name):
        if name in RECORD.names and "records" in self.__dict__:
            return self.records[name]                  # index, metric, energy, c1_re, c1_im, c2_re, c2_im
        if name in COUNTS and "summary" in self.__dict__:
            return int(self.summary[name])
        raise AttributeError(name)

    @property
    def c1(self) -> np.ndarray:
        return self.records["c1_re"].astype(np.float64) + 1j * self.records["c1_im"].astype(np.float64)

    @property
    def c2(self) -> np.ndarray:
        return self.records["c2_re"].astype(np.float64) + 1j * self.records["c2_im"].astype(np.float64)

    @property
    def c(self) -> np.ndarray:
        """c1 + c2 in complex128."""
        return self.c1 + self.c2

    @property
    def gain(self) -> np.ndarray:
        """c / E_r: the complex amplitude of the reference in the stream."""
        return self.c / float(self.e_ref)

    @property
    def phase(self) -> np.ndarray:
        return np.angle(self.c)

    @property
    def freq(self) -> np.ndarray:
        """The carrier offset in cycles per sample: the halves' centres lie L / 2 apart, so angle(c2 conj(c1)) / (pi L),
        unambiguous within +-1 / L.  Exact for a reference of level envelope; one whose energy sits towards the middle
        reads low by the ratio of its halves' centroid distance to L / 2."""
        return np.angle(self.c2 * np.conj(self.c1)) / (np.pi * self.L)

    @property
    def snr_db(self) -> np.ndarray:
        """10 log10(m / (1 - m)): the reference's power over everything else in the window."""
        m = self.records["metric"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 10.0 * np.log10(m / (1.0 - m))

    def to_seconds(self, fs: float) -> np.ndarray:
        """The matches' starts in seconds at sample rate fs."""
        return self.records["index"] / float(fs)

    @property
    def flushed(self) -> bool:
        return bool(self.summary["flushed"])


class Correlator(_IqStreams, nat._Handle, nat._Timer):
    """Correlation search of `streams` IQ streams (1 .. 256) for `reference` (2 .. 1024 complex samples), up to
    `capacity` stored matches each (streams * capacity <= 2^22); trace = K keeps the metric and the correlation of the
    last K windows of every stream for read_trace().

    Window n is a match when its metric is at or above the threshold, above every metric of the min_distance windows
    before it and at or above every one of the min_distance windows after it.  The state accumulates over all calls
    until reset(), configure() or set_reference(); after flush() a stream takes no samples until one of them."""
    _destroy = "tdsa_corr_destroy"
    _timer = ("tdsa_corr_timer_begin", "tdsa_corr_timer_end")
    _process = ("tdsa_corr_process", "tdsa_corr_process_dev")

    def __init__(self, reference, streams: int = 1, capacity: int = 4096, trace: int = 0, device: int = 0,
                 max_host_samples: Optional[int] = None):
        self.streams, self.capacity = int(streams), int(capacity)
        if not 1 <= self.streams <= MAX_STREAMS:
            raise ValueError(f"streams={streams}: 1 .. {MAX_STREAMS}")
        if self.capacity < 1 or self.streams * self.capacity > MAX_RECORDS:
            raise ValueError(f"capacity={capacity}: at least 1, streams * capacity at most {MAX_RECORDS}")
        if int(trace) < 0 or int(trace) != trace:
            raise ValueError(f"trace={trace}: an integer, not negative")
        self.trace = min(int(trace), TRACE_BYTES // (RING_ENTRY_BYTES * self.streams))
        ref = _reference(reference)
        self._stage(max_host_samples)
        self.device = int(device)
        self.reference, self.threshold, self.min_distance = ref, 1.0, int(ref.size)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_corr_create(self.device, self.streams, self.capacity, self.trace, self.max_host_samples,
                                           ref.ctypes.data_as(C.c_void_p), int(ref.size), C.byref(self._h)))

    @property
    def L(self) -> int:
        return int(self.reference.size)

    def configure(self, threshold: float, min_distance: Optional[int] = None) -> None:
        """A new threshold (0 < threshold <= 1) and min_distance (default: the reference's length).  The streams start
        again."""
        thr, w = _checked(threshold, min_distance, self.L)
        nat.check(nat.lib.tdsa_corr_configure(self._h, thr, w))
        self.threshold, self.min_distance = thr, w

    def set_reference(self, reference) -> None:
        """A new reference; threshold and min_distance stay.  The streams start again."""
        ref = _reference(reference)
        nat.check(nat.lib.tdsa_corr_set_reference(self._h, ref.ctypes.data_as(C.c_void_p), int(ref.size)))
        self.reference = ref

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_corr_reset(self._h))

    def flush(self) -> None:
        """Decides the windows still undecided, as if nothing followed them.  The streams end: reset() starts new ones."""
        nat.check(nat.lib.tdsa_corr_flush(self._h))

    def read_summaries(self) -> np.ndarray:
        """Waits for the calls so far; [streams] of SUMMARY."""
        out = np.zeros(self.streams, dtype=SUMMARY)
        nat.check(nat.lib.tdsa_corr_read(self._h, 0, self.streams, None, out.ctypes.data_as(C.c_void_p)))
        return out

    def read(self, stream: int = 0) -> Matches:
        """Waits for the calls so far and reads one stream's summary and its stored matches."""
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"stream={stream}: inside the handle's {self.streams}")
        summary = np.zeros(1, dtype=SUMMARY)
        rec = np.zeros(self.capacity, dtype=RECORD)
        nat.check(nat.lib.tdsa_corr_read(self._h, s, 1, rec.ctypes.data_as(C.c_void_p), summary.ctypes.data_as(C.c_void_p)))
        stored = min(int(summary[0]["n_matches"]), self.capacity)
        return Matches(rec[:stored].copy(), summary[0], self.L, float(reference_energy(self.reference)), s)

    def read_trace(self, stream: int, first: int, count: int):
        """(m [count] float32, c [count] complex64) of the windows first .. first + count - 1 of one stream; the handle
        keeps the last `trace` complete windows, anything else is an error of the library."""
        s, first, count = int(stream), int(first), int(count)
        if not 0 <= s < self.streams:
            raise ValueError(f"stream={stream}: inside the handle's {self.streams}")
        if first < 0 or count < 0:
            raise ValueError(f"first={first}, count={count}: not negative")
        m = np.zeros(count, dtype=np.float32)
        c = np.zeros(count, dtype=np.complex64)
        nat.check(nat.lib.tdsa_corr_read_trace(self._h, s, first, count, m.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)))
        return m, c

    def _debug_limits(self, max_launch_tiles: int = MAX_LAUNCH_TILES, passes: int = 15, variant: int = 0) -> None:
        """For the tests and tools/corrbench.py: fewer tiles per launch, a mask of the passes, a variant of the correlate
        pass."""
        nat.check(nat.lib.tdsa_corr_debug_limits(self._h, int(max_launch_tiles), int(passes), int(variant)))
