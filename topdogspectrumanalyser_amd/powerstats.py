"""Power statistics of IQ streams on the device: CCDF, PAPR / crest factor, APD, gated by a power threshold (DESIGN.md
section 4.17).

The one measurement of a signal analyser that no dB row carries: the statistics of the INSTANTANEOUS power |x|^2 of the
samples.  One HIP pass (tdsa_pstat_*) over raw int8 / uint8 captures, a DownConverter's complex64 stream or all channels
of a Channelizer at once leaves, per stream, integer state in device memory: a histogram of the float32 power with 32
bins per octave over 64 octaves, the exact sum of the power, its peak and minimum, and a count per class of sample (NaN,
gated, infinite, zero, below / above the window).  Integers commute, so the state is the same bits however the samples
were split into calls.  process_device does not wait; read() does, and everything below it is numpy on a few KiB.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._inputs import _IqStreams

MAX_STREAMS = 256
BINS, BINS_PER_OCTAVE, OCTAVES, EXPONENTS = 2048, 32, 64, 256
EXP_LO_MIN, EXP_LO_MAX, EXP_LO_DEFAULT = -126, 64, -40
COUNTS = ("n_total", "n_nan", "n_gated", "n_inf", "n_zero", "n_under", "n_over")
RECORD = np.dtype([(f, np.uint64) for f in COUNTS] + [("max_bits", np.uint32), ("min_bits", np.uint32),
                                                       ("reserved", np.uint32, (2,))])
assert RECORD.itemsize == 72 == C.sizeof(nat.PstatRecord)


def gaussian_ccdf(db):
    """P(p >= mean 10^(db / 10)) of complex Gaussian noise, whose power is exponentially distributed: exp(-10^(db / 10))."""
    return np.exp(-np.power(10.0, np.asarray(db, dtype=np.float64) / 10.0))


def bin_edges(exp_lo: int) -> np.ndarray:
    """The 2049 edges of the histogram, float64: edge_b = 2^(exp_lo + b // 32) (1 + (b % 32) / 32)."""
    b = np.arange(BINS + 1)
    return np.ldexp(1.0 + (b % BINS_PER_OCTAVE) / BINS_PER_OCTAVE, int(exp_lo) + b // BINS_PER_OCTAVE)


def _checked(exp_lo, gate) -> Tuple[int, float]:
    """The parameters as the library takes them; ValueError before it is called."""
    try:
        e = int(exp_lo)
        if e != exp_lo:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"exp_lo={exp_lo!r}: an integer {EXP_LO_MIN} .. {EXP_LO_MAX}") from None
    if not EXP_LO_MIN <= e <= EXP_LO_MAX:
        raise ValueError(f"exp_lo={exp_lo}: {EXP_LO_MIN} .. {EXP_LO_MAX}")
    with np.errstate(over="ignore"):
        g = float(np.float32(gate))
    if not (math.isfinite(g) and g >= 0.0):
        raise ValueError(f"gate={gate}: a finite float32, not negative (0 = off)")
    return e, g


def _db(x):
    with np.errstate(all="ignore"):
        return 10.0 * np.log10(x)


@dataclass
class PowerStatistics:
    """The state of some streams as read() found it.  records: [S] of RECORD; msum: [S][256] uint64; hist: [S][2048]
    uint64; first_stream: the handle's stream that index 0 is.  Powers are linear, in the units of |x|^2 of the unpacked
    samples (int8: (I + jQ) / 128)."""
    records: np.ndarray
    msum: np.ndarray
    hist: np.ndarray
    exp_lo: int
    gate: float
    first_stream: int = 0

    def __len__(self) -> int:
        return int(self.records.shape[0])

    def __getattr__(self, name):
        if (name in COUNTS or name in ("max_bits", "min_bits")) and "records" in self.__dict__:
            return self.records[name]                 # n_total, n_nan, ... max_bits, min_bits: [S] each
        raise AttributeError(name)

    @property
    def counted(self) -> np.ndarray:
        """[S] the samples the statistics are about: all but the gated ones and the NaNs."""
        r = self.records
        return r["n_total"] - r["n_gated"] - r["n_nan"]

    def total_power(self, stream: int = 0) -> Fraction:
        """The exact sum of the power of the stream's finite counted samples.  (Python integers: a numpy int64 shifted
        by the exponent overflows silently.)"""
        m = self.msum[stream]
        t = int(m[0]) + sum(int(m[e]) << (e - 1) for e in range(1, EXPONENTS) if m[e])
        return Fraction(t, 1 << 149)

    @property
    def mean_power(self) -> np.ndarray:
        """[S] float64: the exact total over counted, rounded once; +inf with an infinite sample, NaN with none counted."""
        out = np.empty(len(self), dtype=np.float64)
        for s in range(len(self)):
            n = int(self.counted[s])
            out[s] = math.inf if int(self.records["n_inf"][s]) else float(self.total_power(s) / n) if n else math.nan
        return out

    @property
    def peak_power(self) -> np.ndarray:
        """[S] the largest power: +inf with an infinite sample, else the float32 of max_bits; NaN with none counted."""
        r = self.records
        p = r["max_bits"].copy().view(np.float32).astype(np.float64)
        p[r["n_inf"] > 0] = np.inf
        p[self.counted == 0] = np.nan
        return p

    @property
    def min_power(self) -> np.ndarray:
        """[S] the smallest counted power: 0 with a zero sample, else the float32 of min_bits (+inf where only
        infinite samples were counted); NaN with none counted."""
        r = self.records
        p = r["min_bits"].copy().view(np.float32).astype(np.float64)     # all ones: NaN
        p[r["min_bits"] == 0xFFFFFFFF] = np.inf
        p[r["n_zero"] > 0] = 0.0
        p[self.counted == 0] = np.nan
        return p

    @property
    def papr_db(self) -> np.ndarray:
        """[S] peak-to-average power ratio (crest factor) in dB."""
        return _db(self.peak_power / self.mean_power)

    def edges(self) -> np.ndarray:
        return bin_edges(self.exp_lo)

    def ccdf_at_edges(self, stream: int = 0) -> np.ndarray:
        """[2049] exactly P(p >= edge_k) among the counted samples: (sum of hist[k:] + n_over + n_inf) / counted."""
        r = self.records[stream]
        n = int(self.counted[stream])
        if n == 0:
            return np.full(BINS + 1, np.nan)
        tail = np.concatenate([np.cumsum(self.hist[stream][::-1], dtype=np.uint64)[::-1], np.zeros(1, dtype=np.uint64)])
        tail = tail + np.uint64(int(r["n_over"]) + int(r["n_inf"]))
        return tail.astype(np.float64) / float(n)

    def _axis(self, stream: int, relative: bool) -> np.ndarray:
        e = self.edges()
        return _db(e / self.mean_power[stream]) if relative else _db(e)

    def ccdf_curve(self, stream: int = 0, relative: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """(dB [2049], probability [2049]): the bin edges in dB against the stream's mean power (the CCDF) or absolute
        (relative=False: the APD), and the probability that the power is at or above each."""
        return self._axis(stream, relative), self.ccdf_at_edges(stream)

    def ccdf(self, db, stream: int = 0, relative: bool = True):
        """The probability that the power is at or above `db`: exact at the bin edges, linear in probability over dB
        between them, NaN outside the histogram's window."""
        x, p = self.ccdf_curve(stream, relative)
        return np.interp(np.asarray(db, dtype=np.float64), x, p, left=np.nan, right=np.nan)

    def level_db(self, prob, stream: int = 0, relative: bool = True):
        """The level in dB that the power is at or above with probability `prob` (0.1, 0.01, ...): the inverse of ccdf;
        NaN for a probability the window does not reach."""
        x, p = self.ccdf_curve(stream, relative)
        return np.interp(np.asarray(prob, dtype=np.float64), p[::-1], x[::-1], left=np.nan, right=np.nan)


class PowerStats(_IqStreams, nat._Handle, nat._Timer):
    """Statistics of the instantaneous power of `streams` IQ streams (1 .. 256).

    exp_lo: the histogram covers the powers [2^exp_lo, 2^(exp_lo + 64)), 32 bins per octave; -126 .. 64.  gate: samples
    whose power is below it (a float32 compare) are counted as gated and left out of everything else - the statistics of
    a burst's on-time; 0 = off.  The state accumulates over all calls until reset() or configure()."""
    _destroy = "tdsa_pstat_destroy"
    _timer = ("tdsa_pstat_timer_begin", "tdsa_pstat_timer_end")
    _process = ("tdsa_pstat_process", "tdsa_pstat_process_dev")

    def __init__(self, streams: int = 1, exp_lo: int = EXP_LO_DEFAULT, gate: float = 0.0, device: int = 0,
                 max_host_samples: Optional[int] = None):
        self.streams = int(streams)
        if not 1 <= self.streams <= MAX_STREAMS:
            raise ValueError(f"streams={streams}: 1 .. {MAX_STREAMS}")
        cfg = _checked(exp_lo, gate)
        self._stage(max_host_samples)
        self.device = int(device)
        self.exp_lo, self.gate = EXP_LO_DEFAULT, 0.0
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_pstat_create(self.device, self.streams, self.max_host_samples, C.byref(self._h)))
        self._apply(cfg)

    def _apply(self, cfg) -> None:
        nat.check(nat.lib.tdsa_pstat_configure(self._h, cfg[0], cfg[1]))
        self.exp_lo, self.gate = cfg

    def configure(self, *, exp_lo: Optional[int] = None, gate: Optional[float] = None) -> None:
        """New parameters; what is not named stays.  The state starts again."""
        self._apply(_checked(self.exp_lo if exp_lo is None else exp_lo, self.gate if gate is None else gate))

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_pstat_reset(self._h))

    def read(self, streams=None) -> PowerStatistics:
        """Waits for the calls so far and reads the state of all streams (None), of one (an int) or of a range."""
        if streams is None:
            first, count = 0, self.streams
        elif isinstance(streams, range):
            if streams.step != 1 or len(streams) < 1:
                raise ValueError(f"streams={streams}: a range of step 1 that is not empty")
            first, count = streams.start, len(streams)
        else:
            first, count = int(streams), 1
        if first < 0 or first + count > self.streams:
            raise ValueError(f"streams {first} .. {first + count - 1}: inside the handle's {self.streams}")
        rec = np.zeros(count, dtype=RECORD)
        msum = np.zeros((count, EXPONENTS), dtype=np.uint64)
        hist = np.zeros((count, BINS), dtype=np.uint64)
        nat.check(nat.lib.tdsa_pstat_read(self._h, first, count, rec.ctypes.data_as(C.c_void_p),
                                          msum.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p)))
        return PowerStatistics(rec, msum, hist, self.exp_lo, self.gate, first)
