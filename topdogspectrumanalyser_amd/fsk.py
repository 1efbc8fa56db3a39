"""FSK analysis on the device: symbol clock, deviation, symbols, FSK error.

The vector analyser's FSK mode for 2-, 4- and 8-level FSK, GFSK, MSK and GMSK: per segment of a complex64 stream in HBM
(zoom.DownConverter, a channel of channelizer.Channelizer) or of a float32 stream that is a frequency already
(demod.Demodulator at decimation 1, whose FIR is then the post-detection filter), the discriminator, a boxcar, the
symbol clock from the spectral line of the squared lag differences, a cubic resampler to one level per symbol, two
rounds of decision and least-squares fit for offset and deviation, and the error of every symbol against its level -
one HIP pass, tdsa_fsk_*.  An analyser's recovery, not a receiver's: feed-forward, every segment on its own.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native as nat
from ._inputs import _Segments
from .engine import SpectrumEngine
from .symbols import MAX_SPS, MAX_SYMBOLS, MIN_SPS, ONE, fixed_step, phase_step  # noqa: F401  (importable from here)
from .zoom import check_same_device

MAX_BOXCAR = MAX_LAG = 64
KINDS = {"iq": nat.FSK_IQ, "freq": nat.FSK_FREQ}

RECORD = np.dtype([("delta_fx", np.uint64), ("c_re", np.float32), ("c_im", np.float32), ("p", np.float32),
                   ("offset", np.float32), ("dev", np.float32), ("lo", np.float32), ("hi", np.float32),
                   ("err_peak", np.float32), ("err_sumsq", np.float64), ("err_peak_k", np.int32), ("sum_l", np.int32),
                   ("flags", np.uint32), ("reserved", np.uint32)])
assert RECORD.itemsize == 64
SENTINEL = np.float32(-77.0)          # what process() leaves where the library writes no level ...
SENTINEL_INDEX = np.uint8(0xEE)       # ... and no index


def level_count(levels: Union[int, str]) -> int:
    """M of `levels`: 2, 4 or 8; "msk" (and "gmsk") is 2."""
    if isinstance(levels, str):
        if levels.lower() in ("msk", "gmsk"):
            return 2
        raise ValueError(f"levels={levels!r}: 2, 4, 8 or 'msk'")
    if isinstance(levels, bool) or int(levels) != levels or int(levels) not in (2, 4, 8):
        raise ValueError(f"levels={levels}: 2, 4, 8 or 'msk'")
    return int(levels)


def symbols_per_segment(step: int, seg_len: int, kind: int, boxcar: int) -> int:
    """K = floor((n_b - 4) 2^32 / step) - 1 with n_b = seg_len - (1 for iq) - boxcar + 1 (negative for a segment too
    short to ask)."""
    nb = int(seg_len) - (1 if kind == nat.FSK_IQ else 0) - int(boxcar) + 1
    return ((nb - 4) * ONE) // int(step) - 1 if nb >= 4 else -1


@dataclass
class FskResult:
    """Per segment: levels [n_seg][K] float32 (the discriminator's output at the symbol centres, half turns per sample
    for iq), indices [n_seg][K] uint8 (0 .. M - 1, level l = 2 i - (M - 1)), delta (the first symbol's position in input
    samples, the boxcar's group delay included), timing_quality (|C| / P), offset (the centre of the levels), deviation
    (the outer one, g (M - 1)), mod_index (adjacent-level spacing times the symbol time, iq only), fsk_error (rms error
    over the outer deviation), peak_error (the largest, likewise), flags (FSK_NONFINITE, FSK_ONE_LEVEL) and the records
    as the library gave them."""
    levels: Optional[np.ndarray]
    indices: Optional[np.ndarray]
    delta: np.ndarray
    timing_quality: np.ndarray
    offset: np.ndarray
    deviation: np.ndarray
    mod_index: np.ndarray
    fsk_error: np.ndarray
    peak_error: np.ndarray
    flags: np.ndarray
    records: np.ndarray
    n_levels: int = 2

    def offset_hz(self, fs: float) -> np.ndarray:
        """The carrier offset at sample rate fs, for levels in half turns per sample."""
        return self.offset * (0.5 * float(fs))

    def deviation_hz(self, fs: float) -> np.ndarray:
        """The outer deviation at sample rate fs, for levels in half turns per sample."""
        return self.deviation * (0.5 * float(fs))

    def bits(self, mapping: str = "gray") -> np.ndarray:
        """[n_seg][K log2 M] uint8, most significant bit first: the index itself ("natural") or Gray coded ("gray":
        adjacent levels differ in one bit)."""
        if mapping not in ("gray", "natural"):
            raise ValueError(f"mapping={mapping!r}: 'gray' or 'natural'")
        if self.indices is None:
            raise ValueError("the indices are in device memory: read them from idx_ptr")
        i = self.indices.astype(np.uint8)
        if mapping == "gray":
            i = i ^ (i >> 1)
        nb = self.n_levels.bit_length() - 1
        sh = np.arange(nb - 1, -1, -1, dtype=np.uint8)
        return ((i[..., None] >> sh) & 1).reshape(i.shape[0], -1).astype(np.uint8)


def result_from(records: np.ndarray, levels, indices, K: int, M: int, sps: float, kind: int, boxcar: int) -> FskResult:
    """The derived figures of a call's records."""
    r = records
    with np.errstate(all="ignore"):
        g = r["dev"].astype(np.float64)
        outer = g * (M - 1)
        ok = outer > 0
        rms = np.sqrt(r["err_sumsq"] / K)
        fe = np.where(ok, rms / np.where(ok, outer, 1.0), 0.0)
        pe = np.where(ok, r["err_peak"].astype(np.float64) / np.where(ok, outer, 1.0), 0.0)
    delay = boxcar / 2.0 if kind == nat.FSK_IQ else (boxcar - 1) / 2.0
    h = g * sps if kind == nat.FSK_IQ else np.full(r.size, np.nan)
    return FskResult(levels, indices, r["delta_fx"].astype(np.float64) / ONE + delay, _Segments.timing_quality(r),
                     r["offset"].astype(np.float64), outer, h, fe, pe, r["flags"].copy(), r, M)


class FskAnalyzer(_Segments, nat._Handle, nat._Timer):
    """FSK analysis of segments at `samples_per_symbol` (4 .. 64, any real number).

    levels: 2, 4, 8 or "msk" (2).  input: "iq" (complex64) or "freq" (float32, a frequency already).  timing: "auto" (the
    spectral line of the squared lag differences, per segment) or the first symbol's position among the boxcar's outputs
    in samples, 1 <= timing < samples_per_symbol + 1.  boxcar, lag: B and L, 1 .. 64, by default max(1, floor(sps / 2))
    each - with B = L = 1 the clock drowns in noise from 8 samples per symbol upward."""
    _destroy = "tdsa_fsk_destroy"
    _timer = ("tdsa_fsk_timer_begin", "tdsa_fsk_timer_end")
    _process = ("tdsa_fsk_process", "tdsa_fsk_process_dev")
    _record = RECORD
    _filled = ((SENTINEL, np.float32), (SENTINEL_INDEX, np.uint8))

    def __init__(self, samples_per_symbol: float, levels: Union[int, str] = 2, input: str = "iq",
                 timing: Union[str, float] = "auto", boxcar: Optional[int] = None, lag: Optional[int] = None, device: int = 0,
                 max_host_samples: int = 1 << 20):
        self._rate(samples_per_symbol)
        self.levels = level_count(levels)
        if input not in KINDS:
            raise ValueError(f"input={input!r}: 'iq' or 'freq'")
        self.input, self.kind = input, KINDS[input]
        half = max(1, int(math.floor(self.samples_per_symbol / 2)))
        self.boxcar = half if boxcar is None else int(boxcar)
        self.lag = half if lag is None else int(lag)
        if not 1 <= self.boxcar <= MAX_BOXCAR:
            raise ValueError(f"boxcar={boxcar}: 1 .. {MAX_BOXCAR}")
        if not 1 <= self.lag <= MAX_LAG:
            raise ValueError(f"lag={lag}: 1 .. {MAX_LAG}")
        self._stage(timing, device, max_host_samples)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_fsk_create(self.device, self.max_host_samples, C.byref(self._h)))
        nat.check(nat.lib.tdsa_fsk_configure(self._h, self.step, self.nu, self.levels, self.kind, self.boxcar, self.lag,
                                             self.timing_mode, self.delta_fx))

    @property
    def _unit(self) -> int:
        return 8 if self.kind == nat.FSK_IQ else 4

    def _k(self, seg_len: int) -> int:
        return symbols_per_segment(self.step, seg_len, self.kind, self.boxcar)

    def _result(self, rec, levels, indices, K) -> FskResult:
        return result_from(rec, levels, indices, K, self.levels, self.samples_per_symbol, self.kind, self.boxcar)

    def process(self, x, seg_len: int, hop: Optional[int] = None, out_stride: Optional[int] = None,
                indices: bool = True) -> FskResult:
        """Samples in host memory: every whole segment of seg_len samples, `hop` (default seg_len) apart."""
        a = np.asarray(x)
        if a.ndim != 1 or np.iscomplexobj(a) != (self.kind == nat.FSK_IQ):
            raise ValueError(f"input of dtype {a.dtype} and shape {a.shape}: one "
                             f"{'complex' if self.kind == nat.FSK_IQ else 'real'} stream")
        a = np.ascontiguousarray(a, dtype=np.complex64 if self.kind == nat.FSK_IQ else np.float32)
        K, rec, lev, idx = self._host(a, seg_len, hop, out_stride, indices)
        return self._result(rec, lev, idx, K)

    def process_device(self, engine: Optional[SpectrumEngine], ptr: int, seg_len: int, hop: int, n_seg: int, out_ptr: int,
                       out_stride: int, idx_ptr: Optional[int] = None) -> FskResult:
        """Input and output in device memory, on `engine`'s stream (None: the handle's own).  Segment s is the seg_len
        samples at ptr + unit s hop (unit: 8 bytes for iq, 4 for freq); its K levels go to out_ptr + 4 s out_stride (and
        their indices to idx_ptr + s out_stride).  Returns when the records have arrived; `levels` and `indices` of the
        result are None: they are at out_ptr and idx_ptr."""
        K = self._check(seg_len, hop, n_seg, out_stride)
        if int(ptr) % self._unit:
            raise ValueError(f"input pointer must be aligned to one sample ({self._unit} bytes)")
        if int(out_ptr) % 4:
            raise ValueError("output pointer must be aligned to one float32 (4 bytes)")
        if not ptr or not out_ptr:
            raise ValueError("null pointer")
        if engine is not None:
            check_same_device(engine.device, self.device)
        rec = np.zeros(int(n_seg), dtype=RECORD)
        nat.check(getattr(nat.lib, self._process[1])(self._h, engine._h if engine is not None else None, C.c_void_p(ptr),
                                                     int(seg_len), int(hop), int(n_seg), C.c_void_p(out_ptr), int(out_stride),
                                                     C.c_void_p(idx_ptr) if idx_ptr else None, rec.ctypes.data_as(C.c_void_p)))
        return self._result(rec, None, None, K)
