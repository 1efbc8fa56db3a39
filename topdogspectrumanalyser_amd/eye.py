"""Eye diagrams on the device: I / Q and FSK eyes on the recovered symbol clock.

What a vector analyser shows beside the constellation: segments of a stream in HBM folded on one symbol clock per
segment - the one symbols.SymbolSync or fsk.FskAnalyzer has just put into its records, or the caller's - into a density
image of `points` columns over one symbol by `rows` rows over a value range, kept as integers on the device across
calls (the persistence display) until reset().  The centre column is the producer's symbols, bit for bit; the columns
around it are the same cubic resampler at the positions between them - one HIP pass, tdsa_eye_*.  The opening figures
come from the integer image on the host.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from . import fsk as _fsk
from . import symbols as _sym
from .engine import SpectrumEngine
from .symbols import MAX_SPS, MAX_SYMBOLS, MIN_SPS, ONE, fixed_step
from .zoom import check_same_device

KINDS = {"iq": nat.EYE_IQ, "fm": nat.EYE_FM, "real": nat.EYE_REAL}
POINTS = (4, 8, 16, 32, 64)
MIN_ROWS, MAX_ROWS = 8, 256
MAX_BINS = nat.EYE_MAX_BINS
MAX_BOXCAR = _fsk.MAX_BOXCAR
MIN_SYMBOLS = 3
CLOCK = np.dtype([("delta_fx", np.uint64), ("step_f", np.uint32), ("theta_fx", np.uint32)])
assert CLOCK.itemsize == 16
SENTINEL = np.float32(-77.0)           # what process(traces=True) leaves where the library writes nothing


def eye_count(kind: int) -> int:
    return 2 if kind == nat.EYE_IQ else 1


def symbols_per_segment(step: int, seg_len: int, kind: int, boxcar: int) -> int:
    """K, the producer's own: symbols.symbols_per_segment (iq), fsk.symbols_per_segment with iq (fm) or freq (real)."""
    if kind == nat.EYE_IQ:
        return _sym.symbols_per_segment(step, seg_len)
    return _fsk.symbols_per_segment(step, seg_len, nat.FSK_IQ if kind == nat.EYE_FM else nat.FSK_FREQ, boxcar)


def checked_symbols(step: int, seg_len: int, kind: int, boxcar: int) -> int:
    """K of a segment of seg_len samples; ValueError outside 3 .. 4096."""
    K = symbols_per_segment(step, seg_len, kind, boxcar)
    if not MIN_SYMBOLS <= K <= MAX_SYMBOLS:
        raise ValueError(f"seg_len={seg_len} gives {K} symbols per segment: {MIN_SYMBOLS} .. {MAX_SYMBOLS}")
    return K


def check_parameters(samples_per_symbol: float, input: str, points: int, rows: int, v_range, boxcar: Optional[int]):
    """The constructor's arguments, checked before any device is touched: (step, kind, boxcar, points, rows, lo, hi)."""
    sps = float(samples_per_symbol)
    if not MIN_SPS <= sps <= MAX_SPS:
        raise ValueError(f"samples_per_symbol={samples_per_symbol}: {MIN_SPS:g} .. {MAX_SPS:g}")
    if input not in KINDS:
        raise ValueError(f"input={input!r}: 'iq', 'fm' or 'real'")
    if isinstance(points, bool) or int(points) != points or int(points) not in POINTS:
        raise ValueError(f"points={points}: 4, 8, 16, 32 or 64 per symbol")
    if isinstance(rows, bool) or int(rows) != rows or not MIN_ROWS <= int(rows) <= MAX_ROWS:
        raise ValueError(f"rows={rows}: {MIN_ROWS} .. {MAX_ROWS}")
    if int(points) * int(rows) > MAX_BINS:
        raise ValueError(f"points={points} x rows={rows} = {int(points) * int(rows)} bins: at most {MAX_BINS}")
    lo, hi = check_range(v_range)
    b = max(1, int(math.floor(sps / 2))) if boxcar is None else int(boxcar)
    if not 1 <= b <= MAX_BOXCAR:
        raise ValueError(f"boxcar={boxcar}: 1 .. {MAX_BOXCAR}")
    return fixed_step(sps), KINDS[input], b, int(points), int(rows), lo, hi


def check_range(v_range) -> Tuple[np.float32, np.float32]:
    try:
        with np.errstate(over="ignore"):
            lo, hi = (np.float32(v) for v in v_range)
    except (TypeError, ValueError):
        raise ValueError(f"v_range={v_range!r}: (lo, hi)") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"v_range={tuple(v_range)}: finite float32")
    if not lo < hi:
        raise ValueError(f"v_range={tuple(v_range)}: lo < hi")
    return lo, hi


def clock_array(step: int, result=None, delta: Optional[float] = None, n_seg: int = 1) -> np.ndarray:
    """The clocks of a call, [n_seg] of CLOCK: from the records of a SymbolResult or an FskResult (a record array does
    too), a segment flagged NONFINITE becoming a skip (delta_fx = 0) - or one fixed clock, `delta` samples
    (1 <= delta < samples per symbol + 1) for each of n_seg segments.  ValueError for a clock outside its range."""
    if (result is None) == (delta is None):
        raise ValueError("either a result or delta=")
    if result is None:
        d = int(round(float(delta) * ONE))
        if not ONE <= d < int(step) + ONE:
            raise ValueError(f"delta={delta}: 1 <= delta < samples_per_symbol + 1")
        if int(n_seg) < 1:
            raise ValueError(f"n_seg={n_seg}: at least one segment")
        ck = np.zeros(int(n_seg), dtype=CLOCK)
        ck["delta_fx"] = d
        return ck
    rec = getattr(result, "records", result)
    rec = np.asarray(rec)
    if rec.dtype.names is None or "delta_fx" not in rec.dtype.names:
        raise ValueError("a SymbolResult, an FskResult or their record array")
    ck = np.zeros(rec.size, dtype=CLOCK)
    ck["delta_fx"] = rec["delta_fx"]
    if "step_f" in rec.dtype.names:
        ck["step_f"], ck["theta_fx"] = rec["step_f"], rec["theta_fx"]
    ck["delta_fx"][(rec["flags"] & np.uint32(nat.FSK_NONFINITE)) != 0] = 0     # the same bit in both record kinds
    return check_clocks(step, ck)


def check_clocks(step: int, clocks) -> np.ndarray:
    ck = np.ascontiguousarray(clocks, dtype=CLOCK).reshape(-1)
    d = ck["delta_fx"]
    bad = np.flatnonzero((d != 0) & ((d < np.uint64(ONE)) | (d >= np.uint64(int(step) + ONE))))
    if bad.size:
        raise ValueError(f"clock of segment {int(bad[0])}: delta_fx={int(d[bad[0]])}: 0 (skip) or 2^32 <= delta_fx < step + 2^32")
    return ck


@dataclass
class EyeImage:
    """What read() returns: counts [eyes][rows][points] uint64 (row 0 the lowest value; eyes: I and Q for iq, else one),
    per eye n_points, n_under, n_over, n_nan, the segments seen and skipped, and the value range.  The helpers work in
    float64 from these integers alone."""
    counts: np.ndarray
    n_points: np.ndarray
    n_under: np.ndarray
    n_over: np.ndarray
    n_nan: np.ndarray
    segments: int
    skipped: int
    lo: float
    hi: float

    @property
    def rows(self) -> int:
        return int(self.counts.shape[1])

    @property
    def points(self) -> int:
        return int(self.counts.shape[2])

    def two_symbols(self) -> np.ndarray:
        """[eyes][rows][2 points]: the image tiled to the customary two-symbol display."""
        return np.concatenate([self.counts, self.counts], axis=2)

    def density(self) -> np.ndarray:
        """[eyes][rows][points] float64: counts over the eye's n_points (zeros where there are none)."""
        n = self.n_points.astype(np.float64)[:, None, None]
        return np.where(n > 0, self.counts.astype(np.float64) / np.where(n > 0, n, 1.0), 0.0)

    def row_of(self, value: float) -> int:
        """The row a value lies in, clipped to 0 .. rows - 1."""
        t = (float(value) - float(self.lo)) * (self.rows / (float(self.hi) - float(self.lo)))
        return int(min(max(math.floor(t), 0), self.rows - 1)) if math.isfinite(t) else (0 if t < 0 else self.rows - 1)

    def opening(self, threshold: float, eye: int = 0) -> Tuple[float, float]:
        """(height, width) of the eye around `threshold`.  Height: the rows strictly between the nearest occupied rows
        above and below row_of(threshold) in column points / 2 (the image's edge where there is none), times
        (hi - lo) / rows; 0 if that row is occupied itself.  Width: 1 + the consecutive columns left of points / 2 + those
        right of it whose bin in that row is empty, over points (a fraction of a symbol, no wrap); 0 if the centre is
        occupied."""
        img = self.counts[int(eye)]
        H, P = img.shape
        r, mid = self.row_of(threshold), P // 2
        if img[r, mid] != 0:
            return 0.0, 0.0
        col = img[:, mid] != 0
        above = np.flatnonzero(col[r + 1:])
        below = np.flatnonzero(col[:r])
        top = r + 1 + int(above[0]) if above.size else H
        bottom = int(below[-1]) if below.size else -1
        height = (top - bottom - 1) * (float(self.hi) - float(self.lo)) / H
        row = img[r] == 0
        left = 0
        while mid - 1 - left >= 0 and row[mid - 1 - left]:
            left += 1
        right = 0
        while mid + 1 + right < P and row[mid + 1 + right]:
            right += 1
        return height, (1 + left + right) / P

    @staticmethod
    def thresholds_from(levels) -> np.ndarray:
        """The M - 1 decision thresholds offset + dev (2 j - M), j = 1 .. M - 1: from an FskResult (the medians of its
        unflagged segments' offset and half spacing) or from (offset, dev, M)."""
        if hasattr(levels, "records"):
            rec, M = levels.records, int(levels.n_levels)
            ok = rec["flags"] == 0
            if not np.any(ok):
                raise ValueError("no unflagged segment")
            o, g = float(np.median(rec["offset"][ok])), float(np.median(rec["dev"][ok]))
        else:
            o, g, M = levels
            o, g, M = float(o), float(g), int(M)
        return o + g * (2.0 * np.arange(1, M) - M)


def image_from(counts: np.ndarray, totals: Sequence[int], lo: float, hi: float) -> EyeImage:
    eyes = counts.shape[0]
    t = np.asarray(totals, dtype=np.uint64)
    per = t[:8].reshape(2, 4)[:eyes]
    return EyeImage(counts, per[:, 0].copy(), per[:, 1].copy(), per[:, 2].copy(), per[:, 3].copy(), int(t[8]), int(t[9]),
                    float(lo), float(hi))


class EyeDiagram(nat._Handle, nat._Timer):
    """Eye diagrams of segments at `samples_per_symbol` (4 .. 64, any real number).

    input: "iq" (complex64: two eyes, I and Q, derotated by the clock's carrier), "fm" (complex64 through the FSK
    analysis' discriminator and boxcar) or "real" (float32 through the boxcar).  points: 4, 8, 16, 32 or 64 columns per
    symbol; rows: 8 .. 256 over v_range = (lo, hi); points x rows <= 8192.  boxcar: B, 1 .. 64, by default
    max(1, floor(sps / 2)) as FskAnalyzer's.  max_segments: the segments one call brings."""
    _destroy = "tdsa_eye_destroy"
    _timer = ("tdsa_eye_timer_begin", "tdsa_eye_timer_end")

    def __init__(self, samples_per_symbol: float, input: str = "iq", points: int = 32, rows: int = 128,
                 v_range: Tuple[float, float] = (-1.5, 1.5), boxcar: Optional[int] = None, device: int = 0,
                 max_host_samples: int = 1 << 20, max_segments: int = 1 << 16):
        self.step, self.kind, self.boxcar, self.points, self.rows, self.lo, self.hi = check_parameters(
            samples_per_symbol, input, points, rows, v_range, boxcar)
        self.samples_per_symbol, self.input = float(samples_per_symbol), input
        self.device, self.max_host_samples, self.max_segments = int(device), int(max_host_samples), int(max_segments)
        if self.max_host_samples < 16:
            raise ValueError(f"max_host_samples={max_host_samples}: at least 16")
        if self.max_segments < 1:
            raise ValueError(f"max_segments={max_segments}: at least 1")
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_eye_create(self.device, self.max_host_samples, self.max_segments, C.byref(self._h)))
        self._configure()

    def _configure(self) -> None:
        nat.check(nat.lib.tdsa_eye_configure(self._h, self.step, self.kind, self.boxcar, self.points, self.rows,
                                             float(self.lo), float(self.hi)))

    @property
    def eyes(self) -> int:
        return eye_count(self.kind)

    @property
    def _unit(self) -> int:
        return 4 if self.kind == nat.EYE_REAL else 8

    @property
    def _trace_dtype(self):
        return np.complex64 if self.kind == nat.EYE_IQ else np.float32

    def symbols_per_segment(self, seg_len: int) -> int:
        """K of a segment of seg_len samples, the producer's; ValueError outside 3 .. 4096."""
        return checked_symbols(self.step, seg_len, self.kind, self.boxcar)

    def clocks(self, result=None, delta: Optional[float] = None, n_seg: int = 1) -> np.ndarray:
        """The clock array of a call: clocks(result) from the records of a SymbolResult or an FskResult (a segment
        flagged NONFINITE becomes a skip), or clocks(delta=..., n_seg=...) for one fixed clock."""
        return clock_array(self.step, result, delta, n_seg)

    def _checked(self, seg_len: int, hop: int, clocks) -> Tuple[int, np.ndarray]:
        K = self.symbols_per_segment(seg_len)
        if int(hop) < 1:
            raise ValueError(f"hop={hop}: at least one sample")
        ck = check_clocks(self.step, clocks)
        if not 1 <= ck.size <= self.max_segments:
            raise ValueError(f"{ck.size} clocks: 1 .. {self.max_segments} segments (max_segments)")
        return K, ck

    def process(self, x, seg_len: int, clocks, hop: Optional[int] = None, traces: bool = False) -> Optional[np.ndarray]:
        """Samples in host memory: segment s is the seg_len samples at s hop (default seg_len), one clock each.  Adds to
        the image; with traces=True returns them, [n_seg][K - 2][points] (complex64 for iq, else float32), a skipped
        segment's left at SENTINEL."""
        a = np.asarray(x)
        cplx = self.kind != nat.EYE_REAL
        if a.ndim != 1 or np.iscomplexobj(a) != cplx:
            raise ValueError(f"input of dtype {a.dtype} and shape {a.shape}: one {'complex' if cplx else 'real'} stream")
        a = np.ascontiguousarray(a, dtype=np.complex64 if cplx else np.float32)
        seg_len = int(seg_len)
        hop = seg_len if hop is None else int(hop)
        K, ck = self._checked(seg_len, hop, clocks)
        used = (ck.size - 1) * hop + seg_len
        if used > a.size:
            raise ValueError(f"{ck.size} segments of {seg_len} samples every {hop} need {used} samples, the block has {a.size}")
        if used > self.max_host_samples:
            raise ValueError(f"block of {used} samples: the handle stages at most {self.max_host_samples} (max_host_samples)")
        tr = None
        if traces:
            tr = np.full((ck.size, K - 2, self.points), SENTINEL, dtype=self._trace_dtype)
        nat.check(nat.lib.tdsa_eye_process(self._h, a.ctypes.data_as(C.c_void_p), used, seg_len, hop, int(ck.size),
                                           ck.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p) if traces else None))
        return tr

    def process_device(self, engine: Optional[SpectrumEngine], ptr: int, seg_len: int, hop: int, n_seg: int, clocks,
                       traces_ptr: Optional[int] = None) -> None:
        """Input (and traces) in device memory, the clocks in host memory, on `engine`'s stream behind its work (None:
        the handle's own).  Segment s is the seg_len samples at ptr + unit s hop (unit: 8 bytes, 4 for real); its traces
        go to traces_ptr + trace unit s (K - 2) points.  Does not wait: read() does."""
        K, ck = self._checked(seg_len, hop, clocks)
        if ck.size != int(n_seg):
            raise ValueError(f"{ck.size} clocks for n_seg={n_seg}")
        if not ptr:
            raise ValueError("null pointer")
        if int(ptr) % self._unit:
            raise ValueError(f"input pointer must be aligned to one sample ({self._unit} bytes)")
        tunit = 8 if self.kind == nat.EYE_IQ else 4
        if traces_ptr and int(traces_ptr) % tunit:
            raise ValueError(f"traces pointer must be aligned to one point ({tunit} bytes)")
        if engine is not None:
            check_same_device(engine.device, self.device)
        nat.check(nat.lib.tdsa_eye_process_dev(self._h, engine._h if engine is not None else None, C.c_void_p(int(ptr)),
                                               int(seg_len), int(hop), int(n_seg), ck.ctypes.data_as(C.c_void_p),
                                               C.c_void_p(int(traces_ptr)) if traces_ptr else None))

    def read(self) -> EyeImage:
        """Waits for the calls so far and returns the image."""
        counts = np.zeros((self.eyes, self.rows, self.points), dtype=np.uint64)
        totals = np.zeros(nat.EYE_TOTALS, dtype=np.uint64)
        nat.check(nat.lib.tdsa_eye_read(self._h, counts.ctypes.data_as(C.c_void_p), totals.ctypes.data_as(C.c_void_p)))
        return image_from(counts, totals, self.lo, self.hi)

    def reset(self) -> None:
        """Zeroes the image and the totals."""
        nat.check(nat.lib.tdsa_eye_reset(self._h))

    def set_range(self, lo: float, hi: float) -> None:
        """A new value range; the image starts again."""
        self.lo, self.hi = check_range((lo, hi))
        self._configure()
