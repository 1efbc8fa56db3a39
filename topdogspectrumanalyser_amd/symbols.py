"""Symbol recovery on the device: timing, carrier, one sample per symbol for EVM.

What stands between a complex64 stream in HBM (zoom.DownConverter with root-raised-cosine taps, or a channel of
channelizer.Channelizer) and analytics.Constellation: per segment, the symbol clock from the spectral line of |x|^2
(Oerder-Meyr), a cubic resampler to one sample per symbol on the symbol instants, the carrier offset and phase from the
M-th power (a periodogram refined by the phase between its halves), and the derotation - one HIP pass, tdsa_symsync_*.
An analyser's recovery, not a receiver's: feed-forward, every segment on its own, no symbol decisions.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native as nat
from ._inputs import MAX_SPS, MAX_SYMBOLS, MIN_SPS, ONE, _Segments, fixed_step, phase_step  # noqa: F401  (fsk.py, tests)
from .analytics import constellation_points
from .engine import SpectrumEngine
from .zoom import check_same_device

ORDERS = {"bpsk": 2, "qpsk": 4, "16qam": 4, "64qam": 4, "8psk": 8}

RECORD = np.dtype([("delta_fx", np.uint64), ("c_re", np.float32), ("c_im", np.float32), ("p", np.float32),
                   ("g", np.int32), ("step_f", np.uint32), ("theta_fx", np.uint32), ("peak", np.float32),
                   ("mean", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])
assert RECORD.itemsize == 48
SENTINEL = np.complex64(complex(-77.0, 77.0))    # what process() leaves where the library writes nothing


def rrc_taps(samples_per_symbol: float, alpha: float = 0.35, span: int = 8) -> np.ndarray:
    """Root-raised-cosine taps reaching `span` symbols to either side of the centre (2 floor(span sps) + 1 of them,
    symmetric), float32, unit energy: the matched filter for DownConverter(taps=...); two of them in cascade are a
    raised cosine, free of intersymbol interference to 1e-3 at the default span."""
    sps, a = float(samples_per_symbol), float(alpha)
    if not sps >= 1.0:
        raise ValueError(f"samples_per_symbol={samples_per_symbol}: at least 1")
    if not 0.0 < a <= 1.0:
        raise ValueError(f"alpha={alpha}: 0 < alpha <= 1")
    if int(span) < 1:
        raise ValueError(f"span={span}: at least one symbol")
    half = int(math.floor(int(span) * sps))
    t = np.arange(-half, half + 1, dtype=np.float64) / sps
    h = np.empty_like(t)
    for i, ti in enumerate(t):
        if abs(ti) < 1e-12:
            h[i] = 1.0 - a + 4.0 * a / math.pi
        elif abs(abs(4.0 * a * ti) - 1.0) < 1e-9:
            h[i] = a / math.sqrt(2.0) * ((1 + 2 / math.pi) * math.sin(math.pi / (4 * a))
                                         + (1 - 2 / math.pi) * math.cos(math.pi / (4 * a)))
        else:
            h[i] = (math.sin(math.pi * ti * (1 - a)) + 4 * a * ti * math.cos(math.pi * ti * (1 + a))) / (
                math.pi * ti * (1 - (4 * a * ti) ** 2))
    h /= math.sqrt(float(np.sum(h * h)))
    return h.astype(np.float32)


def carrier_order(modulation: str) -> int:
    """The power that strips the modulation: bpsk 2, qpsk / 16qam / 64qam 4, 8psk 8."""
    try:
        return ORDERS[str(modulation).lower()]
    except KeyError:
        raise ValueError(f"modulation={modulation!r}: one of {sorted(ORDERS)}") from None


def reference_phase(points, M: int) -> float:
    """arg of the sum of p^M over the reference points (float64): where the M-th power of an aligned constellation
    points.  pi for qpsk, 16qam and 64qam, 0 for bpsk and 8psk."""
    p = np.asarray(points)
    if not np.iscomplexobj(p):
        p = p.reshape(-1, 2).astype(np.float64)
        p = p[:, 0] + 1j * p[:, 1]
    p = p.astype(np.complex128).reshape(-1)
    return float(np.angle(np.sum(p ** int(M))))


def symbols_per_segment(step: int, seg_len: int) -> int:
    """K = floor((seg_len - 4) 2^32 / step) - 1 (negative for a segment too short to ask)."""
    return ((int(seg_len) - 4) * ONE) // int(step) - 1 if int(seg_len) >= 4 else -1


@dataclass
class SymbolResult:
    """Per segment: symbols [n_seg][K] complex64, delta (the first symbol's position in samples), timing_quality
    (|C| / P, the depth of the symbol-rate line), freq (carrier in cycles per symbol), phase (radians), lock (peak over
    mean of the carrier transform's power) and flags (SYMSYNC_NONFINITE, SYMSYNC_NO_CARRIER); records and raw (the
    symbols before derotation, when asked for) as the library gave them."""
    symbols: np.ndarray
    delta: np.ndarray
    timing_quality: np.ndarray
    freq: np.ndarray
    phase: np.ndarray
    lock: np.ndarray
    flags: np.ndarray
    records: np.ndarray
    raw: Optional[np.ndarray] = None

    def freq_hz(self, symbol_rate: float) -> np.ndarray:
        return self.freq * float(symbol_rate)


def result_from(records: np.ndarray, symbols: np.ndarray, raw: Optional[np.ndarray] = None) -> SymbolResult:
    """The derived figures of a call's records."""
    r = records
    with np.errstate(all="ignore"):
        lock = np.where(r["mean"] > 0, r["peak"].astype(np.float64) / np.where(r["mean"] > 0, r["mean"], 1.0), 0.0)
    return SymbolResult(symbols, r["delta_fx"].astype(np.float64) / ONE, _Segments.timing_quality(r),
                        r["step_f"].astype(np.int32) / float(ONE), r["theta_fx"].astype(np.int32) * (2.0 * math.pi / ONE), lock, r["flags"].copy(), r, raw)


class SymbolSync(_Segments, nat._Handle, nat._Timer):
    """Symbol recovery of complex64 segments at `samples_per_symbol` (4 .. 64, any real number).

    modulation: names the carrier order and the reference phase (or pass order= and ref_arg= yourself).  timing: "auto"
    (Oerder-Meyr per segment) or the first symbol's position in samples, 1 <= timing < samples_per_symbol + 1.
    carrier=False leaves stage 3 and 4 out: the symbols are the resampler's."""
    _destroy = "tdsa_symsync_destroy"
    _timer = ("tdsa_symsync_timer_begin", "tdsa_symsync_timer_end")
    _process = ("tdsa_symsync_process", "tdsa_symsync_process_dev")
    _record = RECORD
    _filled = ((SENTINEL, np.complex64), (SENTINEL, np.complex64))

    def __init__(self, samples_per_symbol: float, modulation: str = "qpsk", timing: Union[str, float] = "auto",
                 carrier: bool = True, device: int = 0, max_host_samples: int = 1 << 20, order: Optional[int] = None,
                 ref_arg: Optional[float] = None):
        self._rate(samples_per_symbol)
        self.modulation = str(modulation).lower()
        if not carrier:
            self.order, self.ref_arg = 0, 0.0
        else:
            self.order = carrier_order(self.modulation) if order is None else int(order)
            if self.order not in (2, 4, 8):
                raise ValueError(f"order={order}: 2, 4 or 8")
            if ref_arg is None:
                carrier_order(self.modulation)
                ref_arg = reference_phase(constellation_points(self.modulation), self.order)
            self.ref_arg = float(ref_arg)
            if not math.isfinite(self.ref_arg):
                raise ValueError(f"ref_arg={ref_arg}")
        self._stage(timing, device, max_host_samples)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_symsync_create(self.device, self.max_host_samples, C.byref(self._h)))
        nat.check(nat.lib.tdsa_symsync_configure(self._h, self.step, self.nu, self.order, self.ref_arg, self.timing_mode,
                                                 self.delta_fx))

    def _k(self, seg_len: int) -> int:
        return symbols_per_segment(self.step, seg_len)

    def process(self, x, seg_len: int, hop: Optional[int] = None, raw: bool = False,
                out_stride: Optional[int] = None) -> SymbolResult:
        """Complex samples in host memory: every whole segment of seg_len samples, `hop` (default seg_len) apart."""
        a = np.asarray(x)
        if not np.iscomplexobj(a) or a.ndim != 1:
            raise ValueError(f"input of dtype {a.dtype} and shape {a.shape}: one complex stream")
        a = np.ascontiguousarray(a, dtype=np.complex64)
        _, rec, sym, rw = self._host(a, seg_len, hop, out_stride, raw)
        return result_from(rec, sym, rw)

    def process_device(self, engine: Optional[SpectrumEngine], ptr: int, seg_len: int, hop: int, n_seg: int, out_ptr: int,
                       out_stride: int, raw_ptr: Optional[int] = None) -> SymbolResult:
        """Input and output in device memory, on `engine`'s stream (None: the handle's own).  Segment s is the seg_len
        complex64 samples at ptr + 8 s hop; its K symbols go to out_ptr + 8 s out_stride (and, before derotation, to
        raw_ptr).  Returns when the records have arrived; `symbols` of the result is None: they are at out_ptr."""
        self._check(seg_len, hop, n_seg, out_stride)
        for name, p in (("input", ptr), ("output", out_ptr), ("raw output", raw_ptr or 0)):
            if int(p) % 8:
                raise ValueError(f"{name} pointer must be aligned to one complex64 sample (8 bytes)")
        if not ptr or not out_ptr:
            raise ValueError("null pointer")
        if engine is not None:
            check_same_device(engine.device, self.device)
        rec = np.zeros(int(n_seg), dtype=RECORD)
        nat.check(getattr(nat.lib, self._process[1])(self._h, engine._h if engine is not None else None, C.c_void_p(ptr),
                                                     int(seg_len), int(hop), int(n_seg), C.c_void_p(out_ptr),
                                                     int(out_stride), C.c_void_p(raw_ptr) if raw_ptr else None,
                                                     rec.ctypes.data_as(C.c_void_p)))
        return result_from(rec, None)

