"""Modulation quality on the device: symbol decisions, gain / phase / IQ-offset fit, error vector.

The vector analyser's error summary for linear modulations - BPSK, QPSK, 8PSK, 16QAM, 64QAM or any table of up to 64
points: rows of complex64 symbols in HBM as symbols.SymbolSync leaves them, per row two rounds of nearest-point decision
and least-squares fit of y = a r + c, then the error of every symbol against its point - one HIP pass, tdsa_modq_*.
What comes back per row is one record of float64 sums; EVM, MER, magnitude and phase error, rho, the IQ offset and the
bits are formed from it on the host.  An analyser's stage, not a receiver's: no tracking, no equaliser, every row on
its own.  Short 16 / 64QAM rows (a few hundred symbols) whose carrier SymbolSync's M-th-power stage did not lock show as
a large `changed` and `evm_rms`.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as nat
from .analytics import constellation_points
from .engine import SpectrumEngine
from .zoom import check_same_device

MODULATIONS = ("bpsk", "qpsk", "8psk", "16qam", "64qam")
MAX_POINTS, MAX_SYMBOLS, MIN_SYMBOLS = nat.MODQ_MAX_POINTS, nat.MODQ_MAX_SYMBOLS, 2
NONFINITE, DEGENERATE, ONE_POINT = nat.MODQ_NONFINITE, nat.MODQ_DEGENERATE, nat.MODQ_ONE_POINT

RECORD = np.dtype([("a_re", np.float32), ("a_im", np.float32), ("c_re", np.float32), ("c_im", np.float32),
                   ("s_y", np.float64, (2,)), ("s_yy", np.float64), ("s_ry", np.float64, (2,)), ("s_cy", np.float64, (2,)),
                   ("err_sumsq", np.float64), ("ref_sumsq", np.float64), ("mag_sumsq", np.float64),
                   ("phase_sumsq", np.float64), ("err_peak", np.float32), ("err_peak_k", np.uint32), ("changed", np.uint32),
                   ("flags", np.uint32), ("reserved", np.uint32, (2,))])
assert RECORD.itemsize == 128
SENTINEL_INDEX = np.uint8(0xEE)                    # what process() leaves where the library writes no index ...
SENTINEL = np.complex64(complex(-77.0, 77.0))      # ... and no error vector


def table_of(modulation: Optional[str] = None, points=None) -> np.ndarray:
    """The reference points of a call as [T][2] float32: a named table (analytics.constellation_points rounded to
    float32) or the caller's complex points, 1 .. 64 of them, finite and not all zero."""
    if (modulation is None) == (points is None):
        raise ValueError("either modulation= or points=")
    if modulation is not None:
        if modulation not in MODULATIONS:
            raise ValueError(f"modulation={modulation!r}: one of {', '.join(MODULATIONS)}, or points=")
        return np.ascontiguousarray(constellation_points(modulation), dtype=np.float32)
    p = np.asarray(points)
    if p.ndim == 2 and p.shape[1] == 2 and not np.iscomplexobj(p):
        p = p[:, 0] + 1j * p[:, 1]
    if p.ndim != 1:
        raise ValueError(f"points of shape {p.shape}: [T] complex or [T][2] real")
    if not 1 <= p.size <= MAX_POINTS:
        raise ValueError(f"{p.size} points: 1 .. {MAX_POINTS}")
    with np.errstate(over="ignore"):
        t = np.stack([p.real, p.imag], axis=1).astype(np.float32)
    if not np.all(np.isfinite(t)):
        raise ValueError("points: finite float32 values")
    if not np.any(t):
        raise ValueError("points: not all zero")
    return np.ascontiguousarray(t)


def gray_labels(modulation: Optional[str], T: int) -> np.ndarray:
    """The Gray label of every index of a named table: per axis for the grids in their 2^b ix + iy order, by angle for
    8psk, the index itself for bpsk."""
    i = np.arange(T, dtype=np.uint8)
    if modulation in ("qpsk", "16qam", "64qam"):
        b = (T.bit_length() - 1) // 2
        ix, iy = i >> b, i & ((1 << b) - 1)
        return (((ix ^ (ix >> 1)) << b) | (iy ^ (iy >> 1))).astype(np.uint8)
    if modulation in ("bpsk", "8psk"):
        return i ^ (i >> 1)
    raise ValueError("mapping='gray': a named table (modulation=); a table of the caller's has no Gray order here")


@dataclass
class ModQResult:
    """Per segment, in float64 from the record alone: gain |a|, phase arg a (radians), iq_offset c / |a| (complex, in
    units of the table) and iq_offset_db (against the table's rms), evm_rms sqrt(err_sumsq / ref_sumsq), evm_peak (the
    largest error over the rms reference), mer_db, mag_error_rms (over the rms reference), phase_error_rms_deg, rho
    |S_ry|^2 / (S_rr S_yy), changed (the symbols whose decision moved between the two rounds), flags (NONFINITE,
    DEGENERATE, ONE_POINT); indices [n_seg][K] uint8 and errors [n_seg][K] complex64 (None where they stayed on the
    device or were not asked for), and the records as the library gave them."""
    gain: np.ndarray
    phase: np.ndarray
    iq_offset: np.ndarray
    iq_offset_db: np.ndarray
    evm_rms: np.ndarray
    evm_peak: np.ndarray
    mer_db: np.ndarray
    mag_error_rms: np.ndarray
    phase_error_rms_deg: np.ndarray
    rho: np.ndarray
    changed: np.ndarray
    flags: np.ndarray
    indices: Optional[np.ndarray]
    errors: Optional[np.ndarray]
    records: np.ndarray
    K: int
    table: np.ndarray
    modulation: Optional[str] = None

    def bits(self, mapping: str = "gray") -> np.ndarray:
        """[n_seg][K log2 T] uint8, most significant bit first: the index itself ("natural") or its Gray label ("gray":
        per axis for qpsk / 16qam / 64qam, by angle for 8psk).  T must be a power of two.  SymbolSync's carrier stage
        leaves an M-fold rotation of the constellation open, and with it these bits: resolving it - with a sync word
        through correlate.Correlator, say - is the caller's."""
        if mapping not in ("gray", "natural"):
            raise ValueError(f"mapping={mapping!r}: 'gray' or 'natural'")
        T = int(self.table.shape[0])
        if T & (T - 1):
            raise ValueError(f"{T} points: bits need a power of two")
        if self.indices is None:
            raise ValueError("the indices are in device memory: read them from idx_ptr")
        i = self.indices.astype(np.uint8)
        if mapping == "gray":
            i = gray_labels(self.modulation, T)[i]
        nb = T.bit_length() - 1
        sh = np.arange(nb - 1, -1, -1, dtype=np.uint8)
        return ((i[..., None] >> sh) & 1).reshape(i.shape[0], -1).astype(np.uint8)

    def iq_imbalance(self):
        """(gain_imbalance_db, quadrature_error_deg) per segment, on the host in float64: the least-squares y = alpha r +
        beta conj(r) + gamma from the record's S_y, S_ry, S_cy and the sums of r, |r|^2, r^2 over the decisions (from
        np.bincount of the indices); with rho = beta / alpha, 20 log10(|1 + rho| / |1 - rho|) (I over Q) and
        arg(j (1 - rho) / (1 + rho)) - 90 degrees.  NaN for a segment whose points in use are collinear (bpsk)."""
        if self.indices is None:
            raise ValueError("the indices are in device memory: read them from idx_ptr")
        r = self.table[:, 0].astype(np.float64) + 1j * self.table[:, 1].astype(np.float64)
        n_seg = self.records.size
        g, ph = np.full(n_seg, np.nan), np.full(n_seg, np.nan)
        for s in range(n_seg):
            n = np.bincount(self.indices[s, :self.K], minlength=r.size).astype(np.float64)
            used = r[n > 0]
            if self.records["flags"][s] & (NONFINITE | DEGENERATE) or \
                    np.linalg.matrix_rank(np.stack([used.real, used.imag, np.ones(used.size)], axis=1)) < 3:
                continue
            sr, srr, sr2 = np.sum(n * r), np.sum(n * np.abs(r) ** 2), np.sum(n * r * r)
            rec = self.records[s]
            A = np.array([[srr, np.conj(sr2), np.conj(sr)], [sr2, srr, sr], [sr, np.conj(sr), float(self.K)]])
            b = np.array([complex(*rec["s_ry"]), complex(*rec["s_cy"]), complex(*rec["s_y"])])
            alpha, beta, _ = np.linalg.solve(A, b)
            q = beta / alpha
            g[s] = 20.0 * math.log10(abs(1 + q) / abs(1 - q))
            ph[s] = math.degrees(np.angle(1j * (1 - q) / (1 + q))) - 90.0
        return g, ph


def result_from(records: np.ndarray, indices, errors, K: int, table: np.ndarray, modulation: Optional[str] = None) -> ModQResult:
    """The derived figures of a call's records."""
    r = records
    t64 = table.astype(np.float64)
    rms = math.sqrt(float(np.mean(t64[:, 0] ** 2 + t64[:, 1] ** 2)))
    with np.errstate(all="ignore"):
        a = r["a_re"].astype(np.float64) + 1j * r["a_im"].astype(np.float64)
        c = r["c_re"].astype(np.float64) + 1j * r["c_im"].astype(np.float64)
        gain = np.abs(a)
        off = np.where(gain > 0, c / np.where(gain > 0, gain, 1.0), 0.0)
        ref = r["ref_sumsq"]
        ok = ref > 0
        safe = np.where(ok, ref, 1.0)
        evm = np.where(ok, np.sqrt(r["err_sumsq"] / safe), 0.0)
        peak = np.where(ok, np.sqrt(r["err_peak"].astype(np.float64) / (safe / K)), 0.0)
        mer = np.where(evm > 0, -20.0 * np.log10(np.where(evm > 0, evm, 1.0)), np.inf)
        mag = np.where(ok, np.sqrt(r["mag_sumsq"] / safe), 0.0)
        ph = np.sqrt(r["phase_sumsq"] / K) * 180.0
        den = ref * r["s_yy"]
        rho = np.where(den > 0, (r["s_ry"][:, 0] ** 2 + r["s_ry"][:, 1] ** 2) / np.where(den > 0, den, 1.0), 0.0)
        off_db = 20.0 * np.log10(np.abs(off) / rms)
    return ModQResult(gain, np.angle(a), off, off_db, evm, peak, mer, mag, ph, rho, r["changed"].copy(), r["flags"].copy(),
                      indices, errors, r, int(K), table, modulation)


def check_shape(K: int, in_stride: int, n_seg: int, out_stride: int) -> None:
    """The shape of a call, checked before the library is."""
    if not MIN_SYMBOLS <= int(K) <= MAX_SYMBOLS:
        raise ValueError(f"K={K}: {MIN_SYMBOLS} .. {MAX_SYMBOLS} symbols per segment")
    if int(in_stride) < 1:
        raise ValueError(f"in_stride={in_stride}: at least one symbol")
    if int(n_seg) < 1:
        raise ValueError(f"n_seg={n_seg}: at least one segment")
    if int(out_stride) < int(K):
        raise ValueError(f"out_stride={out_stride}: a segment gives {K} symbols")


class ModQuality(nat._Handle, nat._Timer):
    """Modulation quality of rows of symbols against a table: modulation = "bpsk", "qpsk", "8psk", "16qam" or "64qam", or
    points = up to 64 complex reference points of the caller's.  max_host_symbols: the symbols one process() stages."""
    _destroy = "tdsa_modq_destroy"
    _timer = ("tdsa_modq_timer_begin", "tdsa_modq_timer_end")

    def __init__(self, modulation: Optional[str] = None, points=None, device: int = 0, max_host_symbols: int = 1 << 20):
        if modulation is None and points is None:
            modulation = "qpsk"
        self.table = table_of(modulation, points)
        self.modulation = modulation
        self.device, self.max_host_symbols = int(device), int(max_host_symbols)
        if self.max_host_symbols < 2:
            raise ValueError(f"max_host_symbols={max_host_symbols}: at least 2")
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_modq_create(self.device, self.max_host_symbols, C.byref(self._h)))
        nat.check(nat.lib.tdsa_modq_set_points(self._h, self.table.ctypes.data_as(C.c_void_p), int(self.table.shape[0])))

    def process(self, symbols, K: Optional[int] = None, in_stride: Optional[int] = None, errors: bool = False,
                out_stride: Optional[int] = None) -> ModQResult:
        """Symbols in host memory: [n_seg][K] rows, or one stream of which segment s is the K symbols (default: all of
        them) at s in_stride (default K), every whole segment.  errors=True also returns the error vectors.  With an
        out_stride the outputs are [n_seg][out_stride], SENTINEL_INDEX and SENTINEL where the library writes nothing."""
        a = np.asarray(symbols)
        if not np.iscomplexobj(a) or a.ndim not in (1, 2):
            raise ValueError(f"symbols of dtype {a.dtype} and shape {a.shape}: complex, [n_seg][K] or one stream")
        a = np.ascontiguousarray(a, dtype=np.complex64)
        if a.ndim == 2:
            if K is not None and int(K) != a.shape[1] or in_stride is not None and int(in_stride) != a.shape[1]:
                raise ValueError(f"rows of {a.shape[1]} symbols: K and in_stride are the row length")
            K = in_stride = a.shape[1]
            a = a.reshape(-1)
        K = a.size if K is None else int(K)
        in_stride = K if in_stride is None else int(in_stride)
        if a.size < K:
            raise ValueError(f"{a.size} symbols: less than one segment of {K}")
        n_seg = (a.size - K) // max(in_stride, 1) + 1
        stride = K if out_stride is None else int(out_stride)
        check_shape(K, in_stride, n_seg, stride)
        used = (n_seg - 1) * in_stride + K
        if used > self.max_host_symbols:
            raise ValueError(f"block of {used} symbols: the handle stages at most {self.max_host_symbols} (max_host_symbols)")
        idx = np.full((n_seg, stride), SENTINEL_INDEX, dtype=np.uint8)
        err = np.full((n_seg, stride), SENTINEL, dtype=np.complex64) if errors else None
        rec = np.zeros(n_seg, dtype=RECORD)
        nat.check(nat.lib.tdsa_modq_process(self._h, a.ctypes.data_as(C.c_void_p), used, K, in_stride, n_seg,
                                            idx.ctypes.data_as(C.c_void_p), stride,
                                            err.ctypes.data_as(C.c_void_p) if errors else None, rec.ctypes.data_as(C.c_void_p)))
        if out_stride is None:
            idx, err = idx[:, :K], err[:, :K] if errors else None
        return result_from(rec, idx, err, K, self.table, self.modulation)

    def process_device(self, engine: Optional[SpectrumEngine], ptr: int, K: int, in_stride: int, n_seg: int, idx_ptr: int,
                       out_stride: int, err_ptr: Optional[int] = None) -> ModQResult:
        """Symbols and outputs in device memory, on `engine`'s stream behind its work (None: the handle's own): segment s
        is the K complex64 symbols at ptr + 8 s in_stride - SymbolSync.process_device's out_ptr and out_stride; its indices
        go to idx_ptr + s out_stride and, with err_ptr, its error vectors to err_ptr + 8 s out_stride.  Returns when the
        records have arrived; `indices` and `errors` of the result are None: they are at idx_ptr and err_ptr."""
        check_shape(K, in_stride, n_seg, out_stride)
        if not ptr or not idx_ptr:
            raise ValueError("null pointer")
        if int(ptr) % 8:
            raise ValueError("symbols pointer must be aligned to one complex64 symbol (8 bytes)")
        if err_ptr and int(err_ptr) % 8:
            raise ValueError("errors pointer must be aligned to one complex64 error vector (8 bytes)")
        if engine is not None:
            check_same_device(engine.device, self.device)
        rec = np.zeros(int(n_seg), dtype=RECORD)
        nat.check(nat.lib.tdsa_modq_process_dev(self._h, engine._h if engine is not None else None, C.c_void_p(int(ptr)),
                                                int(K), int(in_stride), int(n_seg), C.c_void_p(int(idx_ptr)), int(out_stride),
                                                C.c_void_p(int(err_ptr)) if err_ptr else None, rec.ctypes.data_as(C.c_void_p)))
        return result_from(rec, None, None, int(K), self.table, self.modulation)
