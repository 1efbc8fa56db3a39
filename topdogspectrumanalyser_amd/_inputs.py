"""What the measurement handles share on the way in: IQ streams (PowerStats, PulseAnalyzer, Correlator) and float32 dB rows
(SignalDetector, ChannelMeasure).  Each mixin holds the staging limit of the host entry point, the checks of the input
and both process calls; _process names the library's (host, device) pair, as _destroy and _timer name theirs."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat
from .zoom import check_same_device

FORMATS = {np.dtype(np.int8): nat.IN_I8, np.dtype(np.uint8): nat.IN_U8, np.dtype(np.complex64): nat.IN_C64}


class _IqStreams:
    """`self.streams` IQ streams in int8 / uint8 pairs or complex64, accumulated on the device: neither call returns
    anything."""
    _process = ("", "")

    def _stage(self, max_host_samples: Optional[int]) -> None:
        """max_host_samples of the constructor: the samples, all streams together, one library call stages."""
        if max_host_samples is None:
            max_host_samples = max(1 << 21, self.streams)      # 16 MiB of pinned staging
        self.max_host_samples = int(max_host_samples)
        if self.max_host_samples < self.streams:
            raise ValueError(f"max_host_samples={max_host_samples}: at least one sample per stream ({self.streams})")

    def process(self, iq) -> None:
        """Samples in host memory.  The dtype names the format: int8 or uint8 (interleaved I, Q: a last axis of even
        length) or complex64.  One stream: a 1-D array; more: [streams][...].  A block above the staging goes in pieces,
        which changes no integer of the result."""
        a = np.asarray(iq)
        if a.dtype.kind == "c":
            a = a.astype(np.complex64, copy=False)
        fmt = FORMATS.get(a.dtype)
        if fmt is None:
            raise ValueError(f"samples of dtype {a.dtype}: int8 or uint8 (interleaved I, Q) or complex64")
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.streams:
            raise ValueError(f"samples of shape {np.shape(iq)}: [{self.streams}][n], or [n] for one stream")
        per = 1 if fmt == nat.IN_C64 else 2
        if a.shape[1] % per:
            raise ValueError(f"{a.shape[1]} bytes per stream: interleaved I, Q pairs")
        a = np.ascontiguousarray(a)
        n, most = a.shape[1] // per, self.max_host_samples // self.streams
        call = getattr(nat.lib, self._process[0])
        for k in range(0, n, most):
            nat.check(call(self._h, fmt, C.c_void_p(a.ctypes.data + k * per * a.itemsize), min(most, n - k), n))

    def process_device(self, engine, ptr: int, n: int, stride: Optional[int] = None, in_format: int = nat.IN_C64) -> None:
        """n samples per stream already in device memory, stream c at ptr + c * stride samples (default: n), on
        `engine`'s stream behind its work (None: the handle's own).  Does not wait: read() does."""
        n = int(n)
        stride = n if stride is None else int(stride)
        if in_format not in (nat.IN_I8, nat.IN_U8, nat.IN_C64):
            raise ValueError(f"in_format={in_format}: IN_I8, IN_U8 or IN_C64")
        if n < 0:
            raise ValueError(f"n={n}")
        if not ptr:
            raise ValueError("null pointer")
        unit = 8 if in_format == nat.IN_C64 else 2
        if int(ptr) % unit:
            raise ValueError(f"samples pointer must be aligned to one sample ({unit} bytes)")
        if self.streams > 1 and stride < n:
            raise ValueError(f"stride={stride}: below the call's {n} samples per stream")
        if engine is not None:
            check_same_device(engine.device, self.device)
        nat.check(getattr(nat.lib, self._process[1])(self._h, engine._h if engine is not None else None, in_format,
                                                     C.c_void_p(int(ptr)), n, stride))


ONE = 1 << 32                          # one sample, and one turn of the symbol clock, in 32.32 fixed point
MIN_SPS, MAX_SPS = 4.0, 64.0
MAX_SYMBOLS = 4096


def fixed_step(samples_per_symbol: float) -> int:
    """round(sps 2^32): samples per symbol in 32.32 fixed point."""
    return int(round(float(samples_per_symbol) * ONE))


def phase_step(samples_per_symbol: float) -> int:
    """round(2^32 / sps): the symbol clock's phase step per sample."""
    return int(round(ONE / float(samples_per_symbol)))


class _Segments:
    """Segments of seg_len samples, `hop` apart, each analysed on its own at the symbol clock of the constructor: K
    outputs per segment, an optional second output of the same shape and one record.  A handle supplies _k(seg_len), its
    K formula, _record, the dtype of a record, and _filled, the (sentinel, dtype) of either output."""
    _process = ("", "")
    _record = None
    _filled = ((), ())

    def _rate(self, samples_per_symbol: float) -> None:
        """samples_per_symbol of the constructor: step and nu."""
        sps = float(samples_per_symbol)
        if not MIN_SPS <= sps <= MAX_SPS:
            raise ValueError(f"samples_per_symbol={samples_per_symbol}: {MIN_SPS:g} .. {MAX_SPS:g}")
        self.samples_per_symbol = sps
        self.step, self.nu = fixed_step(sps), phase_step(sps)

    def _stage(self, timing, device: int, max_host_samples: int) -> None:
        """timing ("auto", or the first symbol's position in samples), device and max_host_samples of the constructor."""
        if isinstance(timing, str):
            if timing != "auto":
                raise ValueError(f"timing={timing!r}: 'auto' or the first symbol's position in samples")
            self.timing_mode, self.delta_fx = nat.SYMSYNC_AUTO, 0
        else:
            self.timing_mode, self.delta_fx = nat.SYMSYNC_FIXED, int(round(float(timing) * ONE))
            if not ONE <= self.delta_fx < self.step + ONE:
                raise ValueError(f"timing={timing}: 1 <= timing < samples_per_symbol + 1")
        self.device = int(device)
        self.max_host_samples = int(max_host_samples)
        if self.max_host_samples < 16:
            raise ValueError(f"max_host_samples={max_host_samples}: at least 16")

    def symbols_per_segment(self, seg_len: int) -> int:
        """K of a segment of seg_len samples; ValueError outside 2 .. 4096."""
        K = self._k(seg_len)
        if not 2 <= K <= MAX_SYMBOLS:
            raise ValueError(f"seg_len={seg_len} gives {K} symbols per segment: 2 .. {MAX_SYMBOLS}")
        return K

    def _check(self, seg_len: int, hop: int, n_seg: int, out_stride: int) -> int:
        K = self.symbols_per_segment(seg_len)
        if int(hop) < 1:
            raise ValueError(f"hop={hop}: at least one sample")
        if int(n_seg) < 1:
            raise ValueError(f"n_seg={n_seg}: at least one segment")
        if int(out_stride) < K:
            raise ValueError(f"out_stride={out_stride}: a segment gives {K} symbols")
        return K

    def _host(self, a: np.ndarray, seg_len: int, hop: Optional[int], out_stride: Optional[int], second: bool):
        """The host call over the stream a: every whole segment of seg_len samples, `hop` (default seg_len) apart.
        Returns (K, records, outputs, second outputs or None); the outputs are [n_seg][out_stride] with the sentinel where
        the library writes nothing, or [n_seg][K] where no out_stride is given."""
        seg_len = int(seg_len)
        hop = seg_len if hop is None else int(hop)
        if a.size < seg_len:
            raise ValueError(f"{a.size} samples: less than one segment of {seg_len}")
        n_seg = (a.size - seg_len) // max(hop, 1) + 1
        K = self.symbols_per_segment(seg_len)
        stride = K if out_stride is None else int(out_stride)
        self._check(seg_len, hop, n_seg, stride)
        used = (n_seg - 1) * hop + seg_len
        if used > self.max_host_samples or n_seg * seg_len > self.max_host_samples:
            raise ValueError(f"{n_seg} segments of {seg_len} samples: the handle stages at most {self.max_host_samples} "
                             "(max_host_samples)")
        out, aux = (np.full((n_seg, stride), fill, dtype=dtype) if wanted else None
                    for wanted, (fill, dtype) in zip((True, second), self._filled))
        rec = np.zeros(n_seg, dtype=self._record)
        nat.check(getattr(nat.lib, self._process[0])(self._h, a.ctypes.data_as(C.c_void_p), used, seg_len, hop, n_seg,
                                                     out.ctypes.data_as(C.c_void_p), stride,
                                                     aux.ctypes.data_as(C.c_void_p) if second else None,
                                                     rec.ctypes.data_as(C.c_void_p)))
        if out_stride is None:
            out, aux = out[:, :K], aux[:, :K] if second else None
        return K, rec, out, aux

    @staticmethod
    def timing_quality(records: np.ndarray) -> np.ndarray:
        """|C| / P of a call's records, the depth of the symbol-rate line; 0 where P is not above 0."""
        with np.errstate(all="ignore"):
            p = records["p"].astype(np.float64)
            c = np.hypot(records["c_re"].astype(np.float64), records["c_im"].astype(np.float64))
            return np.where(p > 0, c / np.where(p > 0, p, 1.0), 0.0)


class _DbRows:
    """[n_rows][self.n_bins] float32 dB rows; each call returns the records of its rows.  A handle supplies
    _records(n_rows), the two empty record arrays of a call, and _result(rows, sub), what a call returns for them."""
    _process = ("", "")

    def _stage(self, max_host_rows: Optional[int]) -> None:
        """max_host_rows of the constructor: the rows one host call stages."""
        if max_host_rows is None:
            max_host_rows = max(1, min(4096, (16 << 20) // (4 * self.n_bins)))     # 16 MiB of pinned staging
        self.max_host_rows = int(max_host_rows)
        if self.max_host_rows < 1:
            raise ValueError(f"max_host_rows={max_host_rows}: at least 1")

    def _call(self, fn: str, n_rows: int, *args):
        rr, sub = self._records(n_rows)
        nat.check(getattr(nat.lib, fn)(self._h, *args, n_rows, rr.ctypes.data_as(C.c_void_p), sub.ctypes.data_as(C.c_void_p)))
        return self._result(rr, sub)

    def process(self, rows):
        """Rows in host memory, [n_rows][n_bins] (or one row), float32."""
        a = np.asarray(rows)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != self.n_bins or a.dtype.kind not in "fiu":
            raise ValueError(f"rows of dtype {a.dtype} and shape {a.shape}: [n_rows][{self.n_bins}] real values")
        if a.shape[0] > self.max_host_rows:
            raise ValueError(f"{a.shape[0]} rows: the handle stages at most {self.max_host_rows} (max_host_rows)")
        a = np.ascontiguousarray(a, dtype=np.float32)
        return self._call(self._process[0], a.shape[0], a.ctypes.data_as(C.c_void_p))

    def process_device(self, engine, rows_dev: int, n_rows: int):
        """Rows already in device memory, n_rows of n_bins float32 back to back at rows_dev, on `engine`'s stream behind
        its work (None: the handle's own).  Returns when the records have arrived; no row leaves the device."""
        n_rows = int(n_rows)
        if n_rows < 0:
            raise ValueError(f"n_rows={n_rows}")
        if not rows_dev:
            raise ValueError("null pointer")
        if int(rows_dev) % 4:
            raise ValueError("rows pointer must be aligned to one float32 (4 bytes)")
        if engine is not None:
            check_same_device(engine.device, self.device)
        return self._call(self._process[1], n_rows, engine._h if engine is not None else None, C.c_void_p(int(rows_dev)))
