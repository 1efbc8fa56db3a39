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
