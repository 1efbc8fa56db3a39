"""Memory on the device: the addresses every process_device / push_device / run_device entry point takes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat

MIN_ALLOC = 16       # bytes asked of the allocator at the least, so that a 0-byte buffer still has an address


def read_device(ptr: int, shape, dtype, device: int = 0) -> np.ndarray:
    """Device to host from an address the caller does not own (rows a pipe or a view handed out): a new array of `shape`
    and `dtype`.  The same blocking copy as DeviceBuffer.get, not ordered against any stream, and with no buffer to check
    the range against: the extent is the caller's to know."""
    out = np.empty(shape, dtype=dtype)
    nat.check(nat.lib.tdsa_memcpy_d2h(int(device), out.ctypes.data_as(C.c_void_p), C.c_void_p(int(ptr)), out.nbytes))
    return out


class DeviceBuffer(nat._Handle):
    """`nbytes` of device memory on `device`: freed by close(), on leaving a `with` block, or when collected.

    Addresses come from .ptr and .at(offset, nbytes); at, put and get check their range against `size` (the bytes asked
    for, not the MIN_ALLOC the allocator may have been asked for) before any library call, and raise ValueError after
    close().

    put and get are blocking copies (tdsa_memcpy_h2d / tdsa_memcpy_d2h) and are NOT ordered against a handle's
    non-blocking stream: wait for the work that reads or writes the buffer (engine.synchronize(), or the handle's own
    wait) before get, and before a put that overwrites what queued work still reads.  To copy on a plan's stream use
    tdsa_plan_copy."""

    def __init__(self, nbytes: int, device: int = 0):
        self._p = None
        self.size = int(nbytes)
        self.device = int(device)
        if self.size < 0:
            raise ValueError(f"nbytes={nbytes}")
        p = C.c_void_p()
        nat.check(nat.lib.tdsa_dev_alloc(self.device, max(self.size, MIN_ALLOC), C.byref(p)))
        self._p = int(p.value)

    @classmethod
    def of(cls, array, device: int = 0) -> "DeviceBuffer":
        """A buffer of the array's bytes, holding them."""
        a = np.ascontiguousarray(array)
        return cls(a.nbytes, device).put(a)

    def close(self) -> None:
        """Frees once; TdsaError if the library reports a failed free (the buffer counts as closed either way)."""
        p, self._p = getattr(self, "_p", None), None
        if p is not None:
            nat.check(nat.lib.tdsa_dev_free(self.device, C.c_void_p(p)))

    @property
    def ptr(self) -> int:
        """The base address."""
        return self.at(0)

    def at(self, offset: int, nbytes: int = 0) -> int:
        """The address `offset` bytes in; ValueError unless [offset, offset + nbytes) lies within the buffer."""
        if self._p is None:
            raise ValueError("DeviceBuffer is closed")
        offset, nbytes = int(offset), int(nbytes)
        if offset < 0 or nbytes < 0 or offset + nbytes > self.size:
            raise ValueError(f"bytes {offset} .. {offset + nbytes} of a DeviceBuffer of {self.size}")
        return self._p + offset

    def put(self, array, offset: int = 0) -> "DeviceBuffer":
        """Host to device, the array's bytes to `offset`; returns self."""
        a = np.ascontiguousarray(array)
        dst = self.at(offset, a.nbytes)
        nat.check(nat.lib.tdsa_memcpy_h2d(self.device, C.c_void_p(dst), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return self

    def get(self, shape, dtype, offset: int = 0) -> np.ndarray:
        """Device to host: a new array of `shape` and `dtype` from the bytes at `offset`."""
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        return read_device(self.at(offset, nbytes), shape, dtype, self.device)
