"""DeviceBuffer (devmem.py) without a GPU: a fake library backs "device" memory with host buffers, counts its calls and can
be told to fail, so the bounds, the 16-byte minimum, the device argument and the close-once rule are pinned on the CPU.
Also here: device memory is handled by DeviceBuffer alone (the Python twin of test_lane_level_idioms_are_written_once)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from topdogspectrumanalyser_amd import DeviceBuffer, _native as nat
from topdogspectrumanalyser_amd.devmem import read_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = -2


class FakeLib:
    """tdsa_dev_alloc / tdsa_dev_free / tdsa_memcpy_h2d / tdsa_memcpy_d2h over host memory.  backed=False hands out an
    address with nothing behind it and only records the copies (for sizes no test should allocate)."""

    def __init__(self, backed=True):
        self.backed = backed
        self.calls = []                        # (name, device, ...) in order
        self.live = {}                         # address -> ctypes buffer (None when not backed)
        self.fail_alloc = self.fail_free = False

    def tdsa_last_error_string(self):
        return b"fake failure"

    def tdsa_dev_alloc(self, device, nbytes, out):
        self.calls.append(("alloc", device, nbytes))
        if self.fail_alloc:
            self.fail_alloc = False
            return ERR
        buf = C.create_string_buffer(nbytes) if self.backed else None
        addr = C.addressof(buf) if self.backed else 1 << 40
        self.live[addr] = buf
        out._obj.value = addr
        return 0

    def tdsa_dev_free(self, device, p):
        self.calls.append(("free", device, p.value))
        if self.fail_free:
            self.fail_free = False
            return ERR
        del self.live[p.value]
        return 0

    def _inside(self, addr, n):
        return any(base <= addr and addr + n <= base + len(buf) for base, buf in self.live.items() if buf is not None)

    def tdsa_memcpy_h2d(self, device, dst, src, n):
        self.calls.append(("h2d", device, dst.value, n))
        if self.backed:
            assert self._inside(dst.value, n)
            C.memmove(dst.value, src, n)
        return 0

    def tdsa_memcpy_d2h(self, device, dst, src, n):
        self.calls.append(("d2h", device, src.value, n))
        if self.backed:
            assert self._inside(src.value, n)
            C.memmove(dst, src.value, n)
        return 0


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(nat, "lib", fake)
    return fake


@pytest.fixture
def unbacked(monkeypatch):
    fake = FakeLib(backed=False)
    monkeypatch.setattr(nat, "lib", fake)
    return fake


def test_round_trips_at_offsets(lib):
    size = 64
    for dtype, count in ((np.uint8, 5), (np.float32, 3), (np.complex64, 2)):
        a = (np.arange(count) + 1).astype(dtype)
        for offset in (0, 1, 7, size - a.nbytes):
            with DeviceBuffer(size) as buf:
                buf.put(np.full(size, 0xEE, np.uint8))
                assert buf.put(a, offset) is buf
                got = buf.get(count, dtype, offset)
                assert got.dtype == dtype and np.array_equal(got, a)
                whole = buf.get(size, np.uint8)
                assert np.all(whole[:offset] == 0xEE) and np.all(whole[offset + a.nbytes:] == 0xEE)
    assert not lib.live


def test_put_makes_the_array_contiguous_and_get_takes_a_shape(lib):
    a = np.arange(24, dtype=np.int16).reshape(4, 6)
    with DeviceBuffer.of(a[:, ::2]) as buf:
        assert buf.size == 4 * 3 * 2
        assert np.array_equal(buf.get((4, 3), np.int16), a[:, ::2])


def test_of_round_trips(lib):
    a = np.random.default_rng(0).standard_normal(33).astype(np.float32)
    with DeviceBuffer.of(a) as buf:
        assert buf.size == a.nbytes and lib.calls[0] == ("alloc", 0, a.nbytes)
        assert np.array_equal(buf.get(a.shape, a.dtype), a)


def test_read_device_is_the_same_blocking_copy_from_an_address_it_does_not_own(lib):
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    with DeviceBuffer.of(a, device=1) as buf:
        lib.calls.clear()
        got = read_device(buf.ptr + 16, (2, 4), np.float32, device=1)
        assert got.dtype == np.float32 and np.array_equal(got, a[1:])
        assert lib.calls == [("d2h", 1, buf.ptr + 16, 32)]
        lib.calls.clear()
        buf.get((2, 4), np.float32, 16)
        assert lib.calls == [("d2h", 1, buf.ptr + 16, 32)]      # get is that call behind a bounds check


def test_device_reaches_all_four_calls(lib):
    with DeviceBuffer.of(np.zeros(4, np.float32), device=3) as buf:
        assert buf.device == 3
        buf.get(4, np.float32)
    assert [c[0] for c in lib.calls] == ["alloc", "h2d", "d2h", "free"]
    assert [c[1] for c in lib.calls] == [3, 3, 3, 3]
    lib.calls.clear()
    DeviceBuffer(8, 2).close()
    assert [c[:2] for c in lib.calls] == [("alloc", 2), ("free", 2)]


def test_minimum_goes_to_the_allocator_and_bounds_use_the_requested_size(lib):
    for asked, given in ((0, 16), (1, 16), (15, 16), (16, 16), (17, 17)):
        lib.calls.clear()
        with DeviceBuffer(asked) as buf:
            assert lib.calls == [("alloc", 0, given)] and buf.size == asked
            with pytest.raises(ValueError):
                buf.at(asked, 1)
            assert buf.at(asked) == buf.ptr + asked
    with DeviceBuffer(0) as buf:
        buf.put(np.empty(0, np.float32))                       # nothing into nothing
        assert buf.get(0, np.uint8).size == 0
        n = len(lib.calls)
        with pytest.raises(ValueError):
            buf.put(np.zeros(1, np.uint8))
        with pytest.raises(ValueError):
            buf.get(1, np.uint8)
        assert len(lib.calls) == n


def test_out_of_range_raises_before_any_library_call(lib):
    with DeviceBuffer(32) as buf:
        n = len(lib.calls)
        one, nine = np.zeros(1, np.uint8), np.zeros(9, np.uint8)
        for bad in (lambda: buf.at(-1), lambda: buf.at(-1, 1), lambda: buf.at(33), lambda: buf.at(32, 1),
                    lambda: buf.at(24, 9), lambda: buf.at(0, 33), lambda: buf.at(0, -1),
                    lambda: buf.put(one, -1), lambda: buf.put(one, 32), lambda: buf.put(nine, 24),
                    lambda: buf.get(1, np.uint8, -1), lambda: buf.get(1, np.uint8, 32), lambda: buf.get(9, np.uint8, 24),
                    lambda: buf.get((3, 3), np.float32)):
            with pytest.raises(ValueError):
                bad()
        assert len(lib.calls) == n
        assert buf.at(24, 8) == buf.ptr + 24 and buf.at(32) == buf.ptr + 32
        buf.put(np.zeros(8, np.uint8), 24)
        buf.get(8, np.uint8, 24)
        assert len(lib.calls) == n + 2


def test_offsets_past_2_to_the_32_are_python_ints(unbacked):
    size, offset = 2 ** 32 + 8, 2 ** 32
    with DeviceBuffer(size) as buf:
        assert unbacked.calls == [("alloc", 0, size)]
        assert buf.at(offset, 8) == buf.ptr + offset and buf.at(offset, 8) - buf.ptr == 2 ** 32
        buf.put(np.zeros(8, np.uint8), offset)
        buf.get(1, np.complex64, offset)
        assert unbacked.calls[1:] == [("h2d", 0, buf.ptr + offset, 8), ("d2h", 0, buf.ptr + offset, 8)]
        for bad in (lambda: buf.at(offset, 9), lambda: buf.put(np.zeros(9, np.uint8), offset),
                    lambda: buf.get(9, np.uint8, offset)):
            with pytest.raises(ValueError):
                bad()
        assert len(unbacked.calls) == 3


def test_close_frees_once(lib):
    buf = DeviceBuffer(8)
    buf.close()
    n = len(lib.calls)
    assert lib.calls[-1][0] == "free" and not lib.live
    buf.close()
    with buf:
        pass
    del buf
    assert len(lib.calls) == n


def test_close_after_a_failed_allocation_makes_no_call(lib):
    lib.fail_alloc = True
    made = []

    class Kept(DeviceBuffer):
        def __init__(self, *a):
            made.append(self)
            super().__init__(*a)

    with pytest.raises(nat.TdsaError, match="fake failure"):
        Kept(8)
    assert lib.calls == [("alloc", 0, 16)]
    made[0].close()
    made.pop().__del__()
    assert lib.calls == [("alloc", 0, 16)]


def test_failed_free_raises_from_close_and_not_from_del(lib):
    buf = DeviceBuffer(8)
    lib.fail_free = True
    with pytest.raises(nat.TdsaError):
        buf.close()
    n = len(lib.calls)
    buf.close()                                                # closed all the same: not freed twice
    assert len(lib.calls) == n
    other = DeviceBuffer(8)
    lib.fail_free = True
    other.__del__()                                            # swallowed
    assert lib.calls[-1][0] == "free" and not lib.fail_free
    with pytest.raises(ValueError):
        other.ptr


def test_use_after_close_raises(lib):
    buf = DeviceBuffer(8)
    buf.close()
    n = len(lib.calls)
    for bad in (lambda: buf.ptr, lambda: buf.at(0), lambda: buf.put(np.zeros(1, np.uint8)), lambda: buf.get(1, np.uint8)):
        with pytest.raises(ValueError):
            bad()
    assert len(lib.calls) == n


def test_negative_size_is_refused(lib):
    with pytest.raises(ValueError):
        DeviceBuffer(-1)
    assert not lib.calls


def test_close_all_closes_what_exists_in_order(lib):
    order = []

    class H(nat._Handle):
        def __init__(self, name, h=1):
            self.name, self._h = name, h

        def synchronize(self):
            order.append("wait " + self.name)

        def close(self):
            order.append("close " + self.name)

    class Owner:
        pass

    o = Owner()
    o.engine, o.a, o.pair, o.inner = H("engine"), H("a"), [H("y0"), H("y1")], None
    nat._close_all(o, "pair", "a", "missing", "inner", "engine", wait="engine")
    assert order == ["wait engine", "close y0", "close y1", "close a", "close engine"]
    order.clear()
    o.engine._h = None                                         # an engine already closed is not waited for
    nat._close_all(o, "a", wait="engine")
    nat._close_all(o, "a", wait="nothing")
    assert order == ["close a", "close a"]


def test_device_memory_is_handled_in_one_place():
    """The four C-ABI functions for device memory are named by _native.py's signature table and devmem.py alone (and by
    tools/ubench/, which stays as it is, and this file's fake of them); the old private allocator is gone."""
    names = re.compile(r"tdsa_dev_alloc|tdsa_dev_free|tdsa_memcpy_h2d|tdsa_memcpy_d2h|\b_dev_alloc\b|class _Dev\b|\bDevRows\b")
    allowed = {os.path.join("topdogspectrumanalyser_amd", "_native.py"), os.path.join("topdogspectrumanalyser_amd", "devmem.py"),
               os.path.relpath(os.path.abspath(__file__), ROOT)}
    hits, seen = [], 0
    for top, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if not d.startswith(".") and d not in ("_ref", "__pycache__")]
        rel_top = os.path.relpath(top, ROOT)
        if rel_top == os.path.join("tools", "ubench"):
            dirs[:] = []
            continue
        for f in files:
            rel = os.path.normpath(os.path.join(rel_top, f))
            if f.endswith(".py") and rel not in allowed:
                seen += 1
                text = open(os.path.join(top, f), errors="replace").read()
                hits += [(rel, m) for m in sorted(set(names.findall(text)))]
    assert seen > 100 and not hits, hits
    native = open(os.path.join(ROOT, "topdogspectrumanalyser_amd", "_native.py")).read()
    for name in ("tdsa_dev_alloc", "tdsa_dev_free", "tdsa_memcpy_h2d", "tdsa_memcpy_d2h"):
        assert native.count(name) == 1, name                   # the signature table, nothing else
