"""DeviceBuffer on the MI355X: byte-exact round trips at odd sizes and offsets with the rest of the buffer untouched, the
base alignment, addresses from .at() into a device entry point, and the close-once rule against the real allocator."""
import numpy as np
import pytest

from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.mark.parametrize("nbytes", [0, 1, 7, 8, 4097, (1 << 20) + 3])
def test_round_trips_leave_the_rest_intact(nbytes):
    rng = np.random.default_rng(nbytes)
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    data[data == SENTINEL] = 0
    size = nbytes + 32
    with DeviceBuffer(size) as buf:
        assert buf.ptr % 256 == 0
        for offset in (0, 4, 12):
            buf.put(np.full(size, SENTINEL, np.uint8))
            assert buf.put(data, offset) is buf
            assert np.array_equal(buf.get(nbytes, np.uint8, offset), data)
            whole = buf.get(size, np.uint8)
            assert np.all(whole[:offset] == SENTINEL) and np.all(whole[offset + nbytes:] == SENTINEL)
            assert np.array_equal(whole[offset:offset + nbytes], data)


def test_of_and_typed_get():
    a = np.random.default_rng(1).standard_normal((3, 5)).astype(np.float32)
    with DeviceBuffer.of(a) as buf:
        assert buf.size == a.nbytes
        assert np.array_equal(buf.get((3, 5), np.float32), a)
        assert np.array_equal(buf.get(5, np.float32, 4 * 5), a[1])


def test_addresses_from_at_feed_a_device_entry_point():
    """One frame of N = 64 read from buf.at(2), an address that is only int8-pair aligned: process_device equals
    process() of the same bytes bit for bit."""
    n = 64
    iq = np.random.default_rng(2).integers(-128, 128, 2 * n, dtype=np.int8)
    with SpectrumEngine(n, max_frames=1) as e, DeviceBuffer(2 + iq.nbytes) as d_in, DeviceBuffer(4 * n) as d_out:
        e.set_window(np.hanning(n).astype(np.float32))
        e.configure(db_mode="mag", log_floor=1e-12, dc_alpha=-1.0)      # no state carried from one call to the next
        want = e.process(iq)
        d_in.put(iq, 2)
        e.process_device(nat.IN_I8, d_in.at(2, iq.nbytes), n, n, 1, d_out.ptr)
        e.synchronize()
        got = d_out.get((1, n), np.float32)
    assert want.shape == got.shape and np.array_equal(want.view(np.uint32), got.view(np.uint32))


def test_close_twice_and_allocate_again():
    buf = DeviceBuffer(4096)
    buf.put(np.arange(1024, dtype=np.float32))
    buf.close()
    buf.close()
    with pytest.raises(ValueError):
        buf.ptr
    with DeviceBuffer(4096) as again:
        a = np.arange(1024, dtype=np.float32)[::-1]
        assert np.array_equal(again.put(a).get(1024, np.float32), a)
