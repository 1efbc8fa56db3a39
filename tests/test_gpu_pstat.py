"""The power statistics on the device (tdsa_pstat_*) against tests/pstat_contract.py: the
records, msum and hist under np.array_equal, whatever the shape, the format, the entry point, the load path or the split
into calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pstat_contract as pc
from device_room import room_or_skip
from kernel_build import CSRC
from topdogspectrumanalyser_amd import Channelizer, DeviceBuffer, DownConverter, PowerStats, SpectrumEngine
from topdogspectrumanalyser_amd import _native as nat

pytestmark = pytest.mark.gpu


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, "tdsa_pstat.hpp")).read()).group(1))


T = _const("kPstatTile")
MAX_GRID = _const("kPstatMaxGrid")
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 1)
DTYPE = {pc.I8: np.int8, pc.U8: np.uint8, pc.C64: np.complex64}
GAP = {pc.I8: np.int8(-128), pc.U8: np.uint8(255), pc.C64: np.complex64(complex(np.nan, np.nan))}   # I8: 0x80


def _per(fmt):
    return 1 if fmt == pc.C64 else 2


def _noise(fmt, C_, n, seed):
    """[C][n] complex64 or [C][2 n] bytes: noise, every stream at a level of its own so that the octaves differ."""
    rng = np.random.default_rng(seed)
    if fmt == pc.C64:
        x = rng.standard_normal((C_, n)) + 1j * rng.standard_normal((C_, n))
        return (x * (2.0 ** -(np.arange(C_) % 9))[:, None]).astype(np.complex64)
    lo, hi = (-128, 128) if fmt == pc.I8 else (0, 256)
    return rng.integers(lo, hi, (C_, 2 * n)).astype(DTYPE[fmt])


def _want(x2d, fmt, exp_lo=-40, gate=0.0):
    return pc.run(list(x2d), fmt, exp_lo, gate)


def _same(got, want, tag=""):
    rec, msum, hist = want
    for f in pc.RECORD.names:
        assert np.array_equal(got.records[f], rec[f]), (tag, f, got.records[f][:4], rec[f][:4])
    assert np.array_equal(got.msum, msum), (tag, "msum", np.argwhere(got.msum != msum)[:4])
    assert np.array_equal(got.hist, hist), (tag, "hist", np.argwhere(got.hist != hist)[:4])


def _feed_device(p, x2d, fmt, extra=0, offset=0, engine=None):
    """The streams through the device entry point: `offset` samples into a 16-byte aligned buffer, in_stride = n + extra,
    the gaps (and the lead) filled with samples that would show if they were counted.  Waits, so the buffer may go."""
    x2d = np.ascontiguousarray(x2d)
    per, unit = _per(fmt), 8 // (1 if fmt == pc.C64 else 4)
    n, stride = x2d.shape[1] // per, x2d.shape[1] // per + extra
    full = np.full((x2d.shape[0], stride * per), GAP[fmt], dtype=DTYPE[fmt])
    full[:, :n * per] = x2d
    with DeviceBuffer(full.nbytes + offset * unit + 16) as buf:
        assert buf.ptr % 16 == 0
        if offset:
            buf.put(np.full(offset * per, GAP[fmt], dtype=DTYPE[fmt]))
        buf.put(full, offset * unit)
        p.process_device(engine, buf.at(offset * unit, full.nbytes), n, stride, fmt)
        return p.read()


# ---- shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (1, 2, 3, 256))
@pytest.mark.parametrize("fmt", (pc.I8, pc.U8, pc.C64))
def test_every_length_stream_count_format_entry_point_and_stride(fmt, C_):
    with PowerStats(C_, max_host_samples=C_ * SIZES[-1]) as p:
        for n in SIZES:
            x = _noise(fmt, C_, n, 100 * n + C_)
            want = _want(x, fmt)
            p.reset()
            p.process(x)
            _same(p.read(), want, ("host", n))
            for extra in (0, 1, 7):                       # an odd stride: the streams alternate between the load paths
                p.reset()
                _same(_feed_device(p, x, fmt, extra), want, ("device", n, extra))


@pytest.mark.parametrize("fmt", (pc.I8, pc.U8, pc.C64))
def test_a_base_pointer_one_sample_off_16_bytes(fmt):
    for C_ in (1, 3):
        with PowerStats(C_) as p:
            for n in (1, 65, T + 1, 3 * T + 1):
                x = _noise(fmt, C_, n, n + C_)
                want = _want(x, fmt)
                for offset, extra in ((1, 0), (1, 1), (3, 4)):
                    p.reset()
                    _same(_feed_device(p, x, fmt, extra, offset), want, (C_, n, offset, extra))


# ---- inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (pc.I8, pc.U8, pc.C64))
def test_a_constant_envelope_is_one_bin_and_one_octave(fmt):
    value = {pc.I8: [64, -64], pc.U8: [200, 31], pc.C64: [0.25 - 0.5j]}[fmt]
    with PowerStats(2) as p:
        for n in (T, 3 * T + 1):
            x = np.tile(np.array(value, dtype=DTYPE[fmt]), (2, n))
            want = _want(x, fmt)
            assert np.count_nonzero(want[2][0]) == 1 and np.count_nonzero(want[1][0]) == 1 and want[2].max() == n
            p.reset()
            p.process(x)
            _same(p.read(), want, ("host", n))
            for offset in (0, 1):
                p.reset()
                _same(_feed_device(p, x, fmt, 0, offset), want, ("device", n, offset))


def test_exact_edges_specials_and_a_denormal_power():
    for exp_lo in (-126, -40, 64):
        x = np.concatenate([pc.edge_set(exp_lo)[0], pc.specials()[0]])
        x = np.stack([x, x[::-1]])
        want = _want(x, pc.C64, exp_lo)
        with PowerStats(2, exp_lo=exp_lo) as p:
            p.process(x)
            _same(p.read(), want, ("host", exp_lo))
            p.reset()
            _same(_feed_device(p, x, pc.C64, 1), want, ("device", exp_lo))
    # re = 2^-70: p = 2^-140, a denormal float32, must arrive as 2^9 units of 2^-149 and not as zero
    with PowerStats(1) as p:
        p.process(np.full(70, 2.0 ** -70, dtype=np.complex64))
        s = p.read()
    assert int(s.n_under[0]) == 70 and int(s.n_zero[0]) == 0 and int(s.msum[0, 0]) == 70 << 9 and not s.msum[0, 1:].any()
    assert int(s.min_bits[0]) == int(s.max_bits[0]) == 1 << 9 and s.mean_power[0] == 2.0 ** -140


@pytest.mark.parametrize("fmt", (pc.I8, pc.U8))
def test_all_65536_byte_pairs(fmt):
    i, q = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    x = np.stack([i.ravel(), q.ravel()], axis=1).astype(np.uint8).view(DTYPE[fmt]).reshape(1, -1)
    want = _want(x, fmt)
    with PowerStats(1) as p:
        p.process(x)
        _same(p.read(), want, "host")
        p.reset()
        _same(_feed_device(p, x, fmt, 0, 1), want, "device, by elements")
        p.reset()
        _same(_feed_device(p, x, fmt), want, "device, by vectors")


def test_a_workgroup_that_takes_several_tiles():
    """More tiles than kPstatMaxGrid in one call, for one stream and for four: every workgroup strides over several."""
    block = _noise(pc.I8, 1, T + 3, 5)[0]
    tail = _noise(pc.I8, 1, 5, 6)[0]
    one = pc.State().accumulate(block, pc.I8)
    for C_ in (1, 4):
        reps = (MAX_GRID // C_ + 2) * T // (T + 3) + 1
        n = reps * (T + 3) + 5
        assert (n + T - 1) // T > MAX_GRID // C_ + 1
        x = np.concatenate([np.tile(block, reps), tail])
        want = pc.stack([pc.scaled(one, reps).accumulate(tail, pc.I8)] * C_)
        stride = n + 1                                   # odd: the streams alternate between the load paths
        with PowerStats(C_) as p, DeviceBuffer(2 * stride * C_) as buf:
            for c in range(C_):
                buf.put(x, 2 * stride * c)
            p.process_device(None, buf.ptr, n, stride, pc.I8)
            _same(p.read(), want, C_)


# ---- the state ---------------------------------------------------------------------------------------------------
def test_any_split_into_calls_through_either_entry_point_gives_the_same_bits():
    pieces = (1, 63, T + 1, 500, 3 * T + 1, 64)
    n = sum(pieces)
    x = _noise(pc.C64, 2, n, 9)
    x[0, 5], x[1, -1] = np.nan, np.inf
    want = _want(x, pc.C64)
    with PowerStats(2) as p:
        p.process(x)
        _same(p.read(), want, "one call")
        p.reset()
        k = 0
        for i, m in enumerate(pieces):
            part = x[:, k:k + m]
            if i % 2:
                p.process(part)
            else:
                _feed_device(p, part, pc.C64, i, i % 3)
            p.process_device(None, 4096, 0)              # n_in = 0: nothing happens, the pointer is not read
            p.process(x[:, :0])
            k += m
        _same(p.read(), want, "six calls")


@pytest.mark.parametrize("fmt", (pc.I8, pc.C64))
def test_a_host_block_of_three_streams_above_the_staging_goes_in_pieces(fmt, monkeypatch):
    """max_host_samples = 3 * 7 + 2: process() cuts 20 samples per stream into library calls of 7, 7 and 6, each an offset
    into rows 20 samples apart.  The state is that of one device call over the same samples, and the contract's."""
    calls, entry = [], nat.lib.tdsa_pstat_process
    monkeypatch.setattr(nat.lib, "tdsa_pstat_process", lambda h, f, ptr, n, stride: calls.append((n, stride)) or entry(h, f, ptr, n, stride))
    x = _noise(fmt, 3, 20, 77)
    want = _want(x, fmt)
    with PowerStats(3, max_host_samples=3 * 7 + 2) as p:
        p.process(x)
        host = p.read()
        assert calls == [(7, 20), (7, 20), (6, 20)]
        _same(host, want, "host")
        p.reset()
        dev = _feed_device(p, x, fmt)
        _same(dev, want, "device")
        for a, b in ((host.records, dev.records), (host.msum, dev.msum), (host.hist, dev.hist)):
            assert np.array_equal(a, b)                        # integers all: no NaN to mind


def test_read_of_sub_ranges_reset_reconfiguration_gate_and_window():
    x = _noise(pc.C64, 5, 1000, 3)
    x[:, ::50] = 0
    with PowerStats(5) as p:
        p.process(x)
        want = _want(x, pc.C64)
        _same(p.read(), want, "all")
        for rng in (range(0, 1), range(4, 5), range(1, 4), range(0, 5)):
            got = p.read(rng)
            assert got.first_stream == rng.start and len(got) == len(rng)
            _same(got, tuple(w[rng.start:rng.stop] for w in want), rng)
        _same(p.read(2), tuple(w[2:3] for w in want), "one")
        p.process(x)                                     # the state accumulates ...
        assert np.array_equal(p.read().hist, 2 * want[2]) and np.array_equal(p.read().n_total, 2 * want[0]["n_total"])
        p.reset()                                        # ... until a reset
        _same(p.read(), _want(x[:, :0], pc.C64), "reset")
        gate = float(np.float32(np.median(np.abs(x[0]) ** 2)))
        for exp_lo, g in ((-40, gate), (-40, 0.0), (-126, 0.0), (64, gate), (64, 0.0), (-3, 0.0625)):
            p.process(x[:, :100])                        # what a reconfiguration must forget
            p.configure(exp_lo=exp_lo, gate=g)
            assert (p.exp_lo, p.gate) == (exp_lo, g)
            p.process(x)
            got = p.read()
            _same(got, _want(x, pc.C64, exp_lo, g), (exp_lo, g))
            assert (got.n_gated > 0).all() == (g > 0) and (got.n_zero > 0).all() == (g == 0)


def test_error_returns_with_a_live_handle():
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()
    buf = (C.c_byte * 4096)()
    rec = (nat.PstatRecord * 4)()
    with PowerStats(3, max_host_samples=300) as p, DeviceBuffer(4096) as d:
        h = p._h
        assert lib.tdsa_pstat_configure(h, -127, 0.0) == -1 and lib.tdsa_pstat_configure(h, -40, -1.0) == -1
        assert lib.tdsa_pstat_process(h, 5, buf, 4, 4) == -1 and "in_format" in err()
        assert lib.tdsa_pstat_process(h, pc.I8, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_pstat_process(h, pc.I8, buf, 4, 3) == -1 and "in_stride" in err()
        assert lib.tdsa_pstat_process(h, pc.I8, buf, 101, 101) == -1 and "max_host_samples" in err()
        assert lib.tdsa_pstat_process_dev(h, None, pc.C64, C.c_void_p(d.ptr + 4), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_pstat_process_dev(h, None, pc.I8, C.c_void_p(d.ptr + 1), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_pstat_process_dev(h, None, pc.C64, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_pstat_process_dev(h, None, pc.C64, C.c_void_p(d.ptr), 4, 3) == -1 and "in_stride" in err()
        for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
            assert lib.tdsa_pstat_read(h, first, count, rec, None, None) == -1 and "streams" in err()
        assert lib.tdsa_pstat_read(h, 0, 3, None, None, None) == -1 and "null records" in err()
        assert lib.tdsa_pstat_timer_end(h, None) == -1
        assert lib.tdsa_pstat_process(h, pc.I8, None, 0, 0) == 0 and lib.tdsa_pstat_process_dev(h, None, pc.I8, None, 0, 0) == 0
        assert lib.tdsa_pstat_read(h, 0, 3, rec, None, None) == 0                    # records alone
        assert [r.n_total for r in rec[:3]] == [0, 0, 0] and [r.min_bits for r in rec[:3]] == [0xFFFFFFFF] * 3
        p.timer_begin()
        p.process_device(None, d.ptr, 16, 16, pc.I8)
        assert p.timer_end() >= 0.0
    with PowerStats(1, max_host_samples=8) as p:                                    # C = 1: the stride is ignored
        assert lib.tdsa_pstat_process(p._h, pc.I8, buf, 4, 0) == 0 and int(p.read().n_total[0]) == 4
        p.process(np.zeros(2 * 30, dtype=np.int8))                                  # above the staging: in pieces
        assert int(p.read().n_total[0]) == 34 and int(p.read().n_zero[0]) == 34


# ---- counts and offsets past 2^32 --------------------------------------------------------------------------------
def test_more_than_2_to_the_32_samples_in_one_bin():
    n = 1 << 28
    with room_or_skip(2 * n) as buf, PowerStats(1) as p:
        x = np.tile(np.array([64, 0], dtype=np.int8), 1 << 20)                       # p = 0.25
        for k in range(0, 2 * n, x.nbytes):
            buf.put(x, k)
        for _ in range(17):
            p.process_device(None, buf.ptr, n, n, pc.I8)
        got = p.read()
    st = pc.scaled(pc.State().accumulate(x, pc.I8), 17 * n // (1 << 20))
    assert int(st.hist.max()) == 17 * n > 1 << 32 and int(st.msum[125]) == 17 * n << 23
    _same(got, pc.stack([st]))
    assert got.mean_power[0] == 0.25 and got.papr_db[0] == 0.0


def test_a_stream_past_2_to_the_32_bytes():
    stride, n = (1 << 29) + 1, 3 * T + 1
    x = _noise(pc.C64, 2, n, 12)
    with room_or_skip(8 * (stride + n)) as buf, PowerStats(2) as p:
        buf.put(x[0], 0)
        buf.put(x[1], 8 * stride)
        p.process_device(None, buf.ptr, n, stride, pc.C64)
        got = p.read()
    _same(got, _want(x, pc.C64))


# ---- stream order ------------------------------------------------------------------------------------------------
def test_behind_a_channelizer_and_a_down_converter_on_an_engine_stream():
    rng = np.random.default_rng(4)
    n_in, M, D = 1 << 16, 8, 4
    iq = rng.integers(-128, 128, 2 * n_in).astype(np.int8)
    with SpectrumEngine(64) as eng, Channelizer(M, 1e6) as ch, DownConverter(D, 1e6, 1e5) as ddc, \
            PowerStats(M) as pm, PowerStats(1) as p1, DeviceBuffer.of(iq) as d_in:
        n_ch, n_dd = ch.outputs_completed_by(n_in), n_in // D + 1
        stride = n_ch + 3
        with DeviceBuffer(8 * M * stride) as d_ch, DeviceBuffer(8 * n_dd) as d_dd:
            d_ch.put(np.full(M * stride, np.nan, dtype=np.complex64))
            got_ch = ch.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_ch.ptr, stride)
            pm.process_device(eng, d_ch.ptr, got_ch, stride)          # no wait in between: the stream orders them
            got_dd = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_dd.ptr)
            p1.process_device(eng, d_dd.ptr, got_dd)
            sm, s1 = pm.read(), p1.read()
            eng.synchronize()
            y_ch = d_ch.get((M, stride), np.complex64)[:, :got_ch]
            y_dd = d_dd.get((got_dd,), np.complex64)
    assert got_ch == n_ch > 1000 and got_dd > 1000
    _same(sm, _want(y_ch, pc.C64), "channelizer")
    _same(s1, _want(y_dd[None, :], pc.C64), "down-converter")
    assert (sm.n_total == got_ch).all() and int(sm.n_nan.sum()) == 0
