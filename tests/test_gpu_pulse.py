"""The pulse analysis on the device (tdsa_pulse_*) against tests/pulse_contract.py: the integer
fields of every record, the summaries and which pulses are stored under np.array_equal, whatever the shape, the format,
the entry point, the load path or the split into calls; energy within width 2^-52 energy and acc_re, acc_im within
width 2^-50 energy of the correctly rounded sums (pulse_contract.within_bounds says why)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import pulse_contract as pc
from kernel_build import CSRC
from topdogspectrumanalyser_amd import Channelizer, DeviceBuffer, DownConverter, SpectrumEngine
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd.pulses import PulseAnalyzer

pytestmark = pytest.mark.gpu


def _const(name):
    src = open(os.path.join(CSRC, "tdsa_pulse.hpp")).read()
    expr = re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)
    return int(eval(re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), expr)))


T = _const("kPulseTile")
CPT = _const("kPulseSamplesPerThread")
MAX_TILES = _const("kPulseMaxLaunchTiles")
SIZES = (1, 2, 3, CPT - 1, CPT, CPT + 1, 64 * CPT - 1, 64 * CPT, 64 * CPT + 1, T - 1, T, T + 1, 3 * T + 1)
DTYPE = {pc.I8: np.int8, pc.U8: np.uint8, pc.C64: np.complex64}
GAP = {pc.I8: np.int8(127), pc.U8: np.uint8(255), pc.C64: np.complex64(complex(3.0, 3.0))}   # class A: they would show
ON, OFF = 0.5, 0.1
DISTINCT = 8                                     # the streams of a 256-stream case repeat after this many


def _per(fmt):
    return 1 if fmt == pc.C64 else 2


def _samples(code, fmt, rng):
    """Samples of the classes `code` (pc.A / pc.B / pc.C) with the levels ON, OFF.  Bytes: |I|, |Q| in 80 .. 127 give p >=
    0.78, in 40 .. 50 p in 0.19 .. 0.31, in 0 .. 20 p <= 0.05; complex64: |x| in 0.8 .. 1.2, 0.4 .. 0.5, 0 .. 0.2."""
    n = code.size
    if fmt == pc.C64:
        lo = np.choose(code, [0.4, 0.8, 0.0])
        hi = np.choose(code, [0.5, 1.2, 0.2])
        amp = lo + (hi - lo) * rng.random(n)
        return (amp * np.exp(2j * np.pi * rng.random(n))).astype(np.complex64)
    lo = np.choose(code, [40, 80, 0]).repeat(2)
    hi = np.choose(code, [51, 128, 21]).repeat(2)
    mag = rng.integers(lo, hi)
    sign = rng.integers(0, 2, 2 * n) * 2 - 1
    if fmt == pc.I8:
        return (mag * sign).astype(np.int8)
    return np.clip(128 + mag * sign, 0, 255).astype(np.uint8)


def _random_code(n, rng):
    """Classes in runs: most short, some up to a wave's samples, a few longer than a tile."""
    out = np.empty(0, dtype=np.int64)
    while out.size < n:
        k = 256
        kind = rng.random(k)
        length = np.where(kind < 0.6, rng.integers(1, 5, k), np.where(kind < 0.93, rng.integers(5, 300, k), rng.integers(300, T + 500, k)))
        out = np.concatenate([out, np.repeat(rng.integers(0, 3, k), length)])
    return out[:n]


def _streams(fmt, C_, n, seed):
    rng = np.random.default_rng(seed)
    base = [_samples(_random_code(n, rng), fmt, rng) for _ in range(min(C_, DISTINCT))]
    return np.stack([base[c % len(base)] for c in range(C_)])


def _want(x2d, fmt, **kw):
    kw.setdefault("on_level", ON)
    kw.setdefault("off_level", OFF)
    distinct = [pc.Stream(**kw).feed(s, fmt) for s in x2d[:DISTINCT]]
    return [distinct[c % len(distinct)] for c in range(x2d.shape[0])]


def _same(p, want, tag=""):
    """The handle's state against the contract's streams."""
    sums = p.read_summaries()
    for c, w in enumerate(want):
        ws = w.summary()
        for f in pc.SUMMARY.names:
            assert sums[c][f] == ws[f], (tag, c, f, sums[c], ws)
    for c in sorted({0, 1, len(want) // 2, len(want) - 1} & set(range(len(want)))) if len(want) > 4 else range(len(want)):
        err = pc.within_bounds(p.read(c).records, want[c].records())
        assert err is None, (tag, c, err)


def _feed_device(p, x2d, fmt, extra=0, offset=0, engine=None):
    """The streams through the device entry point: `offset` samples into a 16-byte aligned buffer, in_stride = n + extra,
    the gaps (and the lead) filled with samples that would show if they were read.  Waits, so the buffer may go."""
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
        p.read_summaries()


def _analyzer(C_=1, capacity=4096, **kw):
    p = PulseAnalyzer(C_, capacity, **kw)
    p.configure(ON, OFF)
    return p


# ---- shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (1, 2, 3, 256))
@pytest.mark.parametrize("fmt", (pc.I8, pc.U8, pc.C64))
def test_every_length_stream_count_format_entry_point_and_stride(fmt, C_):
    with _analyzer(C_, max_host_samples=C_ * SIZES[-1]) as p:
        for n in SIZES:
            x = _streams(fmt, C_, n, 100 * n + C_)
            want = _want(x, fmt)
            p.reset()
            p.process(x)
            _same(p, want, ("host", n))
            for extra in (0, 1, 7):                       # an odd stride: the streams alternate between the load paths
                p.reset()
                _feed_device(p, x, fmt, extra)
                _same(p, want, ("device", n, extra))


@pytest.mark.parametrize("fmt", (pc.I8, pc.U8, pc.C64))
def test_a_base_pointer_one_and_three_samples_off_16_bytes(fmt):
    for C_ in (1, 3):
        with _analyzer(C_) as p:
            for n in (1, CPT + 1, T + 1, 3 * T + 1):
                x = _streams(fmt, C_, n, n + C_)
                want = _want(x, fmt)
                for offset, extra in ((1, 0), (1, 1), (3, 4)):
                    p.reset()
                    _feed_device(p, x, fmt, extra, offset)
                    _same(p, want, (C_, n, offset, extra))


# ---- constructed streams -----------------------------------------------------------------------------------------
def _run_code(code, fmt=pc.I8, seed=0, limits=None, **kw):
    """One stream of the classes `code` through the device entry point against the contract."""
    x = _samples(np.asarray(code), fmt, np.random.default_rng(seed))[None, :]
    want = _want(x, fmt, **kw)
    with PulseAnalyzer(1, kw.get("capacity", 4096)) as p:
        p.configure(ON, OFF, kw.get("min_width", 1))
        if limits:
            p._debug_limits(*limits)
        _feed_device(p, x, fmt)
        _same(p, want, kw)
        return p.read(0), want[0]


def test_edges_at_every_offset_around_a_thread_a_wave_and_a_tile_seam():
    """Blocks of three tiles, each with one pulse: it rises at a seam + dr and the first off sample is at a later seam +
    df, for every dr, df in -2 .. 2 and thread, wave and tile seams on either side.  C samples lead up to the rising
    edge (they must not switch on) and fill every other sample of the pulse (they must not switch off)."""
    wave = 64 * CPT
    rises, falls = (5 * CPT, wave, T), (T + 7 * CPT, T + 2 * wave, 2 * T)
    code = []
    for r, f, dr, df in itertools.product(rises, falls, range(-2, 3), range(-2, 3)):
        block = np.full(3 * T, pc.B)
        block[r + dr - 3:r + dr] = pc.C
        block[r + dr:f + df] = pc.A
        block[r + dr + 1:f + df:2] = pc.C
        code.append(block)
    got, want = _run_code(np.concatenate(code))
    assert len(got) == 225 and want.sum["n_short"] == 0
    assert np.array_equal(np.diff(got.toa) > 0, np.ones(224, dtype=bool))


def test_pulses_over_whole_tiles_and_tiles_of_nothing_but_c_samples():
    A_, B_, C_ = (np.full(T, v) for v in (pc.A, pc.B, pc.C))
    half_on = np.concatenate([np.full(T // 2, pc.B), np.full(T - T // 2, pc.A)])
    half_off = half_on[::-1]
    for k in range(4):                                   # a pulse over 0, 1, 2, 3 whole tiles between two half tiles
        got, _ = _run_code(np.concatenate([half_on] + [A_] * k + [half_off, B_]), seed=k)
        assert len(got) == 1 and got.width[0] == T - T // 2 + k * T + T // 2 and got.toa[0] == T // 2
    # a tile of C samples keeps the state that comes in: on behind an A tile, off between two B tiles
    got, _ = _run_code(np.concatenate([A_, C_, B_, B_, C_, B_, half_on, C_, C_, half_off]))
    assert got.width.tolist() == [2 * T, (T - T // 2) + 2 * T + T // 2]
    got, _ = _run_code(np.concatenate([C_, C_, A_[:5], C_, B_]))     # C samples before anything else: off after a reset
    assert got.toa.tolist() == [2 * T] and got.width.tolist() == [5 + T]


def test_all_on_all_off_and_every_other_sample_on():
    got, want = _run_code(np.full(3 * T + 1, pc.A))
    assert len(got) == 0 and got.open_pulse == (0, 3 * T + 1) and got.duty_cycle == 1.0
    got, _ = _run_code(np.full(3 * T + 1, pc.B))
    assert len(got) == 0 and got.open_pulse is None and got.n_on == 0
    code = np.tile([pc.A, pc.B], T + T // 2 + 1)[:3 * T + 1]            # the most pulses a tile can hold
    got, _ = _run_code(code, capacity=2 * T)
    assert len(got) == (3 * T) // 2 and got.open_pulse == (3 * T, 1) and (got.width == 1).all() and np.isnan(got.freq).all()
    got, _ = _run_code(code, fmt=pc.C64, capacity=2 * T)
    assert len(got) == (3 * T) // 2


def test_a_call_longer_than_one_launch():
    """A launch holds kPulseMaxLaunchTiles tiles, one workgroup each - that is the grid cap - and the launcher cuts a
    longer call.  The limit lowered so that small inputs meet it: launches of three, two and one tile cut a call of
    seven; against the contract and against the run with the limit as it is."""
    rng = np.random.default_rng(77)
    code = _random_code(6 * T + 11, rng)
    plain, _ = _run_code(code, fmt=pc.C64, seed=1)
    for limits in ((3, 7), (2, 7), (1, 7)):
        got, _ = _run_code(code, fmt=pc.C64, seed=1, limits=limits)
        for f in pc.INTEGER_FIELDS:
            assert np.array_equal(got.records[f], plain.records[f]), (limits, f)
    x = _streams(pc.I8, 3, 5 * T + 3, 5)
    want = _want(x, pc.I8)
    with _analyzer(3) as p:
        p._debug_limits(6, 7)                               # per stream: launches of two tiles
        _feed_device(p, x, pc.I8, 1)
        _same(p, want, "three streams")


def test_one_call_against_six_pieces_through_both_entry_points():
    pieces = (1, CPT - 1, T + 1, 500, 3 * T + 1, 64)
    n = sum(pieces)
    x = _streams(pc.C64, 2, n, 9)
    want = _want(x, pc.C64)
    with _analyzer(2) as p:
        p.process(x)
        _same(p, want, "one call")
        one = [p.read(c).records for c in range(2)]
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
        _same(p, want, "six calls")
        for c in range(2):
            six = p.read(c).records
            for f in pc.INTEGER_FIELDS:
                assert np.array_equal(six[f], one[c][f]), (c, f)


def _seam_train(fmt, C_, n):
    """[C][n] samples, stream c on where (k + 3 + c) % 8 < 5: with 7 samples a piece every stream has a pulse over the
    seams at 7 and at 14.  int8 pairs, or complex64 in multiples of 1 / 8: every float64 sum of a pulse is exact in any
    order, so the records have one right answer, bit for bit."""
    k = np.arange(n)
    on = (k[None, :] + 3 + np.arange(C_)[:, None]) % 8 < 5
    if fmt == pc.C64:
        return (np.where(on, 1.0 + 0.25 * (k % 4), 0.125 * (k % 2)) + 1j * np.where(on, 0.5 * (k % 3 - 1.0), 0.0)).astype(np.complex64)
    iq = np.stack([np.where(on, 80 + 7 * k % 40, 3), np.where(on, -(85 + k % 30), -2)], axis=-1)
    return iq.reshape(C_, 2 * n).astype(np.int8)


@pytest.mark.parametrize("fmt", (pc.I8, pc.C64))
def test_a_host_block_of_three_streams_above_the_staging_goes_in_pieces(fmt, monkeypatch):
    """max_host_samples = 3 * 7 + 2: process() cuts 20 samples per stream into library calls of 7, 7 and 6, each an offset
    into rows 20 samples apart; the open pulse, the last sample and the parity cross both seams in every stream.  The
    state is that of one device call over the same samples, and the contract's."""
    calls, entry = [], nat.lib.tdsa_pulse_process
    monkeypatch.setattr(nat.lib, "tdsa_pulse_process", lambda h, f, ptr, n, stride: calls.append((n, stride)) or entry(h, f, ptr, n, stride))
    x = _seam_train(fmt, 3, 20)
    want = _want(x, fmt)
    assert all(w.summary()["n_pulses"] >= 2 for w in want)

    def state(p):
        return p.read_summaries(), [p.read(c).records for c in range(3)]

    with _analyzer(3, max_host_samples=3 * 7 + 2) as p:
        p.process(x)
        host = state(p)
        assert calls == [(7, 20), (7, 20), (6, 20)]
        p.reset()
        _feed_device(p, x, fmt)
        dev = state(p)
    for tag, (sums, recs) in (("host", host), ("device", dev)):
        for c, w in enumerate(want):
            for f in pc.SUMMARY.names:
                assert np.array_equal(sums[c][f], w.summary()[f]), (tag, c, f)
            for f in pc.RECORD.names:
                assert np.array_equal(recs[c][f], w.records()[f]), (tag, c, f)


def test_overflow_min_width_across_a_tile_seam_and_non_finite_samples():
    rng = np.random.default_rng(3)
    code = _random_code(3 * T + 1, rng)
    for capacity in (1, 3):
        got, want = _run_code(code, capacity=capacity)
        assert len(got) == capacity and got.n_lost == got.n_pulses - capacity > 0
    # pulses of width w - 1, w, w + 1 that cross the seam between two tiles, and the same inside a tile
    for w in (2, 7, CPT + 2):
        block = np.full(2 * T, pc.B)
        parts = []
        for width in (w - 1, w, w + 1):
            for start in (T - 1, T - width + 1, T // 2):
                b = block.copy()
                b[start:start + width] = pc.A
                parts.append(b)
        got, want = _run_code(np.concatenate(parts), min_width=w)
        assert len(got) == 6 and got.n_short == 3 and got.width.tolist() == [w] * 3 + [w + 1] * 3
        assert got.n_on == 3 * (3 * w)                    # before the width filter
    x = _samples(code, pc.C64, rng)
    on = np.flatnonzero(code == pc.A)
    x[on[5]] = complex(np.inf, 0)                          # p = +inf: class A, the pulse's flag
    x[on[40]] = complex(np.nan, 0)                         # NaN: class B, ends a pulse
    x[on[90]] = complex(0, -np.inf)
    x[np.flatnonzero(code == pc.B)[7]] = complex(np.nan, np.nan)
    x[np.flatnonzero(code == pc.C)[9]] = complex(1e30, 1e30)    # the squares overflow: +inf
    want = _want(x[None, :], pc.C64)
    with _analyzer(1) as p:
        p.process(x)
        _same(p, want, "non-finite, host")
        got = p.read(0)
        assert got.n_nan == 2 and np.count_nonzero(got.flags & 1) >= 2 and np.isinf(got.energy[(got.flags & 1) != 0]).all()
        p.reset()
        _feed_device(p, x[None, :], pc.C64, 0, 1)
        _same(p, want, "non-finite, device")


def test_reset_reconfigure_and_the_levels_themselves():
    x = _streams(pc.C64, 2, T + 100, 21)
    with _analyzer(2) as p:
        p.process(x)
        p.process(x)                                       # the state accumulates ...
        want = [pc.Stream(ON, OFF).feed(s, pc.C64).feed(s, pc.C64) for s in x]
        _same(p, want, "twice")
        p.reset()                                          # ... until a reset
        _same(p, [pc.Stream(ON, OFF) for _ in x], "reset")
        for on, off, w in ((ON, OFF, 1), (0.04, 0.04, 1), (0.25, 0.16, 3), (1.0, 0.01, 2)):
            p.process(x[:, :100])                          # what a reconfiguration must forget
            p.configure(on, off, w)
            assert (p.on_level, p.off_level, p.min_width) == (float(np.float32(on)), float(np.float32(off)), w)
            p.process(x)
            _same(p, _want(x, pc.C64, on_level=on, off_level=off, min_width=w), (on, off, w))
    # p exactly at each level and the float32 below it: (0.5, 0)^2 = 0.25 = on, (0.25, 0)^2 = 0.0625 = off
    below = lambda v: np.nextafter(np.float32(v), np.float32(0))
    x = np.array([0.5, 0.25, below(0.25), 0.25, below(0.5), 0.5, below(0.25), 0.0], dtype=np.complex64)
    with PulseAnalyzer(1, 16) as p:
        p.configure(0.25, 0.0625)
        p.process(x)
        got = p.read(0)
        assert got.toa.tolist() == [0, 5] and got.width.tolist() == [2, 1]
        _same(p, _want(x[None, :], pc.C64, on_level=0.25, off_level=0.0625), "levels")


def test_behind_a_channelizer_and_a_down_converter_on_an_engine_stream():
    rng = np.random.default_rng(4)
    n_in, M, D = 1 << 16, 8, 4
    gate = (np.arange(n_in) % 5000 < 1500).repeat(2)
    iq = (rng.integers(-128, 128, 2 * n_in) * np.where(gate, 1.0, 0.05)).astype(np.int8)
    with SpectrumEngine(64) as eng, Channelizer(M, 1e6) as ch, DownConverter(D, 1e6, 1e5) as ddc, \
            PulseAnalyzer(M, 256) as pm, PulseAnalyzer(1, 256) as p1, DeviceBuffer.of(iq) as d_in:
        n_ch, n_dd = ch.outputs_completed_by(n_in), n_in // D + 1
        stride = n_ch + 3
        with DeviceBuffer(8 * M * stride) as d_ch, DeviceBuffer(8 * n_dd) as d_dd:
            d_ch.put(np.full(M * stride, np.nan, dtype=np.complex64))
            got_ch = ch.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_ch.ptr, stride)
            eng.synchronize()
            y_ch = d_ch.get((M, stride), np.complex64)[:, :got_ch]
            got_dd = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_dd.ptr)
            eng.synchronize()
            y_dd = d_dd.get((got_dd,), np.complex64)
            # levels from the streams themselves: between the gated and the full power
            lv_ch = float(np.float32(0.3 * np.mean(np.abs(y_ch) ** 2)))
            lv_dd = float(np.float32(0.3 * np.mean(np.abs(y_dd) ** 2)))
            pm.configure(lv_ch, lv_ch / 4, 2)
            p1.configure(lv_dd, lv_dd / 4, 2)
            d_ch.put(np.full(M * stride, np.nan, dtype=np.complex64))
            ch.reset()
            ddc.reset()
            got_ch = ch.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_ch.ptr, stride)
            pm.process_device(eng, d_ch.ptr, got_ch, stride)          # no wait in between: the stream orders them
            got_dd = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_dd.ptr)
            p1.process_device(eng, d_dd.ptr, got_dd)
            _same(pm, _want(y_ch, pc.C64, on_level=lv_ch, off_level=lv_ch / 4, min_width=2, capacity=256), "channelizer")
            _same(p1, _want(y_dd[None, :], pc.C64, on_level=lv_dd, off_level=lv_dd / 4, min_width=2, capacity=256), "down-converter")
            assert got_ch == n_ch > 1000 and got_dd > 1000 and p1.read(0).n_pulses >= 3
            eng.synchronize()


def test_error_returns_with_a_live_handle():
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()
    buf = (C.c_byte * 4096)()
    sums = (nat.PulseSummary * 4)()
    rec = (nat.PulseRecord * 4)()
    got = C.c_int(7)
    with PulseAnalyzer(3, 4, max_host_samples=300) as p, DeviceBuffer(4096) as d:
        h = p._h
        for bad in ((0.0, 0.0, 1), (-1.0, -1.0, 1), (float("inf"), 1.0, 1), (float("nan"), 1.0, 1), (1.0, 2.0, 1), (1.0, 0.0, 1),
                    (1.0, float("nan"), 1), (1.0, 1.0, 0), (1.0, 1.0, 1 << 31)):
            assert lib.tdsa_pulse_configure(h, *bad) == -1, bad
        assert lib.tdsa_pulse_process(h, 5, buf, 4, 4) == -1 and "in_format" in err()
        assert lib.tdsa_pulse_process(h, pc.I8, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_pulse_process(h, pc.I8, buf, 4, 3) == -1 and "in_stride" in err()
        assert lib.tdsa_pulse_process(h, pc.I8, buf, 101, 101) == -1 and "max_host_samples" in err()
        assert lib.tdsa_pulse_process_dev(h, None, pc.C64, C.c_void_p(d.ptr + 4), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_pulse_process_dev(h, None, pc.I8, C.c_void_p(d.ptr + 1), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_pulse_process_dev(h, None, pc.C64, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_pulse_process_dev(h, None, pc.C64, C.c_void_p(d.ptr), 4, 3) == -1 and "in_stride" in err()
        for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
            assert lib.tdsa_pulse_read(h, first, count, sums) == -1 and "streams" in err()
        assert lib.tdsa_pulse_read(h, 0, 3, None) == -1 and "null summaries" in err()
        for stream, first, count in ((-1, 0, 1), (3, 0, 1), (0, -1, 1), (0, 0, -1)):
            assert lib.tdsa_pulse_read_pulses(h, stream, first, count, rec, C.byref(got)) == -1 and got.value == 0
        assert lib.tdsa_pulse_read_pulses(h, 0, 0, 1, None, C.byref(got)) == -1 and "null records" in err()
        assert lib.tdsa_pulse_read_pulses(h, 0, 0, 1, rec, None) == -1 and "null n_out" in err()
        for bad in ((2, 7), (MAX_TILES + 1, 7), (16, 8), (16, -1)):
            assert lib.tdsa_pulse_debug_limits(h, *bad) == -1, bad
        assert lib.tdsa_pulse_timer_end(h, None) == -1
        assert lib.tdsa_pulse_process(h, pc.I8, None, 0, 0) == 0 and lib.tdsa_pulse_process_dev(h, None, pc.I8, None, 0, 0) == 0
        assert lib.tdsa_pulse_read(h, 0, 3, sums) == 0 and [s.n_total for s in sums[:3]] == [0, 0, 0]
        assert lib.tdsa_pulse_read_pulses(h, 0, 0, 4, rec, C.byref(got)) == 0 and got.value == 0       # none stored yet
        p.timer_begin()
        p.process_device(None, d.ptr, 16, 16, pc.I8)
        assert p.timer_end() >= 0.0
    with PulseAnalyzer(1, 2, max_host_samples=8) as p:                               # C = 1: the stride is ignored
        p.configure(ON, OFF)
        x = _samples(np.tile([pc.A, pc.A, pc.B], 10), pc.I8, np.random.default_rng(0))
        assert lib.tdsa_pulse_process(p._h, pc.I8, x.ctypes.data_as(C.c_void_p), 6, 0) == 0 and p.read(0).n_total == 6
        p.process(x[12:])                                                           # above the staging: in pieces
        got = p.read(0)
        assert got.n_total == 30 and got.n_pulses == 10 and got.n_lost == 8 and got.toa.tolist() == [0, 3]
        n = C.c_int(0)
        assert lib.tdsa_pulse_read_pulses(p._h, 0, 1, 5, rec, C.byref(n)) == 0 and n.value == 1 and rec[0].toa == 3
