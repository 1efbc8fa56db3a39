"""A handle's launches are totally ordered whichever stream each goes on (the ordering rule of Lane in
csrc/tdsa_capi_internal.hpp).  Each of the six handle types that can launch on a producer plan's stream is fed the same
input in six pieces, hopping engine A's stream -> its own -> engine B's stream -> ..., and has to return exactly what a
second handle returns that was fed the same pieces on its own stream throughout.  Every piece depends on the state the
piece before it left (filter history, ring position, hold row, a step written twice), so a launch that overtakes its
predecessor shows.  Every comparison is np.array_equal on arrays of the same dtype and shape; there is no tolerance."""
import math

import numpy as np
import pytest

from topdogspectrumanalyser_amd import (Channelizer, Demodulator, DeviceBuffer, DownConverter, SpectrumEngine,
                                        SweepAssembler, TraceHistory, ZeroSpan, _native as nat)

pytestmark = pytest.mark.gpu

PIECES = 6


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def engines():
    with SpectrumEngine(64) as a, SpectrumEngine(64) as b:
        yield a, b


def _hopping(engines):
    a, b = engines
    return [(a, None, b)[i % 3] for i in range(PIECES)]


SINGLE = [None] * PIECES


# ---- down-converter: D = 3, 7 taps, pieces of 10 complex64 samples ---------------------------------------------------
def _ddc_run(streams):
    rng = np.random.default_rng(11)
    x = (rng.normal(size=10 * PIECES) + 1j * rng.normal(size=10 * PIECES)).astype(np.complex64)
    taps = np.array([0.05, 0.12, 0.2, 0.26, 0.2, 0.12, 0.05], dtype=np.float32)
    with DownConverter(3, 48000.0, 5000.0, taps=taps, max_host_samples=64) as ddc, DeviceBuffer.of(x) as d_in, \
            DeviceBuffer(8 * (x.size // 3 + 1)) as d_out:
        got = 0
        for i, eng in enumerate(streams):
            got += ddc.process_device(eng, nat.IN_C64, d_in.at(8 * 10 * i, 8 * 10), 10, d_out.at(8 * got))
        ddc.reset()              # waits on the handle's own stream, which it first puts behind the last launch
        return got, d_out.get(got, np.complex64).view(np.uint64)


def test_down_converter_hopping_streams(engines):
    n, y = _ddc_run(_hopping(engines))
    n1, y1 = _ddc_run(SINGLE)
    assert n == n1 == 10 * PIECES // 3
    assert _same(y, y1)


# ---- channelizer: M = 4, oversample 2 (D = 2), 9 taps (3 per branch), pieces of 7 complex64 samples -------------------
def _chan_run(streams):
    rng = np.random.default_rng(15)
    x = (rng.normal(size=7 * PIECES) + 1j * rng.normal(size=7 * PIECES)).astype(np.complex64)
    taps = np.array([0.02, 0.06, 0.12, 0.19, 0.22, 0.19, 0.12, 0.06, 0.02], dtype=np.float32)
    total = 7 * PIECES // 2                                    # 21 outputs per channel: the row stride
    with Channelizer(4, 48000.0, oversample=2, taps=taps, max_host_samples=64) as bank, DeviceBuffer.of(x) as d_in, \
            DeviceBuffer(8 * 4 * total) as d_out:
        counts = []
        for i, eng in enumerate(streams):
            counts.append(bank.process_device(eng, nat.IN_C64, d_in.at(8 * 7 * i, 8 * 7), 7,
                                              d_out.at(8 * sum(counts)), total))
        bank.reset()             # waits on the handle's own stream, which it first puts behind the last launch
        return counts, d_out.get(4 * total, np.complex64).view(np.uint64)


def test_channelizer_hopping_streams(engines):
    n, y = _chan_run(_hopping(engines))
    n1, y1 = _chan_run(SINGLE)
    assert n == n1 == [4, 3] * (PIECES // 2)
    assert _same(y, y1)


# ---- demodulator: FM, 2 channels, R = 3, 7 taps, low-pass pole c = 0.5, pieces of 10 samples per channel --------------
def _demod_run(streams):
    rng = np.random.default_rng(16)
    x = (rng.normal(size=(2, 10 * PIECES)) + 1j * rng.normal(size=(2, 10 * PIECES))).astype(np.complex64)
    taps = np.array([0.05, 0.12, 0.2, 0.26, 0.2, 0.12, 0.05], dtype=np.float32)
    total = 10 * PIECES // 3                                   # 20 outputs per channel: the row stride
    with Demodulator("fm", 48000.0, decimation=3, channels=2, taps=taps, max_host_samples=64) as dem, DeviceBuffer.of(x) as d_in, \
            DeviceBuffer(4 * 2 * total) as d_out:
        dem.set_pole(nat.DEMOD_POLE_LOWPASS, 0.5)              # its block of 64 outputs is never completed
        counts = []
        for i, eng in enumerate(streams):
            counts.append(dem.process_device(eng, d_in.at(8 * 10 * i, 8 * (10 * PIECES + 10)), 10, 10 * PIECES,
                                             d_out.at(4 * sum(counts)), total))
        m = dem.measure()        # waits on the handle's own stream, which it first puts behind the last launch
        return counts, d_out.get(2 * total, np.float32).view(np.uint32), (m.count, m.max, m.min, m.sum, m.sumsq)


def test_demodulator_hopping_streams(engines):
    n, y, m = _demod_run(_hopping(engines))
    n1, y1, m1 = _demod_run(SINGLE)
    assert n == n1 == [4, 3, 3] * (PIECES // 3)
    assert list(m[0]) == [10 * PIECES // 3] * 2
    assert _same(y, y1)
    assert _same(m, m1)


# ---- sweep assembler: 4 steps of nfft 64, one step per piece (steps 0 and 1 are written twice) -----------------------
SW_N, SW_S, SW_F, SW_K0, SW_K1 = 64, 4, 2, 8, 56


def _sweep_run(streams, timer=False):
    rng = np.random.default_rng(12)
    rows = rng.normal(-80.0, 12.0, size=(PIECES, SW_F, SW_N)).astype(np.float32)
    bin_hz = 1000.0
    centres = 100e6 + np.arange(SW_S) * (SW_K1 - SW_K0) * bin_hz
    grid = np.linspace(centres[0] - 40e3, centres[-1] + 40e3, 97)
    with SweepAssembler(SW_N, centres, (SW_K0, SW_K1), bin_hz, grid) as asm, DeviceBuffer.of(rows) as d:
        if timer:
            asm.timer_begin()
        for i, eng in enumerate(streams):
            asm.update_device(eng, i % SW_S, 1, d.at(4 * i * SW_F * SW_N, 4 * SW_F * SW_N), SW_F, "max")
        ms = asm.timer_end() if timer else None
        T, present = asm.steps()
        return dict(T=T, present=present, interp=asm.read("interp"), peak=asm.read("peak")), ms


@pytest.fixture(scope="module")
def sweep_single():
    return _sweep_run(SINGLE)[0]


def test_sweep_assembler_hopping_streams(engines, sweep_single):
    got, _ = _sweep_run(_hopping(engines))
    assert got["present"].all()
    assert _same(got, sweep_single)


def test_sweep_timer_around_updates_on_an_engine_stream(engines, sweep_single):
    """timer_end puts the assembler's stream behind updates that went on a plan's stream before it records."""
    got, ms = _sweep_run([engines[0]] * PIECES, timer=True)
    assert math.isfinite(ms) and ms >= 0.0
    assert _same(got, sweep_single)


# ---- zero span: capacity 64, pieces of 24 samples (the ring wraps inside the third piece) ----------------------------
def _zspan_run(streams):
    rng = np.random.default_rng(13)
    x = (rng.normal(size=24 * PIECES) + 1j * rng.normal(size=24 * PIECES)).astype(np.complex64)
    with ZeroSpan(64.0, detector="mag", buffer_s=1.0, max_host_samples=64) as zs, DeviceBuffer.of(x) as d:
        assert zs.capacity == 64
        for i, eng in enumerate(streams):
            assert zs.push_device(eng, nat.IN_C64, d.at(8 * 24 * i, 8 * 24), 24) == 24
        out = {}
        for name, v in (("free", zs.view("free_run", n_display=64)), ("rise", zs.view("rise", level=1.0, n_display=8))):
            out[name] = dict(samples=v.samples, start=v.start, total=v.total, length=v.length, triggered=v.triggered,
                             min=v.min, max=v.max, mean=v.mean, n_at_or_above=v.n_at_or_above, n_rise=v.n_rise,
                             n_fall=v.n_fall)
        return out


def test_zero_span_hopping_streams(engines):
    got, one = _zspan_run(_hopping(engines)), _zspan_run(SINGLE)
    assert got["free"]["total"] == 24 * PIECES and got["free"]["length"] == 64
    assert _same(got, one)


# ---- history: depth 4, 16 bins, pieces of 3 rows ---------------------------------------------------------------------
def _history_run(streams):
    rng = np.random.default_rng(14)
    rows = rng.normal(-60.0, 20.0, size=(3 * PIECES, 16)).astype(np.float32)
    with TraceHistory(4, 16) as h, DeviceBuffer.of(rows) as d:
        for i, eng in enumerate(streams):
            h.push_rows(eng, d.at(4 * 3 * 16 * i, 4 * 3 * 16), 3)
        return h.lines()


def test_history_hopping_streams(engines):
    got, one = _history_run(_hopping(engines)), _history_run(SINGLE)
    assert got["pushed"] == 3 * PIECES and got["valid"] == 4
    assert _same(got, one)
