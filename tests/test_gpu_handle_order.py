"""A handle's launches are totally ordered whichever stream each goes on (the ordering rule of Lane in
csrc/tdsa_capi_internal.hpp).  Each of the twelve handle types that can launch on a producer plan's stream is fed the same
input in six pieces, hopping engine A's stream -> its own -> engine B's stream -> ..., and has to return exactly what a
second handle returns that was fed the same pieces on its own stream throughout.  Every piece depends on the state the
piece before it left (filter history, ring position, hold row, a step written twice, an open pulse, a record buffer that
has just grown, a limit line that has just been replaced), so a launch that overtakes its predecessor shows.  The four
measurement handles are also held against their contracts, on inputs whose float64 sums are exact in any order.  Every
comparison is np.array_equal on arrays of the same dtype and shape; there is no tolerance."""
import math

import numpy as np
import pytest

import detect_contract as dc
import meas_contract as mc
import pstat_contract as psc
import pulse_contract as plc
from topdogspectrumanalyser_amd import (Channelizer, ChannelMeasure, Demodulator, DeviceBuffer, DownConverter, FskAnalyzer,
                                        PowerStats, PulseAnalyzer, SignalDetector, SpectrumEngine, SweepAssembler, SymbolSync,
                                        TraceHistory, ZeroSpan, _native as nat)

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


def _fields(a):
    """A structured array as a dict of its fields: NaNs compare equal field by field."""
    return {f: np.ascontiguousarray(a[f]) for f in a.dtype.names}


# ---- power statistics: 2 streams, pieces of 10 complex64 samples per stream, row stride 63 ------------------------------
def _pstat_input():
    rng = np.random.default_rng(17)
    x = np.full((2, 63), complex(np.nan, np.nan), dtype=np.complex64)       # the gap would count as NaN samples
    x[:, :10 * PIECES] = rng.normal(size=(2, 10 * PIECES)) + 1j * rng.normal(size=(2, 10 * PIECES))
    return x


def _pstat_run(streams):
    with PowerStats(2, max_host_samples=64) as p, DeviceBuffer.of(_pstat_input()) as d:
        assert d.ptr % 16 == 0                                 # the stride is odd: stream 1 starts 8 bytes off 16
        for i, eng in enumerate(streams):
            p.process_device(eng, d.at(8 * 10 * i, 8 * (63 + 10)), 10, 63)
        s = p.read()             # waits on the handle's own stream, which it first puts behind the last launch
        return dict(records=_fields(s.records), msum=s.msum, hist=s.hist)


def test_power_statistics_hopping_streams(engines):
    got, one = _pstat_run(_hopping(engines)), _pstat_run(SINGLE)
    rec, msum, hist = psc.run(list(_pstat_input()[:, :10 * PIECES]), psc.C64)
    assert list(got["records"]["n_total"]) == [10 * PIECES] * 2 and not got["records"]["n_nan"].any()
    assert _same(got, one)
    assert _same(got, dict(records=_fields(rec), msum=msum, hist=hist))


# ---- pulse analysis: 2 streams, capacity 8, pieces of 24 samples, on for 9 of every 16 ----------------------------------
PULSE_ON, PULSE_OFF = 0.5, 0.1


def pulse_train(n, phase):
    """complex64 [n]: on (power >= 1) where (k + phase) % 16 < 9, else off (power <= 1 / 64).  Every value is a small
    multiple of 1 / 8, so every product and every float64 sum of a pulse is exact in any order."""
    k = np.arange(n)
    on = (k + phase) % 16 < 9
    re = np.where(on, 1.0 + 0.25 * (k % 4), 0.125 * (k % 2))
    im = np.where(on, 0.5 * (k % 3 - 1.0), 0.0)
    return (re + 1j * im).astype(np.complex64)


def _pulse_input():
    # phase 0: pulses over the seams at 24, 72 and 120; phase 5: over those at 48 and 96, and on from the first sample
    return np.stack([pulse_train(24 * PIECES, 0), pulse_train(24 * PIECES, 5)])


def _pulse_run(streams):
    with PulseAnalyzer(2, 8, max_host_samples=64) as p, DeviceBuffer.of(_pulse_input()) as d:
        p.configure(PULSE_ON, PULSE_OFF)
        for i, eng in enumerate(streams):
            p.process_device(eng, d.at(8 * 24 * i, 8 * (24 * PIECES + 24)), 24, 24 * PIECES)
        out = dict(summaries=_fields(p.read_summaries()))   # waits on the handle's own stream, behind the last launch
        for c in range(2):
            out[f"records{c}"] = _fields(p.read(c).records)
        return out


def test_pulse_analyzer_hopping_streams(engines):
    got, one = _pulse_run(_hopping(engines)), _pulse_run(SINGLE)
    want = plc.run(list(_pulse_input()), plc.C64, PULSE_ON, PULSE_OFF, capacity=8)
    assert list(got["summaries"]["n_pulses"]) == [9, 9] and list(got["summaries"]["n_lost"]) == [1, 1]
    assert list(got["summaries"]["open"]) == [0, 1]
    assert _same(got, one)
    assert _same(got["summaries"], _fields(np.stack([w.summary() for w in want])))
    for c in range(2):
        assert _same(got[f"records{c}"], _fields(want[c].records()))


# ---- signal detection: 64 bins, 4 signal records per row, pieces of 1, 3, 2, 7, 1, 5 rows -------------------------------
ROW_PIECES = (1, 3, 2, 7, 1, 5)                                # the record buffers grow at the first, second and fourth
ROW_STARTS = np.concatenate([[0], np.cumsum(ROW_PIECES)])


def _detect_input():
    """Noise around -100 dB under plateaus of exactly 0 dB: with no gap bridged every bin of a run has power 1, and power
    and moment are sums of integers.  Row 4 has five runs for its four records, row 9 a NaN floor."""
    rng = np.random.default_rng(18)
    rows = (-100.0 + rng.standard_normal((int(ROW_STARTS[-1]), 64))).astype(np.float32)
    for r in range(rows.shape[0]):
        for a in rng.choice(np.arange(0, 60, 6), int(rng.integers(0, 4)), replace=False):
            rows[r, a:a + int(rng.integers(1, 6))] = 0.0
    rows[4, 2::12] = 0.0
    rows[9, 10:50] = np.nan
    return rows


def _detect_run(streams):
    rows = _detect_input()
    with SignalDetector(64, margin_db=10.0, max_signals=4, max_host_rows=8) as d, DeviceBuffer.of(rows) as buf:
        got = [d.process_device(eng, buf.at(4 * 64 * int(a), 4 * 64 * n), n) for eng, a, n in zip(streams, ROW_STARTS, ROW_PIECES)]
        out = dict(rows=_fields(np.concatenate([g.rows for g in got])), signals=_fields(np.concatenate([g.signals for g in got])))
        out["occupancy"], out["seen"], out["flagged"] = d.occupancy()
        return out, dict(lo=d.bins[0], hi=d.bins[1], rank=d.rank, margin_db=d.margin_db, min_width=d.min_width,
                         max_gap=d.max_gap, xdb=d.xdb, S=d.max_signals)


def test_signal_detector_hopping_streams(engines):
    (got, params), (one, _) = _detect_run(_hopping(engines)), _detect_run(SINGLE)
    rr, sig, occ, seen, flagged = dc.detect(_detect_input(), **params)
    assert got["rows"]["n_found"][4] > 4 and got["rows"]["flags"][9] == dc.FLAG_NAN_FLOOR and got["flagged"] == 1
    assert _same(got, one)
    assert _same(got, dict(rows=_fields(rr), signals=_fields(sig), occupancy=occ, seen=seen, flagged=flagged))


# ---- symbol recovery and FSK analysis: 4 samples per symbol, segments of 64 samples, pieces as the detector's rows ---------
SEG_LEN = 64


def _seg_input():
    rng = np.random.default_rng(20)
    n = SEG_LEN * int(ROW_STARTS[-1])
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)


def _seg_run(make, units, calls):
    """The calls (engine, first segment, segments) of the handle make() gives, outputs of units[0] and second outputs of
    units[1] bytes K to a segment back to back: both as bytes, and the records of every call."""
    total = int(ROW_STARTS[-1])
    with make() as h, DeviceBuffer.of(_seg_input()) as d_x:
        K = h.symbols_per_segment(SEG_LEN)
        with DeviceBuffer(units[0] * K * total) as d_o, DeviceBuffer(units[1] * K * total) as d_a:
            rec = [h.process_device(eng, d_x.at(8 * SEG_LEN * a, 8 * SEG_LEN * n), SEG_LEN, SEG_LEN, n,
                                    d_o.at(units[0] * K * a, units[0] * K * n), K,
                                    d_a.at(units[1] * K * a, units[1] * K * n)).records for eng, a, n in calls]
            return dict(K=K, out=d_o.get(d_o.size, np.uint8), aux=d_a.get(d_a.size, np.uint8), records=_fields(np.concatenate(rec)))


def _seg_pieces(streams):
    return [(eng, int(a), n) for eng, a, n in zip(streams, ROW_STARTS, ROW_PIECES)]


@pytest.mark.parametrize("make,units,K", [(lambda: SymbolSync(4, "qpsk", max_host_samples=64), (8, 8), 14),
                                          (lambda: FskAnalyzer(4, 2, max_host_samples=64), (4, 1), 13)],
                         ids=["symbol_sync", "fsk_analyzer"])
def test_segment_analysers_hopping_streams(engines, make, units, K):
    got, one = _seg_run(make, units, _seg_pieces(_hopping(engines))), _seg_run(make, units, _seg_pieces(SINGLE))
    whole = _seg_run(make, units, [(None, 0, int(ROW_STARTS[-1]))])
    assert got["K"] == K and got["records"]["p"].size == ROW_STARTS[-1] and not (got["records"]["flags"] & 1).any()
    assert got["out"].any() and got["aux"].any()
    assert _same(got, one)
    assert _same(got, whole)


# ---- channel measurements: as the detector, 2 channels, the limit line replaced after the third piece -------------------
MEAS_CHANNELS = [(0, 31), (32, 63)]


def _meas_input():
    """Every bin 0 dB, -inf or NaN and the number of 0 dB bins of a row a multiple of 4: every power sum is an integer, and
    at fraction 0.5 both targets of the occupied bandwidth are."""
    rng = np.random.default_rng(19)
    rows = rng.choice(np.array([0.0, 0.0, -np.inf, np.nan], dtype=np.float32), (int(ROW_STARTS[-1]), 64))
    rows[:, 5] = 0.0                                           # channel 0 has a peak: the relative line hangs on it
    for row in rows:
        ones = np.flatnonzero(row == 0.0)
        row[ones[ones != 5][:ones.size % 4]] = -np.inf
    return rows


def _meas_limits():
    first = np.full(64, np.nan, dtype=np.float32)
    first[:32] = np.where(np.arange(32) % 5 == 0, 10.0, -10.0)
    second = np.full(64, 10.0, dtype=np.float32)
    second[40:42] = -10.0
    return (first, False), (second, True)


def _meas_run(streams):
    rows, (first, second) = _meas_input(), _meas_limits()
    with ChannelMeasure(64, MEAS_CHANNELS, fraction=0.5, xdb=0.0, limit=first[0], limit_relative=first[1],
                        max_host_rows=8) as m, DeviceBuffer.of(rows) as buf:
        got = []
        for i, (eng, a, n) in enumerate(zip(streams, ROW_STARTS, ROW_PIECES)):
            if i == 3:
                m.set_limit(*second)     # on the handle's own stream, behind the piece that went on engine B's
            got.append(m.process_device(eng, buf.at(4 * 64 * int(a), 4 * 64 * n), n))
        out = dict(rows=_fields(np.concatenate([g.rows for g in got])), channels=_fields(np.concatenate([g.channels for g in got])))
        out["seen"], out["failed"] = m.totals()
        return out


def test_channel_measure_hopping_streams(engines):
    got, one = _meas_run(_hopping(engines)), _meas_run(SINGLE)
    rows, limits, cut = _meas_input(), _meas_limits(), int(ROW_STARTS[3])
    want = [mc.measure(part, MEAS_CHANNELS, (0, 63), 0.5, 0.0, lim, rel)
            for part, (lim, rel) in zip((rows[:cut], rows[cut:]), limits)]
    rr, ch = (np.concatenate([w[k] for w in want]) for k in (0, 1))
    failed = int(np.count_nonzero(rr["flags"] & mc.FLAG_MASK_FAIL))
    assert 0 < np.count_nonzero(rr["flags"][:cut] & mc.FLAG_MASK_FAIL) and 0 < failed < rows.shape[0]
    assert _same(got, one)
    assert _same(got, dict(rows=_fields(rr), channels=_fields(ch), seen=rows.shape[0], failed=failed))
