"""Zero span on the MI355X against the numpy restatement of tests/zero_span_contract.py: the reference's recorded ticks
bit for bit, random 20 Msps histories over a wrapping 40 M sample ring (any split, device against host pushes, all four
input formats, crossings that straddle the physical wrap and a push boundary), the column detectors, the detectors'
tolerances, the tuned channel behind a DownConverter, and DataProcessor with the device path on."""
import os
import types

import numpy as np
import pytest

import zero_span_contract as zc
from topdogspectrumanalyser_amd import DataProcessor, DeviceBuffer, ZeroSpan, _native as nat
from topdogspectrumanalyser_amd.zoom import DownConverter, design_decimator

pytestmark = pytest.mark.gpu

FS = 20e6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zero_span.npz")
NAT_FMT = {"i8": nat.IN_I8, "u8": nat.IN_U8, "c64": nat.IN_C64, "f32r": nat.IN_F32R}
BYTES = {"i8": 2, "u8": 2, "c64": 8, "f32r": 4}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _check_view(zs, history, mode, level, n_display, what=""):
    """One raw view against the contract: start, triggered, length, chunk and statistics."""
    start, trig, chunk = zc.view(history, zs.capacity, n_display, mode, level)
    v = zs.view(mode=mode, level=level, n_display=n_display)
    print(f"{what} total={history.size} n_display={n_display} {mode} level={level!r}: start {v.start} / {start}, "
          f"triggered {int(v.triggered)} / {trig}, length {v.length} / {chunk.size}")
    assert v.total == history.size
    assert (v.start, int(v.triggered), v.length) == (start, trig, chunk.size)
    assert v.samples.dtype == np.float32 and _same(v.samples, chunk)
    _check_stats(v, chunk, level)
    return v


def _check_stats(v, chunk, level):
    st = zc.statistics(chunk, level)
    assert (v.n_at_or_above, v.n_rise, v.n_fall) == (st["n_at_or_above"], st["n_rise"], st["n_fall"])
    assert _same(np.float32(v.min), np.float32(st["min"])) and _same(np.float32(v.max), np.float32(st["max"]))
    if chunk.size and not np.isnan(st["mean"]):
        bound = 2.0 ** -24 * float(np.mean(np.abs(chunk.astype(np.float64))))
        print(f"   info mean {v.mean!r} against {st['mean']!r}: off by {abs(v.mean - st['mean']):.3e}, bound {bound:.3e}")
        assert abs(v.mean - st["mean"]) <= bound


# ---------------------------------------------------------------------------------------------------- golden ticks
def test_golden_ticks_bit_for_bit_from_complex64_and_from_int8():
    rate, ticks = zc.golden_ticks(GOLDEN)
    with ZeroSpan(rate) as za, ZeroSpan(rate) as zb:
        assert za.capacity == 16000
        for i, t in enumerate(ticks):
            za.push(t["block"])
            zb.push(t["raw"])
            for zs in (za, zb):
                v = zs.view(mode=t["mode"], level=t["level"], window_s=t["window"])
                assert _same(v.samples, t["shown"]), (i, t["mode"], t["level"], t["window"])
                assert v.time_s.dtype == np.float32
                assert _same(v.time_s, np.arange(len(t["shown"]), dtype=np.float32) / rate)
        assert za.view().total == sum(len(t["block"]) for t in ticks)


# ---------------------------------------------------------------------------------------------------- 20 Msps histories
def _pulse_stream(rng, n, edges, fmt):
    """(raw, history): a two-level pulse train that changes level at `edges`, a little noise on top, in one input
    format; the history is the REAL detector of it."""
    level_of = np.zeros(n, dtype=np.int8)
    state = 0
    last = 0
    for e in list(edges) + [n]:
        level_of[last:e] = state
        state ^= 1
        last = e
    noise = rng.integers(-3, 4, n).astype(np.int16)
    if fmt in ("i8", "u8"):
        lo, hi = (-40, 60) if fmt == "i8" else (90, 190)
        i = (np.where(level_of == 1, hi, lo) + noise).astype(np.int8 if fmt == "i8" else np.uint8)
        q = rng.integers(-5, 6, n).astype(np.int16)
        q = (q if fmt == "i8" else q + 128).astype(i.dtype)
        raw = np.stack([i, q], axis=1).reshape(-1)
    else:
        re = (np.where(level_of == 1, np.float32(0.47), np.float32(-0.31)) + noise.astype(np.float32) * np.float32(0.0071))
        re = re.astype(np.float32)
        if fmt == "c64":
            raw = np.empty(n, dtype=np.complex64)
            raw.real = re
            raw.imag = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
        else:
            raw = re
    re, im = zc.unpack(raw, fmt)
    return raw, zc.detect(re, im, "real")


def _cuts(rng, n, mandatory):
    """Push boundaries: pieces of 1 .. 4 M samples, with a boundary at every mandatory position."""
    cuts, pos = [], 0
    for m in sorted(mandatory) + [n]:
        while pos < m:
            size = int(rng.integers(1_000_000, 4_000_001))
            left = m - pos
            if left <= 4_000_000 and (left <= size or left - size < 1_000_000):
                size = left
            elif left - size < 1_000_000:
                size = left // 2
            pos += size
            cuts.append(pos)
    return cuts


@pytest.mark.parametrize("fmt", ["i8", "u8", "c64", "f32r"])
def test_random_histories_at_20_msps(fmt):
    rng = np.random.default_rng({"i8": 1, "u8": 2, "c64": 3, "f32r": 4}[fmt])
    cap = int(2.0 * FS)
    n = 47_000_000
    # level changes every 50 k .. 2.5 M samples; one exactly at the physical wrap (samples cap - 1 and cap), the
    # next one at least 1.5 M later; E2 is the change a push boundary of handle A is put on
    edges, pos = [], 0
    while True:
        pos += int(rng.integers(50_000, 2_500_000))
        if pos >= n - 10:
            break
        edges.append(pos)
    edges = sorted([e for e in edges if abs(e - cap) > 1_500_000] + [cap])
    e2 = next(e for e in edges if e > 18_000_000)
    raw, history = _pulse_stream(rng, n, edges, fmt)
    level = 0.1
    assert (history[cap - 1] < level) != (history[cap] < level) and (history[e2 - 1] < level) != (history[e2] < level)
    wrap_mode = "rise" if history[cap] >= level else "fall"
    e2_mode = "rise" if history[e2] >= level else "fall"
    after_e2 = e2 + 40_000                       # before the next change (they are at least 50 k apart)
    after_wrap = cap + 1_400_000
    bps = BYTES[fmt]
    step = 1 if fmt in ("c64", "f32r") else 2

    def piece(a, b):
        return raw[step * a:step * b]

    with ZeroSpan(FS) as za, ZeroSpan(FS) as zb, DeviceBuffer(n * bps) as dev:
        assert za.capacity == cap
        for a in range(0, n, 8_000_000):
            dev.put(np.ascontiguousarray(piece(a, min(n, a + 8_000_000))), a * bps)
        cuts_a = _cuts(rng, n, [e2, after_e2, after_wrap])
        cuts_b = _cuts(rng, n, [after_e2, after_wrap])
        assert e2 in cuts_a and e2 not in cuts_b
        done_b = 0
        pos = 0
        for cut in cuts_a:
            za.push(piece(pos, cut))
            pos = cut
            hist = history[:pos]
            if pos == after_e2:
                # the pair (e2 - 1, e2) straddles two pushes of A; it is the last crossing before the window
                v = _check_view(za, hist, e2_mode, level, 20_000, f"[{fmt}] push boundary")
                assert v.triggered and v.start == e2
            elif pos == after_wrap:
                # the pair (cap - 1, cap) straddles the physical wrap of the ring
                v = _check_view(za, hist, wrap_mode, level, 1_000_000, f"[{fmt}] physical wrap")
                assert v.triggered and v.start == cap
            else:
                nd = int(rng.choice([20_000, 200_000, 2_000_000, 20_000_000, 40_000_000]))
                mode = ("free_run", "rise", "fall")[int(rng.integers(0, 3))]
                _check_view(za, hist, mode, level, nd, f"[{fmt}] A")
                # a second, short window wherever the last crossing is
                _check_view(za, hist, ("rise", "fall")[int(rng.integers(0, 2))], level,
                            int(rng.integers(20_000, 60_000)), f"[{fmt}] A")
            if pos in (after_e2, after_wrap, n):
                # handle B: the same stream from device memory, split elsewhere
                for cb in [c for c in cuts_b if done_b < c <= pos]:
                    zb.push_device(None, NAT_FMT[fmt], dev.at(done_b * bps, (cb - done_b) * bps), cb - done_b)
                    done_b = cb
                assert done_b == pos
                for nd, mode in ((20_000, "rise"), (1_000_000, "fall"), (40_000_000, "rise"), (3_000_000, "free_run")):
                    va = _check_view(za, hist, mode, level, nd, f"[{fmt}] A at a meeting point")
                    vb = _check_view(zb, hist, mode, level, nd, f"[{fmt}] B (device pushes)")
                    assert _same(va.samples, vb.samples) and va.start == vb.start
        assert pos == n and n > cap + 6_000_000
        # one push longer than the ring: only its last `capacity` samples are processed
        za.reset()
        za.push(piece(1_000_000, n))
        v = za.view(mode="free_run", n_display=cap)
        assert v.total == n - 1_000_000 and _same(v.samples, history[n - cap:])
        zb.reset()
        zb.push_device(None, NAT_FMT[fmt], dev.at(1_000_000 * bps, (n - 1_000_000) * bps), n - 1_000_000)
        v = zb.view(mode="free_run", n_display=cap)
        assert v.total == n - 1_000_000 and _same(v.samples, history[n - cap:])


# ---------------------------------------------------------------------------------------------------- columns
@pytest.mark.parametrize("length,points", [
    (5000, 5000), (5000, 5005), (2 * 1024, 1024), (63 * 7, 7), (64 * 1024, 1024), (65 * 1024, 1024), (63, 1), (64, 1),
    (65, 1), (40_000, 1), (40_000 * 7 + 3, 7), (16384 * 3 + 1000, 16384), (16384, 16384), (16384 * 1030, 16384),
    (40_000 * 1024, 1024), (1, 1), (5, 7)])
def test_columns_against_numpy(length, points):
    rng = np.random.default_rng(length % 9973 + points)
    rate = 21e6                                     # capacity 42 M
    extra = int(rng.integers(0, 1000))
    e = (rng.standard_normal(length + extra, dtype=np.float32) * np.float32(0.4)).astype(np.float32)
    if length > 100:
        e[rng.integers(0, e.size, 3)] = np.nan      # a NaN stays in its cell
    level = 0.25
    with ZeroSpan(rate) as zs:
        zs.push(e)
        start, trig, chunk = zc.view(e, zs.capacity, length, "free_run", level)
        assert chunk.size == length
        P, bounds = zc.cells(length, points)
        sizes = np.diff(bounds)
        print(f"L={length} points={points}: P={P}, cells of {sizes.min()} .. {sizes.max()} samples")
        mm = zs.view(level=level, n_display=length, points=points, column="minmax")
        assert mm.columns.shape == (2, P) and (mm.start, mm.length) == (start, length)
        assert _same(mm.columns, zc.columns(chunk, points, "minmax"))
        _check_stats(mm, chunk, level)
        sm = zs.view(level=level, n_display=length, points=points, column="sample")
        assert sm.columns.shape == (P,) and _same(sm.columns, zc.columns(chunk, points, "sample"))
        _check_stats(sm, chunk, level)
        # MEAN: one float32 rounding of a float64 sum - within 2^-23 of the cell's largest |e| (NaN cells stay NaN)
        clean = np.nan_to_num(e, nan=0.5)
        zs.reset()
        zs.push(clean)
        chunk = clean[clean.size - length:]
        mean = zs.view(level=level, n_display=length, points=points, column="mean")
        want = zc.columns(chunk, points, "mean")
        peak = np.array([np.max(np.abs(chunk[bounds[c]:bounds[c + 1]])) for c in range(P)], dtype=np.float64)
        off = np.abs(mean.columns.astype(np.float64) - want)
        print(f"   MEAN: worst |error| / (2^-23 max|e|) = {np.max(off / (2.0 ** -23 * peak)):.3f}")
        assert mean.columns.dtype == np.float32 and np.all(off <= 2.0 ** -23 * peak)
        _check_stats(mean, chunk, level)


def test_columns_of_a_triggered_window_across_the_wrap():
    rng = np.random.default_rng(77)
    with ZeroSpan(8000.0) as zs:                     # capacity 16000
        e = (np.sin(np.arange(30_000) / 37.0) + 0.1 * rng.standard_normal(30_000)).astype(np.float32)
        for a in range(0, e.size, 1234):
            zs.push(e[a:a + 1234])
        for nd, points, mode in ((3000, 100, "rise"), (15_000, 2048, "fall"), (200, 200, "rise"), (7000, 3, "fall")):
            start, trig, chunk = zc.view(e, zs.capacity, nd, mode, 0.3)
            assert trig == 1
            v = zs.view(mode=mode, level=0.3, n_display=nd, points=points)
            assert (v.start, v.triggered) == (start, True) and _same(v.columns, zc.columns(chunk, points, "minmax"))
            _check_stats(v, chunk, 0.3)
            assert v.duty_cycle == v.n_at_or_above / nd and v.n_rise >= 1


# ---------------------------------------------------------------------------------------------------- detectors
def _detector_inputs():
    rng = np.random.default_rng(11)
    amp = 10.0 ** rng.uniform(-6.0, np.log10(4.0), 200_000)
    ph = rng.uniform(0, 2 * np.pi, amp.size)
    c64 = (amp * np.exp(1j * ph)).astype(np.complex64)
    c64[:4] = [1e-6, 4.0, 1e-6j, -4.0j]
    b = np.arange(256)
    pairs = np.stack(np.meshgrid(b, b, indexing="ij"), axis=-1).reshape(-1)
    return {"c64": c64, "i8": (pairs - 128).astype(np.int8), "u8": pairs.astype(np.uint8)}


@pytest.mark.parametrize("fmt", ["c64", "i8", "u8"])
def test_mag_and_db_detectors_within_their_bounds(fmt):
    raw = _detector_inputs()[fmt]
    re, im = zc.unpack(raw, fmt)
    log_floor, offset_db = 1e-12, -12.5
    with ZeroSpan(1e6, detector="mag", log_floor=log_floor, offset_db=offset_db) as zs:
        zs.push(raw[:20])
        zs.push(raw[20:])
        n = re.size
        mag = zs.view(n_display=n).samples
        want = zc.detect64(re, im, "mag")
        nz = want > 0
        rel = np.abs(mag[nz].astype(np.float64) - want[nz]) / want[nz]
        print(f"[{fmt}] MAG: worst relative error {rel.max() / 2.0 ** -23:.3f} x 2^-23 over {n} samples")
        assert mag.size == n and rel.max() <= 2.0 * 2.0 ** -23 and np.all(mag[~nz] == 0)
        assert np.array_equal(mag.view(np.uint32), zc.detect(re, im, "mag").view(np.uint32))   # section 4.10: bit for bit
        zs.set_detector("db")
        assert zs.view(n_display=n).length == 0                       # setting the detector resets the history
        zs.push(raw)
        db = zs.view(n_display=n).samples
        want = zc.detect64(re, im, "db", log_floor, offset_db)
        off = np.abs(db.astype(np.float64) - want)
        print(f"[{fmt}] DB: worst error {off.max():.3e} dB")
        assert db.size == n and off.max() <= 1e-3
        zs.set_detector("real")
        zs.push(raw)
        assert _same(zs.view(n_display=n).samples, re)


# ---------------------------------------------------------------------------------------------------- tuned channel
@pytest.mark.parametrize("D", [8, 64])
def test_tuned_channel_is_the_down_converter_then_the_detector(D):
    rng = np.random.default_rng(D)
    n = 300_000 + 17
    f = 1.234e6
    t = np.arange(n)
    gate = ((t // 5000) % 3 == 0).astype(np.float32)                  # a pulsed carrier at the offset, and noise
    x = (gate * 0.8 * np.exp(2j * np.pi * f / FS * t) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    x = x.astype(np.complex64)
    taps = design_decimator(D)
    with DownConverter(D, FS, f, taps) as ddc:
        y = ddc.process(x)
    cuts = [0, 1, 4097, 100_000, 100_003, 250_001, n]
    for det in ("real", "mag"):
        with ZeroSpan(FS, detector=det, decimation=D, offset_hz=f) as zs:
            assert zs.rate == FS / D and zs.capacity == int(2.0 * FS / D)
            got = sum(zs.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
            assert got == y.size == -(-n // D)
            v = zs.view(n_display=y.size)
            assert v.total == y.size and v.length == y.size
            if det == "real":
                assert _same(v.samples, zc.detect(y.real, y.imag, "real"))
                start, trig, chunk = zc.view(y.real, zs.capacity, 2000, "rise", 0.3)
                w = zs.view(mode="rise", level=0.3, n_display=2000)
                assert (w.start, int(w.triggered)) == (start, trig) and _same(w.samples, chunk)
            else:
                want = zc.detect64(y.real, y.imag, "mag")
                rel = np.abs(v.samples.astype(np.float64) - want) / want
                print(f"D={D} MAG: worst relative error {rel.max() / 2.0 ** -23:.3f} x 2^-23; pulse train: "
                      f"{zs.view(level=0.4, n_display=y.size).n_rise} rises")
                assert rel.max() <= 2.0 * 2.0 ** -23
        # the same from device memory, int8 in
    raw = np.clip(np.rint(np.stack([x.real, x.imag], axis=1) * 100), -128, 127).astype(np.int8).reshape(-1)
    with DownConverter(D, FS, f, taps) as ddc:
        y8 = ddc.process(raw)
    with ZeroSpan(FS, decimation=D, offset_hz=f) as zs, DeviceBuffer(raw.nbytes) as dev:
        dev.put(raw)
        assert zs.push_device(None, nat.IN_I8, dev.ptr, 123_457) + \
            zs.push_device(None, nat.IN_I8, dev.at(2 * 123_457, 2 * (n - 123_457)), n - 123_457) == y8.size
        assert _same(zs.view(n_display=y8.size).samples, y8.real.copy())


# ---------------------------------------------------------------------------------------------------- DataProcessor
class _Widget:
    def update_zero_span_data(self, t, y):
        self.t, self.y = np.array(t), np.array(y)


def _gui(rate, **kw):
    src = types.SimpleNamespace(sample_rate=rate, block=None)
    src.read_samples_only = lambda: src.block
    mw = types.SimpleNamespace(current_source=src, zero_span_widget=_Widget())
    dm = types.SimpleNamespace(zero_span_buffer=None, zero_span_time_window=0.01, zero_span_trigger_mode="free_run",
                               zero_span_trigger_level=0.0)
    return src, mw, dm, DataProcessor(mw, dm, **kw)


def test_data_processor_on_the_device_gives_the_widget_the_reference_bits(golden_dir):
    rate, ticks = zc.golden_ticks(GOLDEN)
    src, mw, dm, dp = _gui(rate, zero_span_on_device=True)
    for i, t in enumerate(ticks):
        dm.zero_span_trigger_mode, dm.zero_span_trigger_level, dm.zero_span_time_window = t["mode"], t["level"], t["window"]
        src.block = t["block"]
        dp._process_zero_span_data()
        assert _same(mw.zero_span_widget.y, t["shown"]), (i, t["mode"])
        assert _same(mw.zero_span_widget.t, np.arange(len(t["shown"]), dtype=np.float32) / rate)
    assert dm.zero_span_buffer is dp._zero_span and not isinstance(dm.zero_span_buffer, np.ndarray)
    # the older recording: stereo blocks among them
    g = np.load(os.path.join(golden_dir, "gui_feeds.npz"))
    src, mw, dm, dp = _gui(float(g["zs_rate"]), zero_span_on_device=True)
    dm.zero_span_time_window = float(g["zs_window"])
    for i, mode in enumerate(g["zs_modes"]):
        dm.zero_span_trigger_mode, dm.zero_span_trigger_level = str(mode), float(g["zs_levels"][i])
        src.block = g[f"zs_block_{i}"]
        dp._process_zero_span_data()
        assert _same(mw.zero_span_widget.y, g[f"zs_shown_{i}"]), (i, mode)


def test_none_in_the_display_managers_buffer_restarts_the_history():
    rate, ticks = zc.golden_ticks(GOLDEN)
    src_d, mw_d, dm_d, dev = _gui(rate, zero_span_on_device=True)
    src_h, mw_h, dm_h, host = _gui(rate)
    ring = None
    for i, t in enumerate(ticks[:60]):
        if i in (17, 18, 40):                       # DisplayManager._set_zero_span / _exit_zero_span
            dm_d.zero_span_buffer = dm_h.zero_span_buffer = None
        for src, dm, dp in ((src_d, dm_d, dev), (src_h, dm_h, host)):
            dm.zero_span_trigger_mode, dm.zero_span_trigger_level, dm.zero_span_time_window = t["mode"], t["level"], 0.5
            src.block = t["block"]
            dp._process_zero_span_data()
        assert _same(mw_d.zero_span_widget.y, mw_h.zero_span_widget.y), i
        if i in (17, 18, 40):
            assert len(mw_d.zero_span_widget.y) == len(t["block"])        # only this block is held
        ring = ring or dev._zero_span
        assert dev._zero_span is ring                                     # the handle is kept across resets ...
    src_d.sample_rate = 2 * rate                                          # ... and replaced when the rate changes
    src_d.block = ticks[0]["block"]
    dev._process_zero_span_data()
    assert dev._zero_span is not ring and dev._zero_span.capacity == int(4.0 * rate)
    assert _same(mw_d.zero_span_widget.y, ticks[0]["block"].real.astype(np.float32))
