"""The channel measurements on the device (tdsa_meas_*) against tests/meas_contract.py.

Exact under np.array_equal: every peak, x-dB and mask field, n_nan, flags, the padding, and the channels' peak_db /
peak_bin / n_nan.  Channel power: within POWER_RTOL of the contract (exp10f on the device against float32 10 ** x in
numpy), bit-equal to tdsa_detect's power for the detector's own [start, stop], and within 2 width 2^-53 of
tdsa_rows_stats on NaN-free ranges.  Occupied bandwidth on general rows: in the power domain - the contract's
piecewise-linear cumulative power C at the device's position is within 2 POWER_RTOL T of the target, the position lies in
its bin, and the bin brackets the target.  obw_total within 1e-12 T needs the contract's T formed from the device's own
p_i: exp10f and numpy's float32 power differ by 1e-7 per bin, so T is summed in numpy from the p_i the device returns
for channels of one bin (the same float64 terms, in sequence instead of the device's tree: n 2^-53 at the very most).
On rows whose p_i are 1 or 0 every sum is exact and k, x and obw_total are bit-equal to the contract.  A row's records
are bit-equal across n_rows, its place, the entry point and the load path."""
import ctypes as C

import numpy as np
import pytest

import meas_contract as mc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import detect as dt
from topdogspectrumanalyser_amd import measure as ms

pytestmark = pytest.mark.gpu

N_BINS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16383, 16384)
SEAMS = (64, 256, 1024)
EXACT_ROW = ("xdb_lo", "xdb_hi", "peak_bin", "n_nan", "n_fail", "worst_bin", "first_fail", "last_fail", "flags", "reserved")
FRACTIONS = (0.5, 0.9, 0.99, 0.999)
f32 = np.float32


def _on_device(m, rows, offset_floats=0, engine=None):
    """The rows through the device entry point, `offset_floats` floats into a 16-byte aligned buffer."""
    rows = np.ascontiguousarray(rows, dtype=f32)
    with DeviceBuffer(rows.nbytes + 4 * offset_floats + 16) as buf:
        assert buf.ptr % 16 == 0
        buf.put(rows, 4 * offset_floats)
        return m.process_device(engine, buf.at(4 * offset_floats, rows.nbytes), rows.shape[0])


def _want(m, rows, p=None):
    return mc.measure(rows, m.channels, m.obw, m.fraction, m.xdb, m.limit, m.limit_relative, p)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same(got, rr, ch, tag=""):
    """What is exact, and the channel powers."""
    for f in EXACT_ROW:
        assert np.array_equal(got.rows[f], rr[f]), (tag, f, got.rows[f][:8], rr[f][:8])
    for f in ("peak_db", "worst_margin"):
        assert np.array_equal(got.rows[f], rr[f], equal_nan=True), (tag, f)
    for f in ("peak_bin", "n_nan", "reserved"):
        assert np.array_equal(got.channels[f], ch[f]), (tag, f)
    assert np.array_equal(got.channels["peak_db"], ch["peak_db"], equal_nan=True), tag
    assert np.allclose(got.channels["power"], ch["power"], rtol=mc.POWER_RTOL, atol=0), tag


def _obw(got, rows, m, tag="", p=None, total_rtol=mc.POWER_RTOL):
    """The occupied bandwidth in the power domain, against the contract's sums of the range (of the powers p, if given)."""
    lo, hi = m.obw
    f = m.fraction
    for r, row in enumerate(np.atleast_2d(rows)):
        pw = mc.powers(row, None if p is None else p[r])[lo:hi + 1]
        with np.errstate(all="ignore"):
            S = np.cumsum(pw)
        T = S[-1]
        if not T > 0 or np.isinf(T):
            assert got.k_lo[r] == got.k_hi[r] == -1 and np.isnan(got.x_lo[r]) and np.isnan(got.x_hi[r]), (tag, r)
            assert got.flags[r] & (ms.FLAG_EMPTY | ms.FLAG_INF) == (ms.FLAG_INF if T > 0 else ms.FLAG_EMPTY), (tag, r)
            continue
        tol = 2 * mc.POWER_RTOL * T
        print(f"{tag} row {r}: T {T!r} device {got.obw_total[r]!r} rel {abs(got.obw_total[r] - T) / T:.3e}")
        assert abs(got.obw_total[r] - T) <= total_rtol * T, (tag, r)
        for x, k, t in ((got.x_lo[r], int(got.k_lo[r]), T * (1.0 - f) / 2.0), (got.x_hi[r], int(got.k_hi[r]), T * (1.0 + f) / 2.0)):
            assert lo <= k <= hi and k - 0.5 <= x <= k + 0.5, (tag, r, k, x)
            assert abs(mc.cumulative(S, lo, x) - t) <= tol, (tag, r, k, x, mc.cumulative(S, lo, x), t, tol)
            below = S[k - lo - 1] if k > lo else 0.0
            assert below - tol < t <= S[k - lo] + tol, (tag, r, k, below, t, S[k - lo])
        assert got.k_lo[r] <= got.k_hi[r] and got.x_lo[r] <= got.x_hi[r], (tag, r)


def _check(m, rows, tag="", offset_floats=0, host=False, want=None):
    rows = np.atleast_2d(np.asarray(rows, dtype=f32))
    got = m.process(rows) if host else _on_device(m, rows, offset_floats)
    rr, ch = want if want is not None else _want(m, rows)
    _same(got, rr, ch, tag)
    _obw(got, rows, m, tag)
    return got


def _device_powers(rows):
    """p_i as the device forms them, [n_rows][n] float64: the power of channels of one bin, sixteen bins a call (0 for a
    NaN bin)."""
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=f32)
    n_rows, n = rows.shape
    p = np.zeros((n_rows, n), dtype=np.float64)
    with ms.ChannelMeasure(n, [(0, 0)]) as m, DeviceBuffer.of(rows) as buf:
        for a in range(0, n, 16):
            bins = list(range(a, min(a + 16, n)))
            m.configure(channels=[(b, b) for b in bins])
            p[:, bins] = m.process_device(None, buf.ptr, n_rows).channels["power"]
    return p


def _mixed_rows(n_rows, n, seed):
    """Rows with everything at once: noise (every other row on a 0.25 dB grid, so values tie), emissions with flat tops,
    single-bin spikes, NaNs and infinities; then a constant row, an all-NaN row, a mostly-NaN row, an alternating row and
    an all -inf row where the count allows."""
    rng = np.random.default_rng(seed)
    rows = (-100.0 + 2.0 * rng.standard_normal((n_rows, n))).astype(f32)
    rows[1::2] = np.round(rows[1::2] * 4) / 4
    for r in range(n_rows):
        for _ in range(int(rng.integers(0, 6))):
            a = int(rng.integers(0, n))
            w = int(rng.integers(1, max(2, min(n, 90))))
            top = f32(-60.0 + 5.0 * rng.integers(0, 4))
            shape = np.minimum(0.0, -0.5 * (np.abs(np.arange(w) - w / 2) - w / 6)).astype(f32)
            rows[r, a:a + w] = (top + shape)[:n - a]
        rows[r, rng.integers(0, n, max(1, n // 100))] = f32(-50.0)
        if r % 3 == 0:
            rows[r, rng.integers(0, n, max(1, n // 150))] = np.nan
        if r % 7 == 3:
            rows[r, rng.integers(0, n)] = np.inf
            rows[r, rng.integers(0, n)] = -np.inf
        if r % 7 == 5:
            rows[r, rng.integers(0, n)] = -np.inf
    if n_rows >= 9:
        rows[4] = f32(-97.5)
        rows[5] = np.nan
        rows[6, rng.random(n) < 0.7] = np.nan
        rows[7] = np.where(np.arange(n) % 2 == 0, f32(-100.0), f32(-40.0))
        rows[8] = -np.inf
    return rows


def _ranges(n):
    """The whole row; lo and hi at odd places; a single bin."""
    out = [(0, n - 1)]
    if n >= 8:
        lo, hi = (n // 3) | 1, min(n - 2, (2 * n // 3) | 1)
        out.append((lo, max(lo, hi)))
    out.append((n // 2, n // 2))
    return out


def _channels(n, seed):
    """Up to 16 channels: the whole row, its ends, single bins, overlapping ranges, ranges over the seams."""
    rng = np.random.default_rng(seed)
    ch = [(n // 3, min(n - 1, n // 3 + n // 4)), (0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n // 2)]
    for s in SEAMS + (4096,):
        if s + 1 < n:
            ch.append((s - 1, s + 1))
            ch.append((int(rng.integers(0, s)), int(rng.integers(s, n))))
    while len(ch) < ms.MAX_CHANNELS:
        a = int(rng.integers(0, n))
        ch.append((a, int(rng.integers(a, n))))
    return ch[:ms.MAX_CHANNELS]


def _limit(n, seed):
    """A line through the noise's upper tail, so that some bins fail, with untested stretches."""
    rng = np.random.default_rng(seed)
    line = (-96.0 + np.round(rng.standard_normal(n) * 4) / 4).astype(f32)
    line[rng.random(n) < 0.1] = np.nan
    return line


# ---- every shape, both load paths, every range --------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_BINS)
def test_every_shape_against_the_contract(n):
    """Mixed rows per n_bins, 257 of them in the first configuration and 24 in the others; n_rows = 1, 2, 3 are the
    first rows (and must repeat their bits), the buffer is 16-byte aligned and one float off, and the totals are the
    sum of every call's."""
    all_rows = _mixed_rows(257, n, 2000 + n)
    line = _limit(n, n)
    configs = [dict(fraction=0.99, xdb=26.0), dict(fraction=0.5, xdb=0.0), dict(fraction=0.999, xdb=1000.0),
               dict(fraction=0.9, xdb=3.0)]
    first = True
    with ms.ChannelMeasure(n, [(0, 0)], max_host_rows=257) as m:
        seen = failed = 0
        for ci, cfg in enumerate(configs):
            obw = _ranges(n)[ci % len(_ranges(n))]
            rows = all_rows if first else all_rows[:24]
            m.configure(channels=_channels(n, 10 * n + ci)[:(16, 5, 1, 16)[ci]], obw=obw, **cfg)
            if ci == 0:
                m.set_limit(line)
            elif ci == 1:
                m.set_limit(line + f32(46.0), relative=True)          # channel 0's peak is near -50
            elif ci == 2:
                m.set_limit(None)
            else:
                m.set_limit(np.full(n, np.nan, dtype=f32))
            tag = f"n={n} cfg={ci} obw={obw}"
            want = _want(m, rows)
            full = _check(m, rows, tag, want=want)
            seen, failed = seen + len(rows), failed + int(np.count_nonzero(want[0]["flags"] & mc.FLAG_MASK_FAIL))
            for k, off in ((1, 1), (2, 0), (3, 1)):
                part = _check(m, rows[:k], tag + f" n_rows={k}", offset_floats=off)
                assert _bits(part.rows, full.rows[:k]) and _bits(part.channels, full.channels[:k]), tag
                seen, failed = seen + k, failed + int(np.count_nonzero(part.flags & ms.FLAG_MASK_FAIL))
            off1 = _on_device(m, rows, 1)
            host = m.process(rows)
            assert _bits(off1.rows, full.rows) and _bits(off1.channels, full.channels), tag
            assert _bits(host.rows, full.rows) and _bits(host.channels, full.channels), tag
            seen, failed = seen + 2 * len(rows), failed + 2 * int(np.count_nonzero(full.flags & ms.FLAG_MASK_FAIL))
            assert m.totals() == (seen, failed), tag
            if ci < 2 and n >= 64:
                assert full.n_fail.any(), tag
            first = False


# ---- ranges on the seams ------------------------------------------------------------------------------------------------
def _seam_ranges():
    out = []
    for s in SEAMS:
        for a in range(s - 2, s + 2):
            for b in range(a, s + 3):
                out.append((a, b))
    return out


@pytest.mark.parametrize("offset", (0, 1))
def test_ranges_start_and_stop_on_every_bin_next_to_a_seam(offset):
    """Every (lo, hi) around the seams of the 64-bin ownership, the 256-bin strides and the 1024-bin strides of the
    16-byte loads, as a channel and as the range of the occupied bandwidth and the x-dB width; ranges of one bin are
    among them."""
    n = 2100
    rows = _mixed_rows(12, n, 5)
    rng = np.random.default_rng(8)
    ranges = _seam_ranges() + [(0, 0), (n - 1, n - 1), (0, 63), (1, 64), (63, 63), (64, 64), (2047, 2099), (2048, 2048)]
    assert sum(a == b for a, b in ranges) >= 14
    with ms.ChannelMeasure(n, [(0, 0)], xdb=3.0, fraction=0.9) as m:
        for at in range(0, len(ranges), 16):
            m.configure(channels=ranges[at:at + 16], obw=ranges[at])
            _check(m, rows, f"channels {at}", offset_floats=offset)
        for k, (a, b) in enumerate(ranges):
            m.configure(channels=[(a, b)], obw=(a, b), fraction=FRACTIONS[k % 4], xdb=(0.0, 3.0, 1000.0)[k % 3])
            got = _check(m, rows, f"obw=({a}, {b})", offset_floats=offset)
            if a == b:                                                   # one bin: both edges inside it
                ok = got.flags == 0
                assert np.all(got.k_lo[ok] == a) and np.all(got.k_hi[ok] == a)
                assert np.allclose(got.x_hi[ok] - got.x_lo[ok], m.fraction, rtol=0, atol=1e-12)


# ---- x-dB ---------------------------------------------------------------------------------------------------------------
def test_xdb_of_zero_and_of_a_thousand_and_equal_maxima():
    n = 700
    row = np.full(n, -100.0, dtype=f32)
    row[300:360] = (-50.0 - 0.01 * np.abs(np.arange(60) - 30.0) ** 2).astype(f32)
    row[330] = row[331] = row[340] = -50.0                              # equal maxima: the first
    row[100] = np.nan
    row[650] = -np.inf
    for xdb, want in ((0.0, (330, 340)), (1000.0, (0, n - 1)), (3.0, None)):
        with ms.ChannelMeasure(n, [(0, n - 1), (331, 400)], xdb=xdb) as m:
            got = _check(m, row, f"xdb={xdb}")
            assert (got.peak_bin[0], got.peak_db[0]) == (330, -50.0) and got.channels["peak_bin"][0, 1] == 331
            if want:
                assert (got.xdb_lo[0], got.xdb_hi[0]) == want
            m.configure(obw=(101, 649))
            got = _check(m, row, f"xdb={xdb} inside")
            if xdb == 1000.0:
                assert (got.xdb_lo[0], got.xdb_hi[0]) == (101, 649)


# ---- the limit line -----------------------------------------------------------------------------------------------------
def test_limits_one_float32_step_either_side_of_a_bins_value():
    n = 1025
    rng = np.random.default_rng(12)
    row = (-80.0 + 3.0 * rng.standard_normal(n)).astype(f32)
    row[[7, 500]] = [0.0, -0.0]
    up, down = np.nextafter(row, f32(np.inf)), np.nextafter(row, f32(-np.inf))
    with ms.ChannelMeasure(n, [(0, n - 1)]) as m:
        for line, n_fail in ((row, 0), (up, 0), (down, n)):
            m.set_limit(line)
            got = _check(m, row, f"n_fail={n_fail}")
            assert got.n_fail[0] == n_fail and bool(got.mask_failed[0]) == (n_fail > 0)
        mixed = np.where(np.arange(n) % 3 == 0, down, np.where(np.arange(n) % 3 == 1, row, up))
        m.set_limit(mixed)
        got = _check(m, row, "mixed")
        assert got.n_fail[0] == len(range(0, n, 3)) and (got.first_fail[0], got.last_fail[0]) == (0, (n - 1) // 3 * 3)
        # the same lines relative to the main channel's peak: lim = float32(line - ref + ref) need not be the line
        ref = f32(np.max(row))
        m.set_limit((mixed - ref).astype(f32), relative=True)
        _check(m, row, "relative")


def test_nan_limits_nan_reference_and_failures_at_the_ends():
    n = 4097
    rng = np.random.default_rng(13)
    rows = (-90.0 + rng.standard_normal((6, n))).astype(f32)
    rows[1, 5:9] = np.nan                                              # the main channel of row 1 holds no number
    rows[2, 0] = rows[3, n - 1] = rows[4, 0] = rows[4, n - 1] = -40.0
    rows[5, 2000] = np.inf
    line = np.full(n, -60.0, dtype=f32)
    with ms.ChannelMeasure(n, [(5, 8), (0, n - 1)]) as m:
        m.set_limit(line)
        got = _check(m, rows, "ends")
        assert list(got.n_fail) == [0, 0, 1, 1, 2, 1]
        assert [(int(a), int(b)) for a, b in zip(got.first_fail, got.last_fail)] == \
            [(-1, -1), (-1, -1), (0, 0), (n - 1, n - 1), (0, n - 1), (2000, 2000)]
        assert got.worst_margin[5] == np.inf and got.worst_bin[5] == 2000 and list(got.mask_failed) == [False, False] + [True] * 4
        line[0] = line[n - 1] = np.nan                                   # the failing bins are not tested any more
        m.set_limit(line)
        got = _check(m, rows, "nan limit")
        assert list(got.n_fail) == [0, 0, 0, 0, 0, 1] and got.worst_bin[2] not in (0, n - 1)
        m.set_limit(np.full(n, np.nan, dtype=f32))
        got = _check(m, rows, "all nan")
        assert not got.n_fail.any() and np.all(got.worst_bin == -1) and np.all(np.isnan(got.worst_margin))
        m.set_limit(np.full(n, -200.0, dtype=f32), relative=True)      # everything fails - except against a NaN reference
        got = _check(m, rows, "nan reference")
        assert np.isnan(got.channels["peak_db"][1, 0]) and got.n_fail[1] == 0 and got.worst_bin[1] == -1
        assert np.all(got.n_fail[[0, 2, 3, 4]] == n) and got.flags[1] == 0
        m.set_limit(None)
        got = _check(m, rows, "no limit")
        assert not got.n_fail.any() and np.all(got.worst_bin == -1) and not (got.flags & ms.FLAG_MASK_FAIL).any()


# ---- channel power ------------------------------------------------------------------------------------------------------
def test_channel_power_has_the_detectors_bits():
    """Channels set to the detector's own [start, stop] on the same rows: the same tree, the same bits.  Runs of widths
    1, 63, 64, 65 and 4097, at bins that are no multiple of 64, two of them holding NaNs (bridged by the detector)."""
    n = 16384
    runs = [(10, 10), (101, 163), (300, 363), (1001, 1065), (5003, 9099), (12000, 12062), (16320, 16383)]
    assert [b - a + 1 for a, b in runs] == [1, 63, 64, 65, 4097, 63, 64]
    rng = np.random.default_rng(21)
    rows = (-100.0 + rng.standard_normal((9, n))).astype(f32)
    for a, b in runs:
        rows[:, a:b + 1] = (-60.0 + 3.0 * rng.standard_normal((9, b - a + 1))).astype(f32)
    rows[:, 7000] = np.nan
    rows[::2, 12030:12032] = np.nan
    with dt.SignalDetector(n, margin_db=20.0, max_gap=2, max_signals=8) as d, ms.ChannelMeasure(n, runs) as m, \
            DeviceBuffer.of(rows) as buf:
        det = d.process_device(None, buf.ptr, 9)
        assert np.all(det.n_found == len(runs))
        for r in range(9):
            assert [(int(s["start"]), int(s["stop"])) for s in det.signals[r][:len(runs)]] == runs
        got = m.process_device(None, buf.ptr, 9)
        assert _bits(got.channels["power"], det.signals["power"][:, :len(runs)])
        assert np.array_equal(got.channels["peak_bin"], det.signals["peak_bin"][:, :len(runs)])
        assert np.array_equal(got.channels["peak_db"], det.signals["peak_db"][:, :len(runs)])
        assert got.channels["n_nan"][0, 4] == 1 and got.channels["n_nan"][0, 5] == 2 and got.channels["n_nan"][1, 5] == 0
        _same(got, *_want(m, rows))


def test_channel_power_against_rows_stats():
    """On NaN-free ranges power is tdsa_rows_stats' band sum of the same bins - the same float32 terms widened, positive,
    in another order: within 2 width 2^-53 relative."""
    n = 4097
    rng = np.random.default_rng(3)
    row = (-100.0 + rng.standard_normal(n)).astype(f32)
    chans = [(0, 0), (60, 70), (126, 129), (200, 460), (1000, 2100), (4090, 4096), (0, 4096), (63, 64), (255, 1024)]
    row[200:461] = (-60.0 + 3.0 * rng.standard_normal(261)).astype(f32)
    with ms.ChannelMeasure(n, chans) as m, SpectrumEngine(64) as eng, DeviceBuffer.of(row) as buf:
        got = m.process_device(eng, buf.ptr, 1)
        for k, (a, b) in enumerate(chans):
            out = C.c_double()
            nat.check(nat.lib.tdsa_rows_stats(eng._h, buf.ptr, 1, n, a, b, -1.0, None, None, C.byref(out)))
            w, ref, pw = b - a + 1, out.value, got.channels["power"][0, k]
            print(f"channel {a}..{b}: power {pw!r} rows_stats {ref!r} rel {abs(pw - ref) / ref:.3e}")
            assert abs(pw - ref) <= 2 * w * 2.0 ** -53 * ref
        assert got.obw_total[0] == pytest.approx(got.channels["power"][0, 6], rel=2 * n * 2.0 ** -53)


# ---- occupied bandwidth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_BINS)
def test_obw_on_general_rows(n):
    """Every fraction on mixed rows, in the power domain; obw_total against the sum of the device's own p_i (the powers
    of one-bin channels), and the channel sums against the same terms."""
    rows = _mixed_rows(24, n, 3000 + n)
    p = _device_powers(rows)
    with np.errstate(all="ignore"):
        ok = ~np.isnan(rows) & ~np.isinf(rows)
        assert np.allclose(p[ok], mc.linear(rows[ok]), rtol=mc.POWER_RTOL, atol=0) and not p[np.isnan(rows)].any()
    with ms.ChannelMeasure(n, [(0, 0)]) as m:
        for obw in _ranges(n):
            for f in FRACTIONS:
                m.configure(channels=_channels(n, n)[:6], obw=obw, fraction=f)
                got = _on_device(m, rows, offset_floats=n % 2)
                tag = f"n={n} obw={obw} f={f}"
                _same(got, *_want(m, rows), tag)
                _obw(got, rows, m, tag)                                  # against numpy's p_i
                _obw(got, rows, m, tag + " device p", p=p, total_rtol=1e-12)
                for c, (a, b) in enumerate(m.channels):
                    w = p[:, a:b + 1].sum(axis=1)
                    fin = np.isfinite(w)
                    assert np.all(np.abs(got.channels["power"][fin, c] - w[fin]) <= 2 * (b - a + 1) * 2.0 ** -53 * w[fin]), tag
                    assert np.array_equal(got.channels["power"][~fin, c], w[~fin]), tag


def _exact_rows(n, lo, hi, rng):
    """Rows of 0.0 dB, -inf and NaN inside [lo, hi] whose T is a multiple of 4 (anything outside): planted crossings and
    random fills."""
    width = hi - lo + 1
    rows = []
    # two ones up to b_lo, four more up to b_hi, two behind: T = 8, targets 2 and 6 reached exactly at b_lo and b_hi
    spots = sorted({lo + 1, hi - 7} | {s + d for s in SEAMS + (128, 2048, 4096) for d in (-2, -1, 0, 1)})
    spots = [b for b in spots if lo + 1 <= b and b + 7 <= hi]
    for b_lo in spots:
        for b_hi in sorted({b_lo + 4, b_lo + 5, hi - 2} | {s + d for s in SEAMS for d in (-1, 0)}):
            if not b_lo + 4 <= b_hi <= hi - 2:
                continue
            for ones in ([lo, b_lo, b_lo + 1, b_lo + 2, b_lo + 3, b_hi, hi - 1, hi],       # power right behind b_lo
                         [lo, b_lo, b_hi - 3, b_hi - 2, b_hi - 1, b_hi, hi - 1, hi]):      # ... or a stretch of none
                row = np.full(n, -np.inf, dtype=f32)
                row[:lo], row[hi + 1:] = -30.0, np.nan
                row[ones] = 0.0
                assert len(set(ones)) == 8
                rows.append(row)
    for _ in range(12):                                                  # dense: ones, zero-power stretches, NaNs
        row = np.full(n, -30.0, dtype=f32)
        seg = rng.choice(np.array([0.0, 0.0, 0.0, -np.inf, np.nan], dtype=f32), width)
        if width >= 32:
            a = int(rng.integers(0, width))
            seg[a:a + int(rng.integers(0, 70))] = -np.inf               # a stretch of zero power
        ones = np.flatnonzero(seg == 0.0)
        seg[ones[:ones.size % 4]] = -np.inf
        row[lo:hi + 1] = seg
        if np.count_nonzero(seg == 0.0):
            rows.append(row)
    full = np.full(n, -30.0, dtype=f32)
    if width % 4 == 0:
        full[lo:hi + 1] = 0.0
        rows.append(full)
    return np.stack(rows) if rows else np.zeros((0, n), dtype=f32)


@pytest.mark.parametrize("n", (8, 64, 65, 257, 1025, 4097, 16384))
def test_obw_crossings_are_bit_equal_where_the_sums_are_exact(n):
    """Every bin 0.0 dB, -inf or NaN: p is 1 or 0 and every partial sum an integer.  T is a multiple of 4 and f = 0.5, so
    both targets are integers: a crossing lands on the upper edge of the bin that reaches it, never in the zero-power
    bins behind it, whatever seam lies there."""
    rng = np.random.default_rng(n)
    for lo, hi in ((0, n - 1), (n // 5, n - 1 - n // 7)):
        if hi - lo + 1 < 4:
            continue
        rows = _exact_rows(n, lo, hi, rng)
        assert len(rows) >= 2
        with ms.ChannelMeasure(n, [(lo, hi)], obw=(lo, hi), fraction=0.5, xdb=0.0) as m:
            rr, ch = _want(m, rows)
            assert not rr["flags"].any() and np.all(rr["obw_total"] % 4 == 0) and np.all(rr["x_lo"] == rr["k_lo"] + 0.5)
            for off in (0, 1):
                got = _on_device(m, rows, off)
                for f in ("k_lo", "k_hi", "x_lo", "x_hi", "obw_total"):
                    assert _bits(got.rows[f], rr[f]), (n, lo, hi, f, got.rows[f], rr[f])
                assert _bits(got.channels["power"], ch["power"])
                _same(got, rr, ch)


def test_obw_flags():
    n = 300
    rows = np.full((5, n), -90.0, dtype=f32)
    rows[0, 50:250] = np.nan                                            # the range holds no number
    rows[1, 50:250] = -np.inf                                           # ... no power
    rows[2, 100] = np.inf                                               # T = +inf
    rows[3, 50:250] = np.nan
    rows[3, 77] = -85.0                                                 # one bin of power among NaNs
    with ms.ChannelMeasure(n, [(0, n - 1)], obw=(50, 249), fraction=0.9) as m:
        got = _check(m, rows)
        assert list(got.flags) == [ms.FLAG_EMPTY, ms.FLAG_EMPTY, ms.FLAG_INF, 0, 0]
        assert list(got.k_lo[:3]) == [-1] * 3 and np.all(np.isnan(got.x_lo[:3])) and np.all(np.isnan(got.x_hi[:3]))
        assert (got.obw_total[0], got.obw_total[1], got.obw_total[2]) == (0.0, 0.0, np.inf)
        assert (got.k_lo[3], got.k_hi[3], got.n_nan[3]) == (77, 77, 199) and abs(got.x_hi[3] - got.x_lo[3] - 0.9) < 1e-12
        assert (got.peak_bin[0], got.xdb_lo[0], got.peak_bin[1], got.xdb_lo[1], got.xdb_hi[1]) == (-1, -1, 50, 50, 249)


# ---- invariance, and behind the engine ----------------------------------------------------------------------------------
def test_a_rows_records_do_not_depend_on_where_it_sits():
    n = 4096
    rows = _mixed_rows(40, n, 77)
    with ms.ChannelMeasure(n, _channels(n, 4), obw=(100, 4000), limit=_limit(n, 4), max_host_rows=64) as m:
        full = _on_device(m, rows)
        for r in (0, 7, 13, 39):
            for ctx in (rows[r:r + 1], np.concatenate([rows[20:25], rows[r:r + 1]]), np.concatenate([rows[r:r + 1], rows[:3]])):
                at = 5 if ctx.shape[0] == 6 else 0
                for got in (_on_device(m, ctx), _on_device(m, ctx, 1), _on_device(m, ctx, 3), m.process(ctx)):
                    assert _bits(got.rows[at], full.rows[r]) and _bits(got.channels[at], full.channels[r])


def test_behind_the_engine_on_its_stream_and_totals():
    """IQ in, dB rows written by the engine into device memory, the measurement behind it on the engine's stream: the
    rows are read back afterwards, for the contract only.  Then the totals over several calls and after a reset."""
    nfft, frames = 1024, 24
    rng = np.random.default_rng(9)
    t = np.arange(nfft * frames)
    x = 0.01 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for f, a in ((0.1, 1.0), (0.1004, 1.0), (-0.3, 0.3)):
        x += a * np.exp(2j * np.pi * f * t)
    x = x.astype(np.complex64)
    main = (nfft // 2 + 92, nfft // 2 + 112)
    with SpectrumEngine(nfft, max_frames=frames) as eng, DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(4 * nfft * frames) as d_rows, \
            ms.ChannelMeasure(nfft, [main, (main[0] - 21, main[0] - 1), (main[1] + 1, main[1] + 21)], xdb=20.0) as m:
        eng.set_window(np.hanning(nfft).astype(f32))
        d_x.put(x)
        eng.process_device(nat.IN_C64, d_x.ptr, x.size, nfft, frames, d_rows.ptr)
        got = m.process_device(eng, d_rows.ptr, frames)
        rows = d_rows.get((frames, nfft), f32)
        _same(got, *_want(m, rows))
        _obw(got, rows, m)
        assert np.all(got.acpr_db()[:, 1:] < -20.0) and m.totals() == (frames, 0)
        again = m.process_device(None, d_rows.ptr, frames)
        assert _bits(again.rows, got.rows) and _bits(again.channels, got.channels)
        m.set_limit(np.full(nfft, -30.0, dtype=f32), relative=True)   # the third tone is 10 dB down: above -30 dBc
        failing = m.process_device(eng, d_rows.ptr, frames)
        assert np.all(failing.mask_failed) and m.totals() == (3 * frames, frames)
        m.process(rows[:5])
        assert m.totals() == (3 * frames + 5, frames + 5)
        m.reset()
        assert m.totals() == (0, 0)
        m.set_limit(None)
        m.process(rows[:2])
        assert m.totals() == (2, 0)


# ---- offsets past 2^32 bytes -------------------------------------------------------------------------------------------
def test_rows_past_4_gib():
    n, n_rows = 16384, 65538
    assert (n_rows - 2) * n * 4 >= 1 << 32
    rng = np.random.default_rng(4)
    planted = (-100.0 + rng.standard_normal((4, n))).astype(f32)
    for k, (a, b) in enumerate(((0, 40), (8000, 8100), (16000, 16383), (5, 5))):
        planted[k, a:b + 1] = -50.0 - k
    block = np.full((1024, n), -100.0, dtype=f32)
    line = np.full(n, -70.0, dtype=f32)
    with ms.ChannelMeasure(n, [(0, n - 1), (7990, 8110)], fraction=0.9, xdb=3.0, limit=line) as m, SpectrumEngine(64) as eng, \
            room_or_skip(n_rows * n * 4) as buf:
        row_bytes = 4 * n
        buf.put(block)
        size = block.nbytes                                           # double the constant block on the device
        while size < n_rows * row_bytes:
            step = min(size, n_rows * row_bytes - size)
            nat.check(nat.lib.tdsa_plan_copy(eng._h, buf.at(size, step), buf.ptr, step, 1))
            size += step
        buf.put(planted[:2])
        buf.put(planted[2:], (n_rows - 2) * row_bytes)
        got = m.process_device(eng, buf.ptr, n_rows)
        at = [0, 1, n_rows - 2, n_rows - 1]
        sub = ms.measurements_from(got.rows[at], got.channels[at])
        _same(sub, *_want(m, planted))
        _obw(sub, planted, m)
        assert list(sub.n_fail) == [41, 101, 384, 1] and list(sub.peak_bin) == [0, 8000, 16000, 5]
        rest = np.ones(n_rows, dtype=bool)
        rest[at] = False
        one = m.process_device(None, buf.at(2 * row_bytes, row_bytes), 1)          # a constant row on its own
        assert np.all(got.rows[rest] == one.rows[0]) and np.all(got.channels[rest] == one.channels[0])
        assert (one.n_fail[0], one.peak_bin[0], one.xdb_hi[0], one.worst_margin[0]) == (0, 0, n - 1, -30.0)
        assert m.totals() == (n_rows + 1, 4)


# ---- argument errors that need a handle --------------------------------------------------------------------------------
def test_library_refuses_bad_calls_on_a_live_handle():
    lib = nat.lib
    h = C.c_void_p()
    nat.check(lib.tdsa_meas_create(0, 64, 2, C.byref(h)))
    try:
        rows = np.zeros((3, 64), dtype=f32)
        rr, ch = np.zeros(3, dtype=ms.ROW_RECORD), np.zeros((3, 16), dtype=ms.CHANNEL_RECORD)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
        ints = lambda *v: (C.c_int * len(v))(*v)                      # noqa: E731
        assert lib.tdsa_meas_process(h, p(rows), 1, p(rr), p(ch)) == -1 and b"not configured" in lib.tdsa_last_error_string()
        assert lib.tdsa_meas_process_dev(h, None, p(rows), 1, p(rr), p(ch)) == -1
        for args in ((1, ints(0), ints(64), 0, 63, 0.99, 26.0), (2, ints(0, 3), ints(63, 64), 0, 63, 0.99, 26.0),
                     (1, ints(0), ints(63), 0, 64, 0.99, 26.0), (1, ints(0), ints(63), 64, 64, 0.99, 26.0)):
            assert lib.tdsa_meas_configure(h, *args) == -1, args
            assert b"handle's 64 bins" in lib.tdsa_last_error_string()
        assert lib.tdsa_meas_process(h, p(rows), 1, p(rr), p(ch)) == -1          # a refused configuration configures nothing
        nat.check(lib.tdsa_meas_configure(h, 2, ints(0, 10), ints(63, 20), 0, 63, 0.99, 26.0))
        line = np.zeros(65, dtype=f32)
        assert lib.tdsa_meas_set_limit(h, p(line), 65, 0) == -1 and b"one per bin" in lib.tdsa_last_error_string()
        assert lib.tdsa_meas_set_limit(h, p(line), 63, 0) == -1
        assert lib.tdsa_meas_set_limit(h, p(line), 64, 2) == -1
        assert lib.tdsa_meas_set_limit(h, p(line), 64, 1) == 0 and lib.tdsa_meas_set_limit(h, None, 0, 0) == 0
        assert lib.tdsa_meas_process(h, None, 1, p(rr), p(ch)) == -1
        assert lib.tdsa_meas_process(h, p(rows), 1, None, p(ch)) == -1
        assert lib.tdsa_meas_process(h, p(rows), 1, p(rr), None) == -1
        assert lib.tdsa_meas_process(h, p(rows), 3, p(rr), p(ch)) == -1 and b"max_host_rows" in lib.tdsa_last_error_string()
        assert lib.tdsa_meas_read_totals(h, None, None) == -1
        assert lib.tdsa_meas_timer_end(h, None) == -1
        rr[:] = 7
        assert lib.tdsa_meas_process(h, p(rows), 0, p(rr), p(ch)) == 0 and np.all(rr["n_fail"] == 7)
        with DeviceBuffer(1024) as buf:
            assert lib.tdsa_meas_process_dev(h, None, buf.at(2), 1, p(rr), p(ch)) == -1
            assert b"aligned" in lib.tdsa_last_error_string()
            assert lib.tdsa_meas_process_dev(h, None, buf.ptr, 0, p(rr), p(ch)) == 0 and np.all(rr["n_fail"] == 7)
        seen = C.c_uint64(9)
        nat.check(lib.tdsa_meas_read_totals(h, C.byref(seen), None))
        assert seen.value == 0
        nat.check(lib.tdsa_meas_process(h, p(rows), 2, p(rr), p(ch)))   # a live handle, configured again, still runs
        nat.check(lib.tdsa_meas_configure(h, 1, ints(5), ints(5), 5, 5, 0.5, 0.0))
        nat.check(lib.tdsa_meas_process(h, p(rows), 2, p(rr), p(ch)))
        assert list(rr["k_lo"][:2]) == [5, 5] and list(rr["obw_total"][:2]) == [1.0, 1.0]
        nat.check(lib.tdsa_meas_read_totals(h, C.byref(seen), None))
        assert seen.value == 4
        cnt = C.c_int()
        nat.check(lib.tdsa_device_count(C.byref(cnt)))
        if cnt.value > 1:                                             # a plan on another device is refused
            with SpectrumEngine(64, device=1) as other, DeviceBuffer(1024) as buf:
                assert lib.tdsa_meas_process_dev(h, other._h, buf.ptr, 1, p(rr), p(ch)) == -1
                assert b"different devices" in lib.tdsa_last_error_string()
    finally:
        lib.tdsa_meas_destroy(h)
