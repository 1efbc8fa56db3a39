"""The signal detection on the device (tdsa_detect_*) against tests/detect_contract.py: floor,
threshold, counts, flags, every integer of the signal records, peak_db, the padding records and the occupancy counts
under np.array_equal; power and moment within POWER_RTOL (the figure tests/test_gpu_analytics.py holds for exp10f on the
device against float32 10 ** x in numpy) and, on NaN-free runs, within 2 width 2^-53 of tdsa_rows_stats, whose terms are
the same bits in another order; a row's records bit-equal across n_rows, its place, the entry point and the load path."""
import ctypes as C

import numpy as np
import pytest

import detect_contract as dc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import detect as dt

pytestmark = pytest.mark.gpu

N_BINS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16383, 16384)
INT_FIELDS = ("start", "stop", "peak_bin", "x_lo", "x_hi")
f32 = np.float32


def _params(d):
    return dict(lo=d.bins[0], hi=d.bins[1], rank=d.rank, margin_db=d.margin_db, min_width=d.min_width, max_gap=d.max_gap,
                xdb=d.xdb, S=d.max_signals)


def _on_device(d, rows, offset_floats=0, engine=None):
    """The rows through the device entry point, `offset_floats` floats into a 16-byte aligned buffer."""
    rows = np.ascontiguousarray(rows, dtype=f32)
    with DeviceBuffer(rows.nbytes + 4 * offset_floats + 16) as buf:
        assert buf.ptr % 16 == 0
        buf.put(rows, 4 * offset_floats)
        return d.process_device(engine, buf.at(4 * offset_floats, rows.nbytes), rows.shape[0])


def _same(got, want_rr, want_sig, tag=""):
    """A call's records against the contract's."""
    assert np.array_equal(got.floor, want_rr["floor"], equal_nan=True), tag          # by value
    assert np.array_equal(got.thr, want_rr["thr"], equal_nan=True), tag
    for f in ("n_found", "n_over", "flags"):
        assert np.array_equal(getattr(got, f), want_rr[f]), (tag, f)
    assert not got.rows["reserved"].any(), tag
    for f in INT_FIELDS:
        assert np.array_equal(got.signals[f], want_sig[f]), (tag, f)
    assert np.array_equal(got.signals["peak_db"], want_sig["peak_db"], equal_nan=True), tag
    for f in ("power", "moment"):
        assert np.allclose(got.signals[f], want_sig[f], rtol=dc.POWER_RTOL, atol=0, equal_nan=True), (tag, f)


def _check(d, rows, tag="", offset_floats=0, host=False, want=None):
    """Process the rows (device entry point, or the host one) and hold the result against the contract (`want`: what
    dc.detect returned for these rows and parameters before); returns (result, the contract's occupancy of the call,
    rows flagged)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=f32))
    got = d.process(rows) if host else _on_device(d, rows, offset_floats)
    rr, sig, occ, _, flagged = want if want is not None else dc.detect(rows, **_params(d))
    _same(got, rr, sig, tag)
    return got, occ, flagged


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _mixed_rows(n_rows, n, seed):
    """Rows with everything at once: noise (every other row in 0.25 dB steps, so values repeat), emissions with flat
    tops, single-bin spikes, NaNs and infinities; then a constant row, an all-NaN row, a mostly-NaN row and an
    alternating row where the count allows."""
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
    if n_rows >= 8:
        rows[4] = f32(-97.5)
        rows[5] = np.nan
        rows[6, rng.random(n) < 0.7] = np.nan
        rows[7] = np.where(np.arange(n) % 2 == 0, f32(-100.0), f32(-40.0))
    return rows


def _ranges(n):
    """The whole row; lo and hi at odd places inside their 64-bin words; a single bin."""
    out = [(0, n - 1)]
    if n >= 8:
        lo, hi = (n // 3) | 1, min(n - 2, (2 * n // 3) | 1)
        out.append((lo, max(lo, hi)))
    out.append((n // 2, n // 2))
    return out


CONFIGS = (dict(margin_db=6.0, min_width=1, max_gap=0, xdb=3.0, max_signals=16),
           dict(margin_db=3.0, min_width=3, max_gap=2, xdb=0.0, max_signals=2),
           dict(margin_db=0.5, min_width=2, max_gap=65, xdb=1000.0, max_signals=64))


# ---- every shape, both load paths, every range --------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_BINS)
def test_every_shape_against_the_contract(n):
    """Mixed rows per n_bins, 257 of them in the first configuration and 24 in the others; n_rows = 1, 2, 3 are the
    first rows (and must repeat their bits), the buffer is 16-byte aligned and one float off, and the occupancy is the
    sum of every call's."""
    all_rows = _mixed_rows(257, n, 1000 + n)
    first = True
    with dt.SignalDetector(n, max_host_rows=257) as d:
        for ci, cfg in enumerate(CONFIGS):
            cfg = dict(cfg, min_width=min(cfg["min_width"], n), max_gap=min(cfg["max_gap"], n))
            for (lo, hi) in _ranges(n):
                for rank in sorted({0, (hi - lo) // 2, hi - lo}) if ci == 0 else [(hi - lo) // 2]:
                    rows = all_rows if first else all_rows[:24]
                    d.configure(bins=(lo, hi), rank=rank, **cfg)
                    d.reset()
                    tag = f"n={n} cfg={ci} bins=({lo}, {hi}) rank={rank}"
                    want = dc.detect(rows, **_params(d))
                    full, occ, flagged = _check(d, rows, tag, want=want)
                    seen = len(rows)
                    for k, off in ((1, 1), (2, 0), (3, 1)):
                        part, o, fl = _check(d, rows[:k], tag + f" n_rows={k}", offset_floats=off)
                        assert _bits(part.rows, full.rows[:k]) and _bits(part.signals, full.signals[:k]), tag
                        occ, flagged, seen = occ + o, flagged + fl, seen + k
                    if first or rank == 0:
                        off1, o, fl = _check(d, rows, tag + " one float off", offset_floats=1, want=want)
                        host, o2, _ = _check(d, rows, tag + " host", host=True, want=want)
                        assert _bits(off1.rows, full.rows) and _bits(off1.signals, full.signals), tag
                        assert _bits(host.rows, full.rows) and _bits(host.signals, full.signals), tag
                        occ, flagged, seen = occ + o + o2, flagged + 2 * fl, seen + 2 * len(rows)
                    counts, rows_seen, rows_flagged = d.occupancy()
                    assert np.array_equal(counts, occ) and (rows_seen, rows_flagged) == (seen, flagged), tag
                    first = False


# ---- the floor ---------------------------------------------------------------------------------------------------------
def test_every_rank_of_a_row_of_distinct_values():
    rng = np.random.default_rng(65)
    row = rng.permutation(np.linspace(-120.0, -20.0, 65)).astype(f32)
    assert np.unique(row).size == 65
    with dt.SignalDetector(65) as d:
        for rank in range(65):
            d.configure(rank=rank, margin_db=0.0)
            got, _, _ = _check(d, row, f"rank={rank}")
            assert got.floor[0] == np.sort(row)[rank] and got.n_over[0] == 64 - rank


@pytest.mark.parametrize("n", (65, 1024))
def test_ranks_among_equal_values_infinities_and_nans(n):
    rng = np.random.default_rng(n)
    equal = rng.choice(np.array([-100.0, -99.5, -0.0, 0.0, 3.0], dtype=f32), n)
    infs = (-100.0 + rng.standard_normal(n)).astype(f32)
    infs[rng.integers(0, n, 5)] = np.inf
    infs[rng.integers(0, n, 5)] = -np.inf
    nans = (-100.0 + rng.standard_normal(n)).astype(f32)
    k = n // 4
    nans[rng.permutation(n)[:k]] = np.nan
    nans[0] = np.array([0xFFC00000], dtype=np.uint32).view(f32)[0]            # a NaN with the sign bit set sorts last too
    all_nan = np.full(n, np.nan, dtype=f32)
    rows = np.stack([equal, infs, nans, all_nan])
    n_nan = int(np.isnan(nans).sum())
    n_ninf, n_pinf = int(np.isneginf(infs).sum()), int(np.isposinf(infs).sum())
    assert n_nan >= 2 and n_ninf >= 1 and n_pinf >= 1
    ranks = {0, 1, n // 2, n - 2, n - 1, n - n_nan - 2, n - n_nan - 1, n - n_nan, n_ninf - 1, n_ninf, n - n_pinf - 1,
             n - n_pinf}
    with dt.SignalDetector(n) as d:
        for rank in sorted(r for r in ranks if 0 <= r < n):
            d.configure(rank=rank, margin_db=1.0)
            got, _, flagged = _check(d, rows, f"n={n} rank={rank}")
            assert got.flags[3] == dc.FLAG_NAN_FLOOR and got.flags[2] == (rank >= n - n_nan) and flagged >= 1
            if rank == n - n_nan - 1:                     # one below the first NaN: the largest number of the row
                assert got.floor[2] == np.nanmax(nans) and got.n_over[2] == 0
        d.reset()
        d.configure(rank=n - n_nan, margin_db=1.0)
        got, occ, flagged = _check(d, rows, "flagged rows")
        counts, seen, fl = d.occupancy()
        assert (seen, fl) == (4, flagged) and flagged == 2 and np.array_equal(counts, occ)


def test_constant_rows_hold_no_signal_at_margin_zero():
    for n in (1, 64, 1000, 16384):
        rows = np.stack([np.full(n, v, dtype=f32) for v in (-100.0, 0.0, -0.0, np.inf, -np.inf, 1e-45)])
        with dt.SignalDetector(n, margin_db=0.0) as d:
            got, occ, _ = _check(d, rows, f"n={n}")
            assert not got.n_over.any() and not got.n_found.any() and not occ.any() and not got.flags.any()


def test_values_one_step_either_side_of_the_threshold():
    n = 300
    for base, margin in ((-100.0, 10.0), (-37.123, 6.02), (0.0, 1e-3), (-1e-3, 0.5)):
        row = np.full(n, base, dtype=f32)
        thr = f32(f32(base) + f32(margin))
        row[10], row[20], row[30] = np.nextafter(thr, f32(np.inf)), thr, np.nextafter(thr, f32(-np.inf))
        row[63], row[64] = np.nextafter(thr, f32(np.inf)), thr
        with dt.SignalDetector(n, margin_db=margin) as d:
            got, _, _ = _check(d, row, f"base={base}")
            assert got.thr[0] == thr and got.n_over[0] == 2 and got.n_found[0] == 2
            assert list(got.signals["start"][0][:2]) == [10, 63] and list(got.signals["stop"][0][:2]) == [10, 63]


# ---- runs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (0, 1))
def test_runs_start_and_stop_on_every_bin_next_to_a_seam(offset):
    """One row per (start, stop) around the seams of the 64-bin words, the 256-bin strides of the float loads and the
    1024-bin strides of the 16-byte loads, and at the ends of the search range."""
    n, lo, hi = 2100, 3, 2090
    rng = np.random.default_rng(7)
    rows = []
    for seam in (64, 128, 256, 1024, 2048):
        for a in range(seam - 2, seam + 2):
            for b in range(a, seam + 3):
                row = (-100.0 + rng.standard_normal(n)).astype(f32)
                row[a:b + 1] = -50.0
                rows.append(row)
    for a, b in ((0, 5), (lo, lo), (lo, lo + 1), (lo - 1, lo + 2), (hi, hi), (hi - 1, hi), (hi - 1, n - 1), (lo + 1, lo + 900)):
        row = (-100.0 + rng.standard_normal(n)).astype(f32)
        row[a:b + 1] = -50.0
        rows.append(row)
    whole = (-100.0 + rng.standard_normal(n)).astype(f32)
    whole[n // 2 - 10:] = -50.0                                       # more than half of either range: the median is signal
    rows.append(whole)
    rows = np.stack(rows)
    with dt.SignalDetector(n, bins=(lo, hi), min_width=1, max_gap=0) as d:
        got, _, _ = _check(d, rows, offset_floats=offset)
        assert np.all(got.n_found[:-1] == 1) and got.n_found[-1] == 0
    with dt.SignalDetector(n, min_width=1, max_gap=0) as d:
        got, _, _ = _check(d, rows, offset_floats=offset)
        assert np.all(got.n_found[:-1] == 1) and got.n_found[-1] == 0


@pytest.mark.parametrize("max_gap", (0, 1, 2, 63, 64, 65, 512))
def test_gaps_of_exactly_max_gap_and_one_more(max_gap):
    n = 512
    rows, want = [], []
    for shift in list(range(0, 70, 7)) + [n - max_gap - 3, n - max_gap - 2]:
        for gap in (max_gap, max_gap + 1):
            if shift < 0 or shift + gap + 2 > n:
                continue
            row = np.full(n, -100.0, dtype=f32)
            row[shift] = row[shift + gap + 1] = -50.0                   # `gap` clear bins between the two
            rows.append(row)
            want.append(1 if gap <= max_gap else 2)
    ends = np.full(n, -100.0, dtype=f32)
    ends[0] = ends[n - 1] = -50.0                                     # the widest gap a row has
    rows.append(ends)
    want.append(1 if n - 2 <= max_gap else 2)
    with dt.SignalDetector(n, max_gap=max_gap, margin_db=10.0, rank=1) as d:
        got, _, _ = _check(d, np.stack(rows), f"max_gap={max_gap}")
        assert list(got.n_found) == want
        merged = np.array([i for i, w in enumerate(want[:-1]) if w == 1], dtype=np.int64)
        assert np.all(got.signals["stop"][merged, 0] - got.signals["start"][merged, 0] == max_gap + 1)


@pytest.mark.parametrize("min_width", (1, 2, 5, 64, 65, 200))
def test_widths_of_exactly_min_width_and_one_less(min_width):
    n = 1024
    rows = []
    for a in (0, 60, 63, 130, n - min_width):
        for w in (min_width, min_width - 1):
            row = np.full(n, -100.0, dtype=f32)
            row[a:a + w] = -50.0
            rows.append(row)                                          # before merging: kept, dropped
    for a in (5, 62, 250):                                            # after merging over a gap of 2: w1 + 2 + w2 bins
        for total in (min_width, min_width - 1):
            if total < 4:
                continue
            row = np.full(n, -100.0, dtype=f32)
            w1 = (total - 2) // 2
            row[a:a + w1] = -50.0
            row[a + w1 + 2:a + total] = -50.0
            rows.append(row)
    rows = np.stack(rows)
    for max_gap in (0, 2):
        with dt.SignalDetector(n, min_width=min_width, max_gap=max_gap, rank=0) as d:
            got, _, _ = _check(d, rows, f"min_width={min_width} max_gap={max_gap}")
            assert list(got.n_found[:10]) == [1, 0] * 5


def test_nan_in_a_bridged_gap_equal_maxima_and_the_xdb_edges():
    n = 700
    row = np.full(n, -100.0, dtype=f32)
    row[100:140] = -60.0
    row[120] = np.nan                                                 # bridged at max_gap >= 1, adds no power
    row[105] = row[131] = row[133] = -55.0                            # equal maxima: the first
    row[300:360] = (-50.0 - 0.01 * np.abs(np.arange(60) - 30.0) ** 2).astype(f32)
    row[330] = row[331] = -50.0
    row[500:520] = -70.0
    row[509], row[510] = -np.inf, np.nan                              # -inf adds zero power
    for max_gap in (0, 1, 2):
        for xdb in (0.0, 3.0, 1000.0):
            with dt.SignalDetector(n, max_gap=max_gap, xdb=xdb) as d:
                got, _, _ = _check(d, row, f"max_gap={max_gap} xdb={xdb}")
                s = got.signals[0]
                assert got.n_found[0] == {0: 5, 1: 4, 2: 3}[max_gap]
                if max_gap >= 1:
                    assert (s["start"][0], s["stop"][0], s["peak_bin"][0]) == (100, 139, 105)
                    assert (s["x_lo"][0], s["x_hi"][0]) == ((105, 133) if xdb < 5 else (100, 139))
                    assert s["peak_bin"][1] == 330
                    if xdb == 0.0:
                        assert (s["x_lo"][1], s["x_hi"][1]) == (330, 331)
                    if xdb == 1000.0:
                        assert (s["x_lo"][1], s["x_hi"][1]) == (300, 359)


@pytest.mark.parametrize("S", (1, 2, 64))
def test_alternating_mask_and_the_first_s_records(S):
    for n, lo, hi in ((16384, 0, 16383), (16383, 1, 16380), (130, 0, 129)):
        alt = np.where(np.arange(n) % 2 == 1, f32(-40.0), f32(-100.0))
        rows = [alt]
        for k in (S - 1, S, S + 1, 2 * S + 3):                        # n_found below, at and above S
            row = np.full(n, -100.0, dtype=f32)
            row[lo + 1 + 2 * np.arange(min(k, (hi - lo) // 2))] = -40.0
            rows.append(row)
        with dt.SignalDetector(n, bins=(lo, hi), rank=0, max_signals=S) as d:
            got, _, _ = _check(d, np.stack(rows), f"n={n} S={S}")
            n_eff = hi - lo + 1
            assert got.n_found[0] == n_eff // 2 == got.n_over[0]
            assert list(got.n_found[1:]) == [min(k, (hi - lo) // 2) for k in (S - 1, S, S + 1, 2 * S + 3)]
            assert np.array_equal(got.signals["start"][0], lo + (1 - lo % 2) + 2 * np.arange(S))


# ---- the two sums ------------------------------------------------------------------------------------------------------
def test_power_and_moment_against_rows_stats():
    """On NaN-free runs power is tdsa_rows_stats' band sum of the same bins - the same float32 terms widened, positive,
    in another order: within 2 width 2^-53 relative.  The moment is held the same way against the exact sum of
    (i - start) p_i with p_i taken back from the device: band sums of single bins."""
    n = 4097
    rng = np.random.default_rng(3)
    row = (-100.0 + rng.standard_normal(n)).astype(f32)
    runs = [(0, 0), (60, 70), (126, 129), (200, 460), (1000, 2100), (4090, 4096)]
    for a, b in runs:
        row[a:b + 1] = (-60.0 + 3.0 * rng.standard_normal(b - a + 1)).astype(f32)
    with dt.SignalDetector(n, margin_db=20.0, max_gap=0) as d, SpectrumEngine(64) as eng, DeviceBuffer(4 * n) as buf:
        buf.put(row)
        got = d.process_device(eng, buf.ptr, 1)
        s = got.signals[0]
        assert [(int(x["start"]), int(x["stop"])) for x in s[:got.count(0)]] == runs

        def band(a, b):
            out = C.c_double()
            nat.check(nat.lib.tdsa_rows_stats(eng._h, buf.ptr, 1, n, a, b, -1.0, None, None, C.byref(out)))
            return out.value
        for k, (a, b) in enumerate(runs):
            w = b - a + 1
            ref = band(a, b)
            print(f"run {a}..{b}: power {s['power'][k]!r} rows_stats {ref!r} rel {abs(s['power'][k] - ref) / ref:.3e}")
            assert abs(s["power"][k] - ref) <= 2 * w * 2.0 ** -53 * ref
            if w <= 300:
                p = np.array([band(i, i) for i in range(a, b + 1)])
                mo = float(np.sum(np.arange(w, dtype=np.float64) * p))
                assert abs(s["moment"][k] - mo) <= 2 * w * 2.0 ** -53 * mo


# ---- invariance, and behind the engine ----------------------------------------------------------------------------------
def test_a_rows_records_do_not_depend_on_where_it_sits():
    n = 4096
    rows = _mixed_rows(40, n, 77)
    with dt.SignalDetector(n, max_gap=3, min_width=2, max_host_rows=64) as d:
        full = _on_device(d, rows)
        for r in (0, 7, 13, 39):
            for ctx in (rows[r:r + 1], np.concatenate([rows[20:25], rows[r:r + 1]]), np.concatenate([rows[r:r + 1], rows[:3]])):
                at = 5 if ctx.shape[0] == 6 else 0
                for got in (_on_device(d, ctx), _on_device(d, ctx, 1), _on_device(d, ctx, 3), d.process(ctx)):
                    assert _bits(got.rows[at], full.rows[r]) and _bits(got.signals[at], full.signals[r])


def test_behind_the_engine_on_its_stream():
    """IQ in, dB rows written by the engine into device memory, the detector behind it on the engine's stream: the rows
    are read back afterwards, for the contract only."""
    nfft, frames = 1024, 24
    rng = np.random.default_rng(9)
    t = np.arange(nfft * frames)
    x = 0.01 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for f, a in ((0.1, 1.0), (0.1004, 1.0), (-0.3, 0.3)):
        x += a * np.exp(2j * np.pi * f * t)
    x = x.astype(np.complex64)
    with SpectrumEngine(nfft, max_frames=frames) as eng, dt.SignalDetector(nfft, margin_db=15.0, max_gap=2) as d, \
            DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(4 * nfft * frames) as d_rows:
        eng.set_window(np.hanning(nfft).astype(f32))
        d_x.put(x)
        eng.process_device(nat.IN_C64, d_x.ptr, x.size, nfft, frames, d_rows.ptr)
        got = d.process_device(eng, d_rows.ptr, frames)
        rows = d_rows.get((frames, nfft), f32)
        rr, sig, occ, _, _ = dc.detect(rows, **_params(d))
        _same(got, rr, sig)
        assert np.all(got.n_found >= 2) and np.array_equal(d.occupancy()[0], occ)
        again = d.process_device(None, d_rows.ptr, frames)
        assert _bits(again.rows, got.rows) and _bits(again.signals, got.signals)


# ---- occupancy ---------------------------------------------------------------------------------------------------------
def test_occupancy_accumulates_resets_and_does_not_depend_on_the_split():
    n = 1025
    rows = _mixed_rows(257, n, 31)
    with dt.SignalDetector(n, max_host_rows=257) as one, dt.SignalDetector(n, max_host_rows=257) as many:
        _, occ, flagged = _check(one, rows)
        assert flagged >= 1
        counts, seen, fl = one.occupancy()
        assert np.array_equal(counts, occ) and (seen, fl) == (257, flagged) and counts.dtype == np.uint32
        with DeviceBuffer(rows.nbytes) as buf:
            buf.put(rows)
            for r in range(257):
                many.process_device(None, buf.at(4 * n * r, 4 * n), 1)
        c2, s2, f2 = many.occupancy()
        assert _bits(c2, counts) and (s2, f2) == (257, flagged)
        one.process(rows[:100])
        counts, seen, fl = one.occupancy()
        assert np.array_equal(counts, occ + dc.detect(rows[:100], **_params(one))[2]) and seen == 357
        one.reset()
        counts, seen, fl = one.occupancy()
        assert not counts.any() and (seen, fl) == (0, 0)
        one.process(rows[5:6])                                        # the all-NaN row: flagged, adds to no bin
        counts, seen, fl = one.occupancy()
        assert not counts.any() and (seen, fl) == (1, 1)


# ---- offsets past 2^32 bytes -------------------------------------------------------------------------------------------
def test_rows_past_4_gib():
    n, n_rows, S = 16384, 65538, 4
    assert (n_rows - 2) * n * 4 >= 1 << 32
    rng = np.random.default_rng(4)
    planted = (-100.0 + rng.standard_normal((4, n))).astype(f32)
    for k, (a, b) in enumerate(((0, 40), (8000, 8100), (16000, 16383), (5, 5))):
        planted[k, a:b + 1] = -50.0 - k
    block = np.full((1024, n), -100.0, dtype=f32)
    with dt.SignalDetector(n, max_signals=S, margin_db=10.0) as d, SpectrumEngine(64) as eng, \
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
        got = d.process_device(eng, buf.ptr, n_rows)
        rr, sig, occ, _, _ = dc.detect(planted, **_params(d))
        at = [0, 1, n_rows - 2, n_rows - 1]
        sub = dt.detections_from(got.rows[at], got.signals[at])
        _same(sub, rr, sig)
        assert list(sub.n_found) == [1, 1, 1, 1]
        rest = np.ones(n_rows, dtype=bool)
        rest[at] = False
        assert not got.n_found[rest].any() and not got.n_over[rest].any() and not got.flags.any()
        assert np.all(got.floor[rest] == f32(-100.0)) and np.all(got.signals["start"][rest] == -1)
        counts, seen, flagged = d.occupancy()
        assert np.array_equal(counts, occ) and (seen, flagged) == (n_rows, 0)


# ---- argument errors that need a handle --------------------------------------------------------------------------------
def test_library_refuses_bad_calls_on_a_live_handle():
    lib = nat.lib
    h = C.c_void_p()
    nat.check(lib.tdsa_detect_create(0, 64, 2, C.byref(h)))
    try:
        rows = np.zeros((3, 64), dtype=f32)
        rr, sig = np.zeros(3, dtype=dt.ROW_RECORD), np.zeros((3, 64), dtype=dt.SIGNAL_RECORD)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
        assert lib.tdsa_detect_process(h, p(rows), 1, p(rr), p(sig)) == -1 and b"not configured" in lib.tdsa_last_error_string()
        assert lib.tdsa_detect_process_dev(h, None, p(rows), 1, p(rr), p(sig)) == -1
        for args in ((0, 64, 0, 10.0, 1, 0, 3.0, 16), (0, 63, 0, 10.0, 65, 0, 3.0, 16), (0, 63, 0, 10.0, 1, 65, 3.0, 16)):
            assert lib.tdsa_detect_configure(h, *args) == -1, args
        nat.check(lib.tdsa_detect_configure(h, 0, 63, 32, 10.0, 1, 0, 3.0, 16))
        assert lib.tdsa_detect_process(h, None, 1, p(rr), p(sig)) == -1
        assert lib.tdsa_detect_process(h, p(rows), 1, None, p(sig)) == -1
        assert lib.tdsa_detect_process(h, p(rows), 1, p(rr), None) == -1
        assert lib.tdsa_detect_process(h, p(rows), 3, p(rr), p(sig)) == -1 and b"max_host_rows" in lib.tdsa_last_error_string()
        assert lib.tdsa_detect_read_occupancy(h, None, None, None) == -1
        assert lib.tdsa_detect_timer_end(h, None) == -1
        rr[:] = 7
        assert lib.tdsa_detect_process(h, p(rows), 0, p(rr), p(sig)) == 0 and np.all(rr["n_found"] == 7)
        with DeviceBuffer(1024) as buf:
            assert lib.tdsa_detect_process_dev(h, None, buf.at(2), 1, p(rr), p(sig)) == -1
            assert b"aligned" in lib.tdsa_last_error_string()
            assert lib.tdsa_detect_process_dev(h, None, buf.ptr, 0, p(rr), p(sig)) == 0 and np.all(rr["n_found"] == 7)
        seen = C.c_uint64(9)
        nat.check(lib.tdsa_detect_read_occupancy(h, None, C.byref(seen), None))
        assert seen.value == 0
        cnt = C.c_int()
        nat.check(lib.tdsa_device_count(C.byref(cnt)))
        if cnt.value > 1:                                             # a plan on another device is refused
            with SpectrumEngine(64, device=1) as other, DeviceBuffer(1024) as buf:
                assert lib.tdsa_detect_process_dev(h, other._h, buf.ptr, 1, p(rr), p(sig)) == -1
                assert b"different devices" in lib.tdsa_last_error_string()
    finally:
        lib.tdsa_detect_destroy(h)
