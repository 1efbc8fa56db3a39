"""The channel measurements without a device: the numpy contract on planted rows whose figures
are known in closed form, channel_plan against the band power oracle, limit_line against np.interp, record layouts,
the arithmetic of Measurements, and every argument error of the Python layer and of the C-ABI that needs no handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import meas_contract as mc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import measure as ms

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from oracle import analytics_oracle as ao  # noqa: E402

f32 = np.float32


def _result(rr, ch):
    return ms.measurements_from(np.atleast_1d(rr), ch.reshape(np.atleast_1d(rr).shape[0], -1))


# ---- the contract -------------------------------------------------------------------------------------------------------
def test_flat_row_in_closed_form():
    """Every bin 0.0 dB: p = 1, so a channel's power is its width, T the range's width W, and the two edges lie at
    lo - 1/2 + W (1 -+ f) / 2: the occupied bandwidth is W f bins.  At f = 0.5 and W = 1000 every figure is exact."""
    n, lo, hi = 1200, 100, 1099
    row = np.zeros(n, dtype=f32)
    limit = np.full(n, 0.0, dtype=f32)
    rr, ch = mc.measure_row(row, [(0, n - 1), (5, 5), (100, 163)], (lo, hi), 0.5, 3.0, limit)
    assert list(ch["power"]) == [n, 1.0, 64.0] and list(ch["peak_bin"]) == [0, 5, 100] and not ch["n_nan"].any()
    assert np.all(ch["peak_db"] == 0.0)
    assert rr["obw_total"] == 1000.0 and (rr["x_lo"], rr["x_hi"]) == (lo - 0.5 + 250.0, lo - 0.5 + 750.0)
    assert (rr["k_lo"], rr["k_hi"]) == (lo + 249, lo + 749)             # S[k] = k - lo + 1 reaches 250 at lo + 249
    assert (rr["xdb_lo"], rr["xdb_hi"], rr["peak_bin"], rr["peak_db"]) == (lo, hi, lo, 0.0)
    assert (rr["n_fail"], rr["first_fail"], rr["last_fail"], rr["flags"]) == (0, -1, -1, 0)
    assert (rr["worst_bin"], rr["worst_margin"]) == (0, 0.0)            # on the line is not above it
    for f in (0.9, 0.99, 0.999):
        rr, _ = mc.measure_row(row, [(0, 0)], (lo, hi), f, 0.0)
        assert abs((rr["x_hi"] - rr["x_lo"]) - 1000.0 * f) <= 1e-9
        assert abs(0.5 * (rr["x_hi"] + rr["x_lo"]) - 0.5 * (lo + hi)) <= 1e-9
    rr, _ = mc.measure_row(row, [(0, 0)], (lo, hi), 0.5, 0.0, limit - f32(1.0))
    assert (rr["n_fail"], rr["first_fail"], rr["last_fail"], rr["flags"]) == (n, 0, n - 1, mc.FLAG_MASK_FAIL)
    assert (rr["worst_bin"], rr["worst_margin"]) == (0, 1.0)


def test_raised_cosine_width_from_its_own_cumulative_sum():
    """The 99 % edges of a raised-cosine emission, against the positions read off the cumulative sum of its float64
    powers.  The row holds those powers rounded to float32 dB, an error of POWER_RTOL T at most in any partial sum: a
    position moves by no more than that over the power of the bin it lies in."""
    centre, half = 1000, 200
    row, shape = mc.raised_cosine_row(2048, centre, half)
    rr, ch = mc.measure_row(row, [(centre - half, centre + half)], (0, 2047), 0.99, 26.0)
    S = np.cumsum(shape)
    T = S[-1]
    edges = centre - half - 0.5 + np.arange(S.size + 1)
    for x, k, t in ((rr["x_lo"], rr["k_lo"], 0.005 * T), (rr["x_hi"], rr["k_hi"], 0.995 * T)):
        want = np.interp(t, np.concatenate(([0.0], S)), edges)
        tol = 2 * mc.POWER_RTOL * T / shape[int(k) - (centre - half)]
        assert tol < 0.05 and abs(x - want) <= tol and k - 0.5 <= x <= k + 0.5
    assert abs(rr["obw_total"] - T) <= mc.POWER_RTOL * T and abs(ch["power"][0] - T) <= mc.POWER_RTOL * T
    assert abs(0.5 * (rr["x_lo"] + rr["x_hi"]) - centre) <= 1e-3        # symmetric
    assert (rr["peak_bin"], rr["flags"]) == (centre, 0)
    down = 10.0 * np.log10(shape / shape.max())
    assert np.min(np.abs(down + 26.0)) > 1e-3                           # no bin close enough to the edge for rounding to matter
    k26 = np.flatnonzero(down >= -26.0)
    assert (rr["xdb_lo"], rr["xdb_hi"]) == (centre - half + k26[0], centre - half + k26[-1])


def test_acpr_set_by_construction():
    main, adj = (400, 499), ((300, 399), (500, 599), (200, 299), (600, 699))
    row = mc.acpr_row(1024, main, adj[:2], -20.0, -40.0)
    rr, ch = mc.measure_row(row, [main] + list(adj), (0, 1023), 0.99, 3.0)
    m = _result(rr, ch)
    acpr = m.acpr_db()[0]
    assert acpr[0] == 0.0 and np.all(np.abs(acpr[1:3] + 40.0) <= 1e-5) and np.all(acpr[3:] < -150.0)
    assert abs(m.channel_power_db(1000.0)[0, 0] - (-20.0 + 10 * np.log10(100 * 1000.0))) <= 1e-5
    assert (rr["xdb_lo"], rr["xdb_hi"]) == main and 399.5 < rr["x_lo"] < 400.5 < 498.5 < rr["x_hi"] < 499.5
    # a mask relative to the main channel's peak: -30 dBc outside it fails nowhere, -45 dBc in both adjacent channels
    limit = np.full(1024, -30.0, dtype=f32)
    limit[main[0]:main[1] + 1] = np.nan
    rr, _ = mc.measure_row(row, [main], (0, 1023), 0.99, 3.0, limit, relative=True)
    assert (rr["n_fail"], rr["flags"], rr["worst_bin"], rr["worst_margin"]) == (0, 0, 300, -10.0)
    limit[~np.isnan(limit)] = -45.0
    rr, _ = mc.measure_row(row, [main], (0, 1023), 0.99, 3.0, limit, relative=True)
    assert (rr["n_fail"], rr["first_fail"], rr["last_fail"], rr["flags"]) == (200, 300, 599, mc.FLAG_MASK_FAIL)
    assert rr["worst_margin"] == 5.0


def test_contract_flags_nans_and_empty_ranges():
    row = np.full(64, np.nan, dtype=f32)
    rr, ch = mc.measure_row(row, [(0, 63)], (0, 63), 0.5, 3.0, np.zeros(64, dtype=f32))
    assert rr["flags"] == mc.FLAG_EMPTY and (rr["k_lo"], rr["k_hi"], rr["peak_bin"], rr["xdb_lo"], rr["xdb_hi"]) == (-1,) * 5
    assert np.isnan(rr["x_lo"]) and np.isnan(rr["peak_db"]) and np.isnan(rr["worst_margin"]) and rr["n_nan"] == 64
    assert (ch["power"][0], ch["peak_bin"][0], ch["n_nan"][0]) == (0.0, -1, 64) and np.isnan(ch["peak_db"][0])
    row[:] = -np.inf
    rr, ch = mc.measure_row(row, [(0, 63)], (0, 63), 0.5, 3.0)
    assert rr["flags"] == mc.FLAG_EMPTY and rr["peak_bin"] == 0 and (rr["xdb_lo"], rr["xdb_hi"]) == (0, 63)
    row[10] = np.inf
    rr, ch = mc.measure_row(row, [(0, 63)], (0, 63), 0.5, 3.0)
    assert rr["flags"] == mc.FLAG_INF and rr["k_lo"] == -1 and np.isinf(rr["obw_total"]) and rr["peak_bin"] == 10
    # relative to a NaN reference nothing is tested
    row = np.zeros(64, dtype=f32)
    row[:8] = np.nan
    rr, _ = mc.measure_row(row, [(0, 7), (0, 63)], (0, 63), 0.5, 3.0, np.full(64, -100.0, dtype=f32), relative=True)
    assert (rr["n_fail"], rr["worst_bin"], rr["flags"]) == (0, -1, 0) and np.isnan(rr["worst_margin"])


def test_crossings_on_a_bins_upper_edge_and_over_zero_power_bins():
    """p in {1, 0}: the sums are exact.  A target that S reaches exactly belongs to the bin that reaches it (x on its
    upper edge), and zero-power bins behind it are not the crossing."""
    row = np.full(32, -np.inf, dtype=f32)
    row[[2, 3, 10, 11, 20, 21, 30, 31]] = 0.0                            # T = 8: t_lo = 2, t_hi = 6 at f = 0.5
    rr, _ = mc.measure_row(row, [(0, 31)], (0, 31), 0.5, 0.0)
    assert (rr["k_lo"], rr["x_lo"], rr["k_hi"], rr["x_hi"], rr["obw_total"]) == (3, 3.5, 21, 21.5, 8.0)
    row[[2, 3]] = np.nan                                                 # T = 6: t_lo = 1.5, t_hi = 4.5
    rr, _ = mc.measure_row(row, [(0, 31)], (0, 31), 0.5, 0.0)
    assert (rr["k_lo"], rr["x_lo"], rr["k_hi"], rr["x_hi"], rr["n_nan"]) == (11, 11.0, 30, 30.0, 2)


# ---- the helpers --------------------------------------------------------------------------------------------------------
def test_channel_plan_against_the_band_power_oracle():
    n = 2001
    freq = np.linspace(90e6, 110e6, n)
    rng = np.random.default_rng(3)
    row = (-90.0 + 3.0 * rng.standard_normal(n)).astype(f32)
    plan = ms.channel_plan(freq, 100e6, 1e6, 1.25e6, n_adjacent=2)
    centres = [100e6, 98.75e6, 101.25e6, 97.5e6, 102.5e6]                # main, lower 1, upper 1, lower 2, upper 2
    assert len(plan) == 5
    rr, ch = mc.measure_row(row, plan, (0, n - 1), 0.99, 26.0)
    got = _result(rr, ch).channel_power_db((freq[-1] - freq[0]) / (n - 1))[0]
    for (lo, hi), c, db in zip(plan, centres, got):
        assert (lo, hi) == ao.band_bin_range(freq, c - 0.5e6, c + 0.5e6)
        assert abs(db - ao.band_power_db(freq, row.astype(np.float64), c - 0.5e6, c + 0.5e6)) <= 1e-4
    assert ms.channel_plan(freq, 100e6, 1e6) == plan[:1]
    assert ms.channel_plan(freq, 100e6, 1e6, None, 1) == ms.channel_plan(freq, 100e6, 1e6, 1e6, 1)
    for args in ((100e6, 0.0), (100e6, -1.0), (100e6, float("nan")), (float("inf"), 1e6), (100e6, 1e6, 0.0),
                 (100e6, 1e6, 1e6, -1), (100e6, 1e6, 1e6, 8),
                 (90.2e6, 1e6),                                           # leaves the row below
                 (100e6, 1e6, 5e6, 2),                                    # the second adjacent pair leaves it
                 (100.005e6, 1e3)):                                       # between two bins: no bin
        with pytest.raises(ValueError):
            ms.channel_plan(freq, *args)
    with pytest.raises(ValueError):
        ms.channel_plan(np.zeros((2, 2)), 0.0, 1.0)


def test_limit_line_against_np_interp():
    freq = np.linspace(90e6, 110e6, 801)
    pts = [(-4e6, -60.0), (-1.5e6, -40.0), (-0.5e6, -20.0), (0.5e6, -20.0), (1.5e6, -40.0), (4e6, -60.0)]
    line = ms.limit_line(freq, pts, centre_hz=100e6)
    x = freq - 100e6
    inside = (x >= -4e6) & (x <= 4e6)
    want = np.interp(x, [p[0] for p in pts], [p[1] for p in pts]).astype(f32)
    assert line.dtype == f32 and line.shape == (801,)
    assert np.array_equal(line[inside], want[inside]) and np.all(np.isnan(line[~inside])) and inside.sum() == 321
    assert np.array_equal(ms.limit_line(freq - 100e6, pts), line, equal_nan=True)
    for bad in ([], [(0.0, 1.0, 2.0)], [(1.0, 0.0), (0.0, 0.0)], [(float("nan"), 0.0)]):
        with pytest.raises(ValueError):
            ms.limit_line(freq, bad)


def test_channels_from_emission():
    freq = np.linspace(0.0, 1000.0, 1001)
    em = np.zeros((), dtype=[("centre_hz", "<f8"), ("bandwidth_hz", "<f8")])
    em["centre_hz"], em["bandwidth_hz"] = 500.0, 20.0
    assert ms.channels_from_emission(em, freq, n_adjacent=1) == [(490, 510), (470, 490), (510, 530)]
    assert ms.channels_from_emission(em, freq, spacing_hz=30.0, n_adjacent=1, bandwidth_hz=10.0) == \
        [(495, 505), (465, 475), (525, 535)]


# ---- records and Measurements -------------------------------------------------------------------------------------------
def test_record_layouts():
    assert mc.ROW.itemsize == ms.ROW_RECORD.itemsize == 80 and mc.CHANNEL.itemsize == ms.CHANNEL_RECORD.itemsize == 24
    assert [ms.ROW_RECORD.fields[f][1] for f in ms.ROW_RECORD.names] == [0, 8, 16] + list(range(24, 68, 4)) + [68, 72, 76]
    assert [ms.CHANNEL_RECORD.fields[f][1] for f in ms.CHANNEL_RECORD.names] == [0, 8, 12, 16, 20]
    assert mc.ROW.descr == ms.ROW_RECORD.descr and mc.CHANNEL.descr == ms.CHANNEL_RECORD.descr
    assert ms.ROW_RECORD.names[3:14] == ("k_lo", "k_hi", "xdb_lo", "xdb_hi", "peak_bin", "n_nan", "n_fail", "worst_bin",
                                         "first_fail", "last_fail", "flags")
    assert (ms.FLAG_EMPTY, ms.FLAG_INF, ms.FLAG_MASK_FAIL) == (mc.FLAG_EMPTY, mc.FLAG_INF, mc.FLAG_MASK_FAIL) == (1, 2, 4)
    assert (ms.MAX_BINS, ms.MAX_CHANNELS) == (mc.MAX_BINS, mc.MAX_CHANNELS) == (16384, 16)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tdsa_hip.h")).read()
    assert "tdsa_meas_row" in hdr and "tdsa_meas_channel" in hdr and "#define TDSA_MEAS_MASK_FAIL 4" in hdr


def test_measurements_arithmetic():
    rr = np.zeros(2, dtype=ms.ROW_RECORD)
    ch = np.zeros((2, 3), dtype=ms.CHANNEL_RECORD)
    ch["power"] = [[1.0, 0.01, 1e-4], [2.0, 2.0, 0.0]]
    rr["x_lo"], rr["x_hi"], rr["k_hi"] = [9.5, np.nan], [29.5, np.nan], [29, -1]
    rr["xdb_lo"], rr["xdb_hi"] = [10, -1], [19, -1]
    rr["flags"] = [0, ms.FLAG_MASK_FAIL | ms.FLAG_EMPTY]
    m = ms.measurements_from(rr, ch)
    assert len(m) == 2 and list(m.mask_failed) == [False, True] and m.channels.shape == (2, 3)
    assert np.allclose(m.acpr_db()[0], [0.0, -20.0, -40.0], atol=1e-12) and m.acpr_db()[1, 1] == 0.0
    assert m.acpr_db()[1, 2] < -2900.0                                  # no power: far down, not NaN
    assert np.allclose(m.channel_power_db(100.0), [[20.0, 0.0, -20.0], [10 * np.log10(200.0)] * 2 + [-300.0]], atol=1e-9)
    freq = 1000.0 + 10.0 * np.arange(64)
    assert m.obw_hz(freq, 0) == (200.0, 1000.0 + 19.5 * 10.0) and all(np.isnan(m.obw_hz(freq, 1)))
    assert m.xdb_hz(freq, 0) == (100.0, 1000.0 + 14.5 * 10.0) and all(np.isnan(m.xdb_hz(freq, 1)))
    for call in (lambda: m.obw_hz(freq[:20], 0), lambda: m.xdb_hz(freq[:19], 0), lambda: m.obw_hz(freq.reshape(8, 8), 0)):
        with pytest.raises(ValueError):
            call()
    assert m.k_hi is not rr["k_hi"] and m.rows is rr                     # the fields are copies, the records the library's


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_python_layer_raises_before_the_library_is_called(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")
    monkeypatch.setattr(nat.lib, "tdsa_meas_create", boom, raising=False)
    ok = [(0, 63)]
    for n, ch, kw in ((0, ok, {}), (16385, ok, {}), (64, [], {}), (64, [(0, 1)] * 17, {}), (64, [(-1, 5)], {}),
                      (64, [(5, 4)], {}), (64, [(0, 64)], {}), (64, [(0, 63), (3,)], {}), (64, 5, {}),
                      (64, ok, dict(obw=(-1, 5))), (64, ok, dict(obw=(5, 4))), (64, ok, dict(obw=(0, 64))),
                      (64, ok, dict(fraction=0.0)), (64, ok, dict(fraction=1.0)), (64, ok, dict(fraction=float("nan"))),
                      (64, ok, dict(fraction=-0.5)), (64, ok, dict(xdb=-1.0)), (64, ok, dict(xdb=float("nan"))),
                      (64, ok, dict(xdb=float("inf"))), (64, ok, dict(limit=np.zeros(63, np.float32))),
                      (64, ok, dict(limit=np.zeros((1, 64), np.float32))), (64, ok, dict(limit=np.zeros(64, np.complex64))),
                      (64, ok, dict(max_host_rows=0))):
        with pytest.raises(ValueError):
            ms.ChannelMeasure(n, ch, **kw)


def test_calls_are_checked_before_the_library_is_called():
    d = object.__new__(ms.ChannelMeasure)                  # no device: the checks need the configuration only
    d.n_bins, d.max_host_rows, d.channels, d.obw, d.fraction, d.xdb, d.device, d._h = 64, 4, [(0, 63)], (0, 63), 0.99, 26.0, 0, None
    for call in (lambda: d.process(np.zeros((2, 63), np.float32)), lambda: d.process(np.zeros((2, 2, 64), np.float32)),
                 lambda: d.process(np.zeros((5, 64), np.float32)), lambda: d.process(np.zeros((1, 64), np.complex64)),
                 lambda: d.process_device(None, 0, 1), lambda: d.process_device(None, 258, 1),
                 lambda: d.process_device(None, 256, -1), lambda: d.configure(channels=[(0, 64)]),
                 lambda: d.configure(fraction=1.5), lambda: d.configure(obw=(3, 2)), lambda: d.configure(xdb=-0.1),
                 lambda: d.set_limit(np.zeros(65, np.float32)), lambda: d.set_limit("line")):
        with pytest.raises(ValueError):
            call()


def test_library_refuses_bad_arguments_without_touching_a_device():
    lib = nat.lib
    ints = lambda *v: (C.c_int * len(v))(*v)                            # noqa: E731
    good = (1, ints(0), ints(63), 0, 63, 0.99, 26.0)
    bad = [(0, ints(0), ints(63), 0, 63, 0.99, 26.0), (17, ints(*[0] * 17), ints(*[1] * 17), 0, 63, 0.99, 26.0),
           (1, None, ints(63), 0, 63, 0.99, 26.0), (1, ints(0), None, 0, 63, 0.99, 26.0),
           (1, ints(-1), ints(63), 0, 63, 0.99, 26.0), (1, ints(5), ints(4), 0, 63, 0.99, 26.0),
           (2, ints(0, 0), ints(63, 16384), 0, 63, 0.99, 26.0), (1, ints(0), ints(63), -1, 63, 0.99, 26.0),
           (1, ints(0), ints(63), 5, 4, 0.99, 26.0), (1, ints(0), ints(63), 0, 16384, 0.99, 26.0),
           (1, ints(0), ints(63), 0, 63, 0.0, 26.0), (1, ints(0), ints(63), 0, 63, 1.0, 26.0),
           (1, ints(0), ints(63), 0, 63, float("nan"), 26.0), (1, ints(0), ints(63), 0, 63, float("inf"), 26.0),
           (1, ints(0), ints(63), 0, 63, 0.99, -0.5), (1, ints(0), ints(63), 0, 63, 0.99, float("nan")),
           (1, ints(0), ints(63), 0, 63, 0.99, float("inf"))]
    for args in bad:
        assert lib.tdsa_meas_configure(None, *args) == -1, args
        assert b"null" not in lib.tdsa_last_error_string(), args        # the argument was refused, not the handle
    assert lib.tdsa_meas_configure(None, *good) == -1 and b"null" in lib.tdsa_last_error_string()
    h = C.c_void_p()
    assert lib.tdsa_meas_create(0, 64, 1, None) == -1
    for n_bins, rows in ((0, 1), (-5, 1), (16385, 1), (64, 0)):
        assert lib.tdsa_meas_create(0, n_bins, rows, C.byref(h)) == -1 and not h.value
        assert b"n_bins" in lib.tdsa_last_error_string() or b"max_host_rows" in lib.tdsa_last_error_string()
    buf = (C.c_ubyte * 256)()
    assert lib.tdsa_meas_set_limit(None, buf, 64, 2) == -1 and b"relative" in lib.tdsa_last_error_string()
    assert lib.tdsa_meas_set_limit(None, buf, 64, 0) == -1 and b"null" in lib.tdsa_last_error_string()
    assert lib.tdsa_meas_process(None, buf, 1, buf, buf) == -1
    assert lib.tdsa_meas_process_dev(None, None, buf, 1, buf, buf) == -1
    assert lib.tdsa_meas_read_totals(None, None, None) == -1
    assert lib.tdsa_meas_reset(None) == -1
    assert lib.tdsa_meas_timer_begin(None) == -1 and lib.tdsa_meas_timer_end(None, None) == -1
    assert lib.tdsa_meas_destroy(None) == 0
