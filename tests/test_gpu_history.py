"""The 3-D history views on the MI355X: the run recorded from the reference's RibbonWidget, ThreeD and Surface
(tests/golden/history.npz) bit for bit, and the numpy restatement of tests/history_contract.py for everything else -
batches against single pushes, the ring's wrap, bin counts from 2 to 2^17, the screen reduction, the argmax tie rule on
a plateau, an amplitude change between pushes, device against host destinations, and the three view classes behind a
DataProcessor tick.  Every comparison is np.array_equal on arrays of the same dtype and shape."""
import os
import types

import numpy as np
import pytest

import history_contract as hc
from topdogspectrumanalyser_amd import DataProcessor, DeviceBuffer, RibbonView, SurfaceView, ThreeDView, TraceHistory, _native as nat
from topdogspectrumanalyser_amd.utils.constants import DisplayMode

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "history.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _peak_same(a, b):
    return int(a[0]) == int(b[0]) and _same(np.float32(a[1]), np.float32(b[1]))


def _rows(rng, n_rows, n, plateau=True):
    """float32 dB rows without NaN: noise around -80 dBm, a few bins off the scale on both sides, +-inf, a plateau."""
    rows = (rng.normal(-80.0, 12.0, size=(n_rows, n))).astype(np.float32)
    for r in range(n_rows):
        rows[r, rng.integers(0, n)] = 40.0
        rows[r, rng.integers(0, n)] = -300.0
        if r % 3 == 1:
            rows[r, rng.integers(0, n)] = np.inf
            rows[r, rng.integers(0, n)] = -np.inf
        if plateau and r % 4 == 2 and n >= 8:
            a = int(rng.integers(0, n - n // 4))
            rows[r, a:a + max(n // 4, 2)] = 25.0
    return rows


def _check_ribbon(h, m, x, columns=None, what=""):
    v, w = h.ribbon(x, columns), m.ribbon(x, columns)
    print(f"ribbon {what} n={h.n_bins} depth={h.depth} columns={columns}: verts {v['verts'].shape}, "
          f"differing verts {(v['verts'] != w['verts']).sum()}, colours {(v['colours'] != w['colours']).sum()}")
    assert _same(v["verts"], w["verts"]) and _same(v["colours"], w["colours"])
    if columns is not None:
        assert _same(v["bins"], w["bins"])
    return v


def _check_lines(h, m, columns=None, first=0, count=None, what=""):
    for mode in ("index", "rgba"):
        v, w = h.lines(first, count, mode, columns), m.lines(first, count, columns)
        print(f"lines {what} n={h.n_bins} depth={h.depth} columns={columns} {mode}: z {v['z'].shape}, "
              f"differing z {(v['z'] != w['z']).sum()}, colours {(v[mode] != w[mode]).sum()}, "
              f"peaks {v['live_peak']} / {w['live_peak']}, {v['hold_peak']} / {w['hold_peak']}")
        assert _same(v["z"], w["z"]) and _same(v[mode], w[mode]) and _same(v["hold"], w["hold"])
        assert _peak_same(v["live_peak"], w["live_peak"]) and _peak_same(v["hold_peak"], w["hold_peak"])
        assert (v["min"] is None) == (w["min"] is None)
        if w["min"] is not None:
            assert _same(v["min"], w["min"])
        if columns is not None:
            assert _same(v["bins"], w["bins"]) and _same(v["hold_bins"], w["hold_bins"])
            if w["min"] is not None:
                assert _same(v["min_bins"], w["min_bins"])
    return v


def _check_surface(h, m, columns=None, what=""):
    v, w = h.surface(columns), m.surface(columns)
    print(f"surface {what} n={h.n_bins} depth={h.depth} columns={columns}: z {v['z'].shape}, differing z "
          f"{(v['z'] != w['z']).sum()}, colours {(v['colours'] != w['colours']).sum()}, peak {v['live_peak']} / "
          f"{w['live_peak']}, norm {v['peak_norm']!r} / {w['peak_norm']!r}")
    assert _same(v["z"], w["z"]) and _same(v["colours"], w["colours"])
    assert _peak_same(v["live_peak"], w["live_peak"]) and v["peak_norm"] == w["peak_norm"]
    if columns is not None:
        assert _same(v["bins"], w["bins"])
    return v


# ---------------------------------------------------------------------------------------------------- the recorded run
def test_golden_ribbon_bit_for_bit(g):
    x = g["ribbon_x"]
    with TraceHistory(30, 256, "heights") as h:
        k = 0
        for i, row in enumerate(g["ribbon_rows"]):
            h.set_amplitude(*g["ribbon_amp"][i])
            h.push(row)
            if i in g["ribbon_steps"]:
                v = h.ribbon(x)
                assert _same(v["verts"], g["ribbon_verts"][k]) and _same(v["colours"], g["ribbon_colours"][k]), i
                k += 1
        assert k == len(g["ribbon_steps"])
    assert _same(TraceHistory.ribbon_faces(256), g["ribbon_faces"])


def test_golden_line_stack_bit_for_bit(g):
    L = int(g["lines_depth"])
    with TraceHistory(L, 256, "heights") as h:
        k = 0
        for i, row in enumerate(g["lines_rows"]):
            h.set_amplitude(*g["lines_amp"][i])
            max_on, min_on = bool(g["lines_max_on"][i]), bool(g["lines_min_on"][i])
            if not max_on:
                h.reset_hold()
            h.push(row, g["lines_max_trace"][i] if max_on else None, g["lines_min_trace"][i] if min_on else None, hold=max_on)
            if i in g["lines_steps"]:
                v, c = h.lines(), h.lines(colours="rgba")
                assert _same(v["z"], g["lines_z"][k]) and _same(c["z"], g["lines_z"][k]), i
                assert _same(c["rgba"], g["lines_rgba"][k]), i
                assert _same(hc.line_rgba(v["index"]), g["lines_rgba"][k]), i
                assert _same(v["z"][0][v["live_peak"][0]], np.float32(g["lines_peak"][k][2])), i
                assert float(g["lines_x"][v["live_peak"][0]]) == g["lines_peak"][k][0], i
                if max_on:
                    assert _same(v["hold"], g["lines_hold"][k]), i
                    assert float(g["lines_x"][v["hold_peak"][0]]) == g["lines_max_peak"][k][0], i
                    assert float(v["hold_peak"][1]) == g["lines_max_peak"][k][2], i
                if min_on:
                    assert _same(v["min"], g["lines_min"][k]), i
                else:
                    assert v["min"] is None
                k += 1
        assert k == len(g["lines_steps"])
    assert _same(TraceHistory.line_palette(), hc.line_palette())


def test_golden_surface_bit_for_bit(g):
    with TraceHistory(int(g["surface_depth"]), 256, "levels") as h:
        k = 0
        for i, row in enumerate(g["surface_rows"]):
            h.set_amplitude(*g["surface_amp"][i])
            h.push(row)
            if i in g["surface_steps"]:
                v = h.surface()
                assert _same(v["z"], g["surface_z"][k]), i
                assert _same(v["colours"], hc.surface_colours(g["surface_z"][k])), i
                assert v["peak_norm"] == g["surface_peak"][k][2], i
                k += 1
        assert k == len(g["surface_steps"])


# ---------------------------------------------------------------------------------------------------- pushes
@pytest.mark.parametrize("n,depth,n_rows", [(1000, 30, 17), (1000, 30, 75), (1024, 300, 300), (6, 5, 9)])
def test_a_batch_of_device_rows_equals_single_pushes(n, depth, n_rows):
    rng = np.random.default_rng(n * depth + n_rows)
    rows = _rows(rng, n_rows, n)
    x = np.linspace(-10, 10, n, dtype=np.float32)
    with TraceHistory(depth, n) as a, TraceHistory(depth, n) as b, DeviceBuffer(rows.nbytes) as d:
        m = hc.HistoryModel(depth, n, "heights")
        for h in (a, b, m):
            h.set_amplitude(-10.0, 90.0)
        a.push(rows[0])
        b.push(rows[0])
        m.push(rows[0])
        d.put(rows[1:])
        a.push_rows(None, d.ptr, n_rows - 1)
        for r in rows[1:]:
            b.push(r)
            m.push(r)
        va, vb = _check_lines(a, m, what="batch"), _check_lines(b, m, what="single")
        assert va["pushed"] == vb["pushed"] == n_rows
        _check_ribbon(a, m, x, what="batch")
    with TraceHistory(depth, n, "levels") as a, DeviceBuffer(rows.nbytes) as d:
        m = hc.HistoryModel(depth, n, "levels")
        d.put(rows)
        a.push_rows(None, d.ptr, n_rows)
        m.push_rows(rows)
        _check_surface(a, m, what="batch")


def test_rows_of_an_engine_go_into_the_history_on_its_stream():
    from oracle import spectrum_oracle as so
    from topdogspectrumanalyser_amd import SpectrumEngine

    nfft, nf = 1024, 12
    iq = so.synth_iq_int8(nfft * nf, nfft, seed=5)
    with SpectrumEngine(nfft, max_frames=nf, device=0) as e, TraceHistory(8, nfft) as h, DeviceBuffer(4 * nfft * nf) as d, \
            DeviceBuffer(iq.nbytes) as src:
        e.set_window(so.hackrf_window(nfft))
        e.configure(db_mode="mag", log_floor=so.LOG_FLOOR, dc_alpha=1.0)
        src.put(iq)
        e.process_device(nat.IN_I8, src.ptr, nfft * nf, nfft, nf, d.ptr)
        h.set_amplitude(0.0, 120.0)
        h.push_rows(e, d.ptr, nf)
        v = h.lines()
        e.synchronize()
        rows = d.get((nf, nfft), np.float32)
        m = hc.HistoryModel(8, nfft, "heights")
        m.set_amplitude(0.0, 120.0)
        m.push_rows(rows)
        w = m.lines()
        assert _same(v["z"], w["z"]) and _same(v["index"], w["index"]) and _same(v["hold"], w["hold"])
        assert _peak_same(v["live_peak"], w["live_peak"])


@pytest.mark.parametrize("depth", [1, 2, 30, 300])
def test_the_ring_wraps(depth):
    n = 1000
    rng = np.random.default_rng(depth)
    rows = _rows(rng, 2 * depth + 3, n)
    x = np.linspace(-10, 10, n, dtype=np.float32)
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for i, r in enumerate(rows):
            for t in (h, m, s, ms):
                t.push(r)
            if i in (0, depth - 1, depth, 2 * depth - 1, 2 * depth + 2):
                _check_lines(h, m, what=f"after {i + 1}")
                _check_ribbon(h, m, x, what=f"after {i + 1}")
                _check_surface(s, ms, what=f"after {i + 1}")
        assert h.lines()["valid"] == depth
        if depth >= 2:
            _check_lines(h, m, first=1, count=depth - 1, what="a range")
            _check_lines(h, m, first=0, count=1, what="line 0")
        h.reset()
        m.reset()
        h.push(rows[0])
        m.push(rows[0])
        v = _check_lines(h, m, what="after reset")
        assert v["valid"] == 1 and (h.lines()["index"][1:] == hc.NEVER_PUSHED).all()


@pytest.mark.parametrize("n", [2, 1000, 16384, 1 << 17])
def test_bin_counts_against_the_restatement(n):
    rng = np.random.default_rng(n)
    depth = 30 if n <= 16384 else 6
    rows = _rows(rng, depth + 4, n)
    x = (np.linspace(-10, 10, n) + rng.normal(0, 1e-3, n)).astype(np.float32)
    with TraceHistory(depth, n) as h, TraceHistory(5, n, "levels") as s:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(5, n, "levels")
        for t in (h, m, s, ms):
            t.set_amplitude(-5.0, 85.0)
        for i, r in enumerate(rows):
            mx, mn = np.maximum.reduce(rows[:i + 1]), np.minimum.reduce(rows[:i + 1])
            for t in (h, m):
                t.push(r, mx, mn)
            for t in (s, ms):
                t.push(r)
        _check_ribbon(h, m, x)
        _check_lines(h, m)
        _check_surface(s, ms)


@pytest.mark.parametrize("n,columns", [(16384, 1), (16384, 1024), (16384, 16384), (1000, 7), (1000, 333), (1000, 1000),
                                       (6, 4)])
def test_the_screen_reduction(n, columns):
    rng = np.random.default_rng(n + columns)
    depth = 30
    rows = _rows(rng, depth + 2, n)
    x = np.linspace(-10, 10, n, dtype=np.float32)
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for i, r in enumerate(rows):
            for t in (h, m):
                t.push(r, None, rows[0])
            for t in (s, ms):
                t.push(r)
        _check_ribbon(h, m, x, columns)
        _check_lines(h, m, columns)
        _check_lines(h, m, columns, first=3, count=5)
        _check_surface(s, ms, columns)


def test_a_plateau_reports_its_first_bin():
    n = 16384
    row = np.full(n, -60.0, dtype=np.float32)
    row[5000:9000] = 12.0                          # clipped to z = 8 over 4000 bins
    row[12000] = 30.0                              # a higher level, the same z
    with TraceHistory(4, n) as h, TraceHistory(4, n, "levels") as s:
        h.push(row)
        s.push(row)
        v = h.lines()
        assert v["live_peak"] == (5000, np.float32(8.0)) and v["hold_peak"] == (5000, np.float32(8.0))
        assert int(np.argmax(v["z"][0])) == 5000
        assert s.surface()["live_peak"] == (12000, np.float32(30.0))
        r = h.lines(columns=16)                    # cells of 1024 bins: the plateau starts inside cell 4
        assert r["bins"][0, 4] == 5000 and r["bins"][0, 5] == 5120 and r["bins"][0, 0] == 0
        row2 = np.full(n, -200.0, dtype=np.float32)            # all at the bottom: every bin ties at 0
        h.push(row2)
        s.push(row2)
        assert h.lines()["live_peak"] == (0, np.float32(0.0))
        assert s.surface()["live_peak"] == (0, np.float32(-200.0))


def test_rows_keep_the_amplitude_they_were_pushed_with():
    n = 1000
    rng = np.random.default_rng(77)
    rows = _rows(rng, 12, n)
    amps = [(0.0, 100.0), (-20.0, 60.0), (10.0, 133.3), (-3.7, 0.1)]
    x = np.linspace(-10, 10, n, dtype=np.float32)
    with TraceHistory(30, n) as h, TraceHistory(8, n, "levels") as s:
        m, ms = hc.HistoryModel(30, n, "heights"), hc.HistoryModel(8, n, "levels")
        for i, r in enumerate(rows):
            for t in (h, m, s, ms):
                t.set_amplitude(*amps[i // 3])
                t.push(r)
        _check_ribbon(h, m, x)
        _check_lines(h, m)
        _check_surface(s, ms)
        for t in (s, ms):
            t.set_amplitude(-30.0, 0.0)            # zmax == zmin: 0.5 everywhere
        v = _check_surface(s, ms)
        assert (v["z"] == 0.5).all() and v["peak_norm"] == 0.5


@pytest.mark.parametrize("n,columns", [(1000, None), (16384, 1024), (6, None)])
def test_device_destinations_equal_host_destinations(n, columns):
    rng = np.random.default_rng(n)
    rows = _rows(rng, 9, n)
    x = np.linspace(-10, 10, n, dtype=np.float32)
    P = columns or n
    with TraceHistory(30, n) as h, TraceHistory(7, n, "levels") as s:
        for r in rows:
            h.push(r, None, rows[0])
            s.push(r)
        v = h.ribbon(x, columns)
        with DeviceBuffer(v["verts"].nbytes) as dv, DeviceBuffer(v["colours"].nbytes) as dc, DeviceBuffer(4 * 30 * P) as db:
            h.ribbon(x, columns, device_out=dict(primary=dv.ptr, colours=dc.ptr, bins=db.ptr))
            assert _same(dv.get(v["verts"].shape, np.float32), v["verts"])
            assert _same(dc.get(v["colours"].shape, np.float32), v["colours"])
            if columns:
                assert _same(db.get(v["bins"].shape, np.int32), v["bins"])
        for mode, dt in (("index", np.uint8), ("rgba", np.float32)):
            v = h.lines(2, 20, mode, columns)
            with DeviceBuffer(v["z"].nbytes) as dz, DeviceBuffer(v[mode].nbytes) as dc, DeviceBuffer(4 * P) as dh, DeviceBuffer(4 * P) as dm, \
                    DeviceBuffer(4 * P) as dhb:
                w = h.lines(2, 20, mode, columns, device_out=dict(primary=dz.ptr, colours=dc.ptr, hold=dh.ptr,
                                                                   min_row=dm.ptr, hold_bins=dhb.ptr))
                assert _same(dz.get(v["z"].shape, np.float32), v["z"]) and _same(dc.get(v[mode].shape, dt), v[mode])
                assert _same(dh.get(P, np.float32), v["hold"]) and _same(dm.get(P, np.float32), v["min"])
                if columns:
                    assert _same(dhb.get(P, np.int32), v["hold_bins"])
                assert w["live_peak"] == v["live_peak"] and w["hold_peak"] == v["hold_peak"]
        v = s.surface(columns)
        with DeviceBuffer(v["z"].nbytes) as dz, DeviceBuffer(v["colours"].nbytes) as dc:
            w = s.surface(columns, device_out=dict(primary=dz.ptr, colours=dc.ptr))
            assert _same(dz.get(v["z"].shape, np.float32), v["z"]) and _same(dc.get(v["colours"].shape, np.float32), v["colours"])
            assert w["peak_norm"] == v["peak_norm"]
            with pytest.raises(nat.TdsaError, match="16 bytes"):
                s.surface(columns, device_out=dict(primary=dz.at(4)))


def test_views_refuse_the_wrong_kind_and_bad_ranges():
    with TraceHistory(4, 16) as h, TraceHistory(4, 16, "levels") as s:
        with pytest.raises(nat.TdsaError, match="heights"):
            s.lines()
        with pytest.raises(nat.TdsaError, match="heights"):
            s.ribbon(np.zeros(16, np.float32))
        with pytest.raises(nat.TdsaError, match="levels"):
            h.surface()
        with pytest.raises(nat.TdsaError, match="range_db"):
            h.set_amplitude(0.0, 0.0)
        with pytest.raises(ValueError):
            h.lines(first=3, count=2)
        with pytest.raises(ValueError):
            h.lines(columns=17)
        with pytest.raises(ValueError):
            h.push(np.zeros(15, np.float32))


# ---------------------------------------------------------------------------------------------------- the view classes
def _tick(view, mode, attr, live, mx, fb, mn=None):
    """One DataProcessor timer tick with `view` as the active widget."""
    mw = types.SimpleNamespace(current_stacked_index=mode, live_power_levels=live, max_power_levels=mx,
                               min_power_levels=mn, frequency_bins=fb, is_popped_out=False,
                               marker_manager=types.SimpleNamespace(update=lambda: None),
                               status_label=types.SimpleNamespace(setText=lambda s: pytest.fail(s)))
    setattr(mw, attr, view)
    dp = DataProcessor.__new__(DataProcessor)
    dp.mw = mw
    dp.dm = types.SimpleNamespace(DISPLAY_WIDGETS_MAP={mode: lambda w: getattr(w, attr)})
    dp._spectrum_tick(lambda: None)


def test_view_classes_behind_a_data_processor_tick(g):
    fb = g["freq_bins"]
    rib = RibbonView()
    k = 0
    for i, row in enumerate(g["ribbon_rows"]):
        rib.set_amplitude(*g["ribbon_amp"][i])
        _tick(rib, DisplayMode.RIBBON, "ribbon_widget", (row, row) if i % 2 else row, None, fb)
        if i in g["ribbon_steps"]:
            assert _same(rib.verts, g["ribbon_verts"][k]) and _same(rib.colours, g["ribbon_colours"][k]), i
            k += 1
    assert _same(rib.x, g["ribbon_x"]) and _same(rib.faces, g["ribbon_faces"]) and rib.reinits == 1
    rib.close()

    td = ThreeDView()
    td.set_history_lines(int(g["lines_depth"]))
    td.set_peak_search_enabled(True)
    k = 0
    for i, row in enumerate(g["lines_rows"]):
        td.set_amplitude(*g["lines_amp"][i])
        if bool(g["lines_max_on"][i]) != td.max_peak_search_enabled:
            td.set_max_peak_search_enabled(bool(g["lines_max_on"][i]))
        if bool(g["lines_min_on"][i]) != td.min_hold_enabled:
            td.set_min_hold_enabled(bool(g["lines_min_on"][i]))
        _tick(td, DisplayMode.THREE_D, "three_d_widget", row, g["lines_max_trace"][i], fb, g["lines_min_trace"][i])
        if i in g["lines_steps"]:
            assert _same(td.z, g["lines_z"][k]) and _same(hc.line_rgba(td.index), g["lines_rgba"][k]), i
            assert np.array_equal(np.asarray(td.peak), g["lines_peak"][k]), i
            texts = [td.live_freq_text, td.live_power_text, td.max_freq_text, td.max_power_text]
            assert texts == [str(t) for t in g["lines_texts"][k]], i
            assert np.array_equal(np.asarray(td.max_hold_colour, dtype=np.float64), g["lines_hold_rgba"][k]), i
            assert np.array_equal(np.asarray(td.min_hold_colour, dtype=np.float64), g["lines_min_rgba"][k]), i
            if g["lines_max_on"][i]:
                assert _same(td.max_hold_z, g["lines_hold"][k]), i
                assert np.array_equal(np.asarray(td.max_peak), g["lines_max_peak"][k]), i
            if g["lines_min_on"][i]:
                assert _same(td.min_hold_z, g["lines_min"][k]), i
            k += 1
    assert np.array_equal(td.x, g["lines_x"]) and np.array_equal(td.y, g["lines_y"]) and td.reinits == 1
    td.close()

    sf = SurfaceView()
    sf.set_history_lines(int(g["surface_depth"]))
    sf.set_peak_search_enabled(True)
    k = 0
    for i, row in enumerate(g["surface_rows"]):
        sf.set_amplitude(*g["surface_amp"][i])
        _tick(sf, DisplayMode.SURFACE, "surface_widget", row, None, fb)
        if i in g["surface_steps"]:
            assert _same(sf.z, g["surface_z"][k]), i
            assert np.array_equal(np.asarray(sf.peak), g["surface_peak"][k]), i
            assert [sf.peak_label_text, sf.peak_info_text] == [str(t) for t in g["surface_texts"][k]], i
            k += 1
    assert np.array_equal(sf.x, g["surface_x"]) and np.array_equal(sf.y, g["surface_y"]) and sf.reinits == 1
    # the re-init rule: another end frequency or bin count starts the history again, the same axis does not
    _tick(sf, DisplayMode.SURFACE, "surface_widget", g["surface_rows"][0], None, fb.copy())
    assert sf.reinits == 1
    fb2 = fb.copy()
    fb2[-1] += 1.0
    _tick(sf, DisplayMode.SURFACE, "surface_widget", g["surface_rows"][0], None, fb2)
    assert sf.reinits == 2 and sf.history.surface()["pushed"] == 1
    sf.close()
