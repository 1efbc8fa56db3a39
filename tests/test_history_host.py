"""3-D history views, host side (no GPU): the numpy restatement in tests/history_contract.py reproduces every array the
reference's RibbonWidget, ThreeD and Surface handed their GL items in the recorded run (tests/golden/history.npz) with
np.array_equal; the screen reduction agrees with a brute-force loop; the view classes keep the reference's re-init rule
and read-out strings; the C-ABI refuses bad arguments before it touches a device; and without a GPU the handles report
an error instead of falling back."""
import ctypes as C
import os

import numpy as np
import pytest

import history_cases as cases
import history_contract as hc
from topdogspectrumanalyser_amd import RibbonView, SurfaceView, ThreeDView, TraceHistory, _native as nat, history3d

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "history.npz")
ERR_ARG = -1
NO_GPU = not os.path.exists("/dev/kfd")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- the recorded run
def test_the_fixture_is_data_of_the_agreed_shape(g):
    assert os.path.getsize(GOLDEN) <= 1 << 20
    assert g["ribbon_rows"].shape == (40, 256) and g["lines_rows"].shape == (20, 256) and g["surface_rows"].shape == (16, 256)
    assert int(g["lines_depth"]) == 12 and int(g["surface_depth"]) == 10
    for k in ("ribbon_rows", "lines_rows", "surface_rows"):
        rows = g[k]
        assert rows.dtype == np.float32 and not np.isnan(rows).any()
        assert np.isposinf(rows).any() and np.isneginf(rows).any()            # +-inf are inside the contract
        assert (rows > 0).any() and (rows < -110).any()                       # above and below the scale
    assert len(np.unique(g["ribbon_amp"], axis=0)) == 2 and len(np.unique(g["lines_amp"], axis=0)) == 2
    assert g["lines_max_on"].any() and not g["lines_max_on"].all() and g["lines_min_on"].any()
    assert (g["ribbon_verts"][-1][:, 0::2, 2] == np.float32(8)).sum() > 40    # a saturated run


def test_contract_reproduces_the_recorded_ribbon(g):
    m = hc.HistoryModel(30, 256, "heights")
    x = hc.ribbon_x(g["freq_bins"])
    assert _same(x, g["ribbon_x"]) and _same(hc.ribbon_faces(256), g["ribbon_faces"])
    assert _same(history3d.ribbon_faces(256), g["ribbon_faces"])
    k = 0
    for i, row in enumerate(g["ribbon_rows"]):
        m.set_amplitude(*g["ribbon_amp"][i])
        m.push(row)
        if i in g["ribbon_steps"]:
            v = m.ribbon(x)
            assert _same(v["verts"], g["ribbon_verts"][k]), i              # x, y_front / y_back and z of every vertex
            assert _same(v["colours"], g["ribbon_colours"][k]), i          # RGB and alpha of every vertex
            k += 1
    assert k == 3 and m.pushed == 40                                      # the 30-row history wrapped


def test_contract_reproduces_the_recorded_line_stack(g):
    L = int(g["lines_depth"])
    m = hc.HistoryModel(L, 256, "heights")
    assert np.array_equal(hc.line_x(g["freq_bins"]), g["lines_x"])
    assert _same(history3d.line_palette(), hc.line_palette())
    k = 0
    for i, row in enumerate(g["lines_rows"]):
        m.set_amplitude(*g["lines_amp"][i])
        max_on, min_on = bool(g["lines_max_on"][i]), bool(g["lines_min_on"][i])
        if not max_on:
            m.reset_hold()                                                 # set_max_peak_search_enabled(False)
        m.push(row, g["lines_max_trace"][i], g["lines_min_trace"][i] if min_on else None, hold=max_on)
        if i not in g["lines_steps"]:
            continue
        v = m.lines()
        assert _same(v["z"], g["lines_z"][k]), i
        assert v["index"].dtype == np.uint8 and _same(v["rgba"], g["lines_rgba"][k]), i        # index through the palette
        assert set(np.unique(v["index"])) <= set(range(hc.LINE_HUES)) | {hc.NEVER_PUSHED}
        li, lz = v["live_peak"]
        y0 = float(g["lines_y"][0])
        assert np.array_equal([float(g["lines_x"][li]), y0, float(lz)], g["lines_peak"][k]), i
        texts = [hc.format_freq_hz(float(g["freq_bins"][li])), f"{float(row[li]):.1f} dBm", "", ""]
        if max_on:
            assert _same(v["hold"], g["lines_hold"][k]), i
            assert np.array_equal(g["lines_hold_rgba"][k], hc.MAX_HOLD_COLOUR)
            mi, mz = v["hold_peak"]
            assert np.array_equal([float(g["lines_x"][mi]), y0, float(mz)], g["lines_max_peak"][k]), i
            texts[2:] = [hc.format_freq_hz(float(g["freq_bins"][mi])), f"{float(g['lines_max_trace'][i][mi]):.1f} dBm"]
        else:
            assert not g["lines_hold_rgba"][k].any()
        if min_on:
            assert _same(v["min"], g["lines_min"][k]) and np.array_equal(g["lines_min_rgba"][k], hc.MIN_HOLD_COLOUR), i
        else:
            assert v["min"] is None and not g["lines_min_rgba"][k].any()
        assert texts == [str(t) for t in g["lines_texts"][k]], i
        k += 1
    assert k == len(g["lines_steps"]) == 6


def test_contract_reproduces_the_recorded_surface(g):
    m = hc.HistoryModel(int(g["surface_depth"]), 256, "levels")
    fb = g["freq_bins"] * 1e-6
    k = 0
    for i, row in enumerate(g["surface_rows"]):
        m.set_amplitude(*g["surface_amp"][i])
        m.push(row)
        if i not in g["surface_steps"]:
            continue
        v = m.surface()
        assert v["z"].dtype == np.float32 and _same(v["z"], g["surface_z"][k]), i     # float32(reference)
        b, level = v["live_peak"]
        nx = (fb[b] - fb[0]) / (fb[-1] - fb[0])
        assert np.array_equal([nx, 0.0, v["peak_norm"]], g["surface_peak"][k]), i
        assert ["Live peak", f"{hc.format_freq_mhz(fb[b])}\n{level:.1f} dBm"] == [str(t) for t in g["surface_texts"][k]], i
        assert _same(v["colours"][..., 0], v["z"]) and not v["colours"][..., 1].any()
        assert _same(v["colours"][..., 2], np.float32(1) - v["z"])
        k += 1
    assert k == 5
    assert (g["surface_z"][-1] == 0.5).all()                               # zmax == zmin on the last step


def test_heights_are_float32_operation_by_operation():
    row = np.array([-33.3, -100.0, 0.0, 1e-3, -np.inf, np.inf, -99.99999], dtype=np.float32)
    z = hc.heights(row, -10.0, 90.0)
    want = np.clip((row - np.float32(-100.0)) / np.float32(90.0) * np.float32(8), 0, 8)
    assert z.dtype == np.float32 and _same(z, want.astype(np.float32))
    z64 = np.clip((row.astype(np.float64) + 100.0) / 90.0 * 8, 0, 8)
    assert np.abs(z - z64).max() <= 8 * 2.0 ** -22                          # and close to the exact value
    assert _same(hc.line_index(np.array([0, 0.5, 1, 7.99, 8], np.float32)), np.array([8, 7, 7, 0, 0], np.uint8))


# ---------------------------------------------------------------------------------------------------- the reduction
@pytest.mark.parametrize("n,P", [(256, 64), (256, 256), (256, 1), (1000, 7), (1000, 333), (17, 16), (2, 2)])
def test_reduction_against_a_brute_force_loop(n, P):
    rng = np.random.default_rng(n * 1000 + P)
    rows = rng.normal(0, 1, (5, n)).astype(np.float32)
    rows[1, : n // 2] = 3.0                                                # ties: the first bin wins
    rows[2, rng.integers(0, n)] = -np.inf
    vals, bins = hc.reduce_columns(rows, P)
    assert vals.dtype == np.float32 and bins.dtype == np.int32 and vals.shape == bins.shape == (5, P)
    cells = hc.cells(n, P)
    assert cells[0][0] == 0 and cells[-1][1] == n and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(cells, cells[1:]))
    for r in range(5):
        for c, (a, b) in enumerate(cells):
            best, at = None, None
            for j in range(a, b):
                if best is None or rows[r, j] > best:
                    best, at = rows[r, j], j
            assert (vals[r, c], bins[r, c]) == (best, at), (r, c)
    m = hc.HistoryModel(5, n, "heights")
    m.push_rows(rows * 10 - 50)
    v = m.lines(columns=P)
    assert _same(v["index"], hc.line_index(v["z"])) and v["z"].shape == (5, P)      # colours follow the reduced value
    x = np.linspace(-10, 10, n, dtype=np.float32)
    rb = m.ribbon(x, P)
    assert rb["verts"].shape == (5, 2 * P, 3) and _same(rb["verts"][:, 0::2, 0], x[rb["bins"]])


# ---------------------------------------------------------------------------------------------------- the view classes
def test_view_classes_keep_the_reinit_rule_and_the_axes(g):
    class Ring:
        made = 0

        def __init__(self, depth, n_bins, kind="heights", device=0):
            Ring.made += 1
            self.depth, self.n_bins, self.kind, self.rows, self.amp = depth, n_bins, kind, 0, None

        def set_amplitude(self, *a):
            self.amp = a

        def push(self, *a, **k):
            self.rows += 1

        def reset(self):
            self.rows = 0

        def reset_hold(self):
            pass

        def close(self):
            pass

        def ribbon(self, x, columns=None):
            return dict(verts=None, colours=None, bins=None)

        def lines(self, **k):
            return dict(z=None, index=None, bins=None, hold=None, min=None, live_peak=(3, np.float32(2.0)),
                        hold_peak=(5, np.float32(4.0)))

        def surface(self, columns=None):
            return dict(z=None, colours=None, bins=None, live_peak=(3, np.float32(-31.26)), peak_norm=0.25)

    fb = g["freq_bins"]
    row = g["lines_rows"][0]
    real, history3d.TraceHistory = history3d.TraceHistory, Ring
    try:
        for cls, depth, kind in ((RibbonView, 30, "heights"), (ThreeDView, 300, "heights"), (SurfaceView, 100, "levels")):
            v = cls()
            assert v.isVisible() and v.history is None
            v.set_amplitude(-20.0, 70.0)
            v.update_widget_data(None, None, fb)
            assert v.history is None
            v.update_widget_data((row, row), None, fb)                     # the audio source's (left, right)
            h = v.history
            assert (h.depth, h.n_bins, h.kind, h.rows, h.amp) == (depth, 256, kind, 1, (-20.0, 70.0))
            v.update_widget_data(row, None, fb.copy())
            assert v.history is h and h.rows == 2                          # the same axis: the history goes on
            moved = fb.copy()
            moved[0] -= 1.0
            v.update_widget_data(row, None, moved)
            if cls is RibbonView:                                          # the ribbon keeps its heights, x moves
                assert v.history is h and h.rows == 3 and _same(v.x, hc.ribbon_x(moved))
            else:
                assert v.history is not h and v.history.rows == 1
            v.update_widget_data(row[:128], None, fb[:128])
            assert v.history.n_bins == 128 and v.history.rows == 1
            for name in ("update_frequency_bins", "set_amplitude", "set_peak_search_enabled", "set_max_peak_search_enabled",
                         "set_min_hold_enabled", "set_log_freq", "isVisible", "update_widget_data"):
                assert callable(getattr(v, name)), name
        assert callable(ThreeDView().set_history_lines) and callable(SurfaceView().set_history_lines)

        r = RibbonView()
        r.update_widget_data(row, None, fb)
        assert _same(r.x, g["ribbon_x"]) and _same(r.faces, g["ribbon_faces"])

        t = ThreeDView()
        t.set_history_lines(12)
        t.set_peak_search_enabled(True)
        t.set_max_peak_search_enabled(True)
        t.update_widget_data(row, g["lines_max_trace"][3], fb)
        assert t.history.depth == 12 and np.array_equal(t.x, g["lines_x"]) and np.array_equal(t.y, g["lines_y"])
        assert t.peak == (float(g["lines_x"][3]), 10.0, 2.0) and t.max_peak == (float(g["lines_x"][5]), 10.0, 4.0)
        assert t.live_freq_text == hc.format_freq_hz(float(fb[3])) == "99.024 MHz"
        assert t.live_power_text == f"{float(row[3]):.1f} dBm" and t.max_power_text == f"{float(g['lines_max_trace'][3][5]):.1f} dBm"
        assert t.max_hold_colour == hc.MAX_HOLD_COLOUR and t.min_hold_colour == (0, 0, 0, 0)
        t.set_log_freq(True)
        assert np.array_equal(t.x, hc.line_x(fb, True)) and t.history.rows == 0
        t.set_history_lines(7)
        assert t.history.depth == 7 and len(t.y) == 7
        t.set_peak_search_enabled(False)
        assert t.peak is None and t.live_freq_text == ""

        s = SurfaceView()
        s.set_history_lines(10)
        s.set_peak_search_enabled(True)
        s.update_widget_data(row, None, fb)
        assert s.history.depth == 10 and np.array_equal(s.x, g["surface_x"]) and np.array_equal(s.y, g["surface_y"])
        mhz = fb * 1e-6
        assert s.peak == (float((mhz[3] - mhz[0]) / (mhz[-1] - mhz[0])), 0.0, 0.25)
        assert (s.peak_label_text, s.peak_info_text) == ("Live peak", "99.024 MHz\n-31.3 dBm")
        s.update_widget_data(row, None, np.array([1.0, np.nan, 3.0]))        # refused, as the widget refuses it
        assert s.history.n_bins == 256
    finally:
        history3d.TraceHistory = real
    assert [hc.format_freq_hz(f) for f in (2.4e9, 99.5e6, 1500.0, 12.34)] == ["2.400 GHz", "99.500 MHz", "1.500 kHz", "12.3 Hz"]
    assert [hc.format_freq_mhz(f) for f in (99.5, 0.0015, 0.00001234)] == ["99.500 MHz", "1.500 kHz", "12.3 Hz"]
    assert history3d._format_freq_hz(99.5e6) == "99.500 MHz" and history3d._format_freq_mhz(0.0015) == "1.500 kHz"


# ---------------------------------------------------------------------------------------------------- the C-ABI
def test_struct_sizes():
    assert C.sizeof(nat.HistoryInfo) == 48 and C.sizeof(nat.HistoryOut) == 64


def test_argument_errors_come_before_any_device_call():
    lib, h = nat.lib, C.c_void_p()
    msg = lambda: lib.tdsa_last_error_string().decode()      # noqa: E731
    for args, word in (((0, 30, 1, 0), "n_bins"), ((0, 0, 16, 0), "depth"), ((0, -3, 16, 0), "depth"),
                       ((0, 1 << 20, 1 << 10, 0), "depth"), ((0, 30, 16, 2), "kind"), ((0, 30, 16, -1), "kind")):
        assert lib.tdsa_history_create(*args, C.byref(h)) == ERR_ARG and word in msg() and not h.value, args
    assert lib.tdsa_history_create(0, 30, 16, 0, None) == ERR_ARG
    row = np.zeros(16, np.float32)
    p = row.ctypes.data_as(C.c_void_p)
    out, info = nat.HistoryOut(), nat.HistoryInfo()
    assert lib.tdsa_history_set_amplitude(None, 0.0, 100.0) == ERR_ARG and "null" in msg()
    assert lib.tdsa_history_reset(None) == ERR_ARG and lib.tdsa_history_reset_hold(None) == ERR_ARG
    assert lib.tdsa_history_push(None, p, None, None, 1) == ERR_ARG
    assert lib.tdsa_history_push_dev(None, None, p, 1) == ERR_ARG
    assert lib.tdsa_history_ribbon(None, p, 0, C.byref(out), C.byref(info)) == ERR_ARG
    assert lib.tdsa_history_lines(None, 0, 1, 0, None, 0, C.byref(out), C.byref(info)) == ERR_ARG
    assert lib.tdsa_history_surface(None, 0, C.byref(out), C.byref(info)) == ERR_ARG
    assert lib.tdsa_history_timer_begin(None) == ERR_ARG and lib.tdsa_history_timer_end(None, None) == ERR_ARG
    assert lib.tdsa_history_destroy(None) == 0
    with pytest.raises(ValueError):
        TraceHistory(30, 16, "depths")


@pytest.mark.skipif(not NO_GPU, reason="checks the no-GPU error path")
def test_without_a_gpu_the_handles_report_an_error():
    with pytest.raises(nat.TdsaError):
        TraceHistory(30, 256)
    assert b"failed" in nat.lib.tdsa_last_error_string()
    for cls in (RibbonView, ThreeDView, SurfaceView):
        v = cls()
        with pytest.raises(nat.TdsaError):
            v.update_widget_data(np.zeros(8, np.float32), None, np.linspace(1e6, 2e6, 8))
        assert getattr(v, "z", None) is None and getattr(v, "verts", None) is None


# ---------------------------------------------------------------------------------------------------- the shape cases
# tests/history_cases.py builds the rows of tests/test_gpu_history_shapes.py; what those rows claim is proved here.
def test_push_geometry_is_the_launcher_rule():
    assert cases.header_const("kHistPushMaxWgs") == 2048 and cases.header_const("kHistMaxCells") == history3d.MAX_CELLS
    src = open(os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc", "tdsa_history.hip")).read()
    launcher = src[src.index("hipError_t launch_hist_push"):src.index("hipError_t launch_hist_reduce")]
    assert "kHistPushMaxWgs / gx" in launcher and "2048" not in launcher
    assert cases.push_geometry(1024, 300) == (1, 300, 1, 1) and cases.push_geometry(1000, 75) == (1, 75, 1, 1)
    want = {(8192, 257): (8, 129, 2, 1), (4099, 250): (17, 84, 3, 1), (1001, 2051): (4, 411, 5, 1), (1024, 2049): (1, 1025, 2, 1)}
    for shape in cases.CHUNK_SHAPES:
        assert cases.push_geometry(*shape) == want[shape], shape
    assert cases.push_geometry(1024, 2049, aligned=False) == (4, 410, 5, 4)    # the same rows behind an odd pointer


@pytest.mark.parametrize("depth", cases.CHUNK_DEPTHS)
@pytest.mark.parametrize("n,n_rows", cases.CHUNK_SHAPES)
def test_chunk_cases_run_the_chunk_paths(n, n_rows, depth):
    case = cases.chunk_case(n, n_rows, depth)
    gx, gy, rpw, last = case["geometry"]
    skip, batch = case["skip"], case["batch"]
    assert batch.shape == (n_rows, n) and batch.nbytes <= 9 << 20 and not np.isnan(batch).any()
    assert rpw >= 2 and 1 <= last < rpw and (gy - 1) * rpw + last == n_rows            # a short last chunk
    assert 0 < skip == n_rows - depth
    # one host row first: slot (1 + k) % depth, so row k of the batch wraps to slot 0 where (1 + k) % depth == 0
    wraps = [k for k in range(skip + 1, n_rows) if (1 + k) % depth == 0]
    assert wraps, (skip, depth)
    if depth == 30:                                            # (depth 7: see the next test)
        assert skip % rpw != 0                                 # the first line of the ring is not the first row of a chunk
        assert any(k % rpw != 0 for k in wraps)                # and the ring wraps inside a chunk
    everything = np.concatenate([case["first"][None], batch])
    top = np.argmax(everything, axis=0) - 1                    # row of the batch that holds each column's maximum
    for name, cols in case["classes"].items():
        assert len(cols) >= 200
        for c in cols:
            k = case["planted"][int(c)]
            col = everything[:, c]
            assert top[c] == k and (np.delete(col, k + 1) < col[k + 1]).all(), (name, c)     # the maximum, and alone
            assert cases.CEILING < col[k + 1] < -10.0                                          # inside the height scale
            if name == "skipped":
                assert k < skip
                continue
            assert k >= skip
            second = int(np.argsort(col)[-2]) - 1
            if name == "chunk_end":
                assert k % rpw == rpw - 1 and second == k + 1
            else:
                assert k % rpw == 0 and second == k - 1 and second >= skip
    free = np.setdiff1d(np.arange(n), np.concatenate(list(case["classes"].values())))
    assert (batch[:, free] == 40.0).any() and np.isposinf(batch[:, free]).any() and np.isneginf(batch[:, free]).any()


def test_chunk_depth_7_puts_the_first_line_on_a_chunk_seam_or_inside_one():
    """With a depth of 7 the first stored row of three batches is the first row of a chunk, of the fourth it is not."""
    inside = {shape: (shape[1] - 7) % cases.push_geometry(*shape)[2] != 0 for shape in cases.CHUNK_SHAPES}
    assert inside == {(8192, 257): False, (4099, 250): False, (1001, 2051): True, (1024, 2049): False}


def test_one_bin_and_misaligned_cases_take_one_bin_lanes():
    for n in cases.ONE_BIN_N:
        P = cases.one_bin_columns(n)
        assert cases.lane_width(n) == 1 and 1 <= P <= n and P % 4 != 0
    assert max(cases.ONE_BIN_N) > 4 * cases.BLOCK and 65 in cases.ONE_BIN_N and 257 in cases.ONE_BIN_N
    for n in cases.MISALIGNED_N:
        assert n % 4 == 0
        rows = np.arange(3 * n, dtype=np.float32).reshape(3, n)
        for off in cases.MISALIGNED_OFFSETS:
            buf, at = cases.misaligned_buffer(rows, off)
            assert at % 16 == off and _same(buf[at // 4:at // 4 + 3 * n].reshape(3, n), rows)
            assert np.isposinf(buf[:at // 4]).all() and np.isposinf(buf[at // 4 + 3 * n:]).all()
            assert at // 4 >= 4 and buf.size - (at // 4 + 3 * n) >= 4


@pytest.mark.parametrize("n", cases.NEGATIVE_N)
def test_negative_rows_are_what_they_claim(n):
    V = cases.lane_width(n)
    named = cases.negative_rows(n)
    ats = {name: at for name, _, at, _ in named}
    assert ats["bin 0"] == 0 and ats["last bin"] == n - 1 and ats["last lane of a wave"] == 64 * V - 1
    assert ats["first bin of the second workgroup"] == 256 * V == (1024 if V == 4 else 256)
    for name, row, at, negative in named:
        assert row.dtype == np.float32 and row.shape == (n,) and not np.isnan(row).any()
        assert int(np.argmax(row)) == at == cases.key_argmax(row), name
        if negative:
            assert not (row >= 0).any(), name
            if np.isfinite(row[at]):
                assert (np.delete(row, at) < row[at]).sum() >= n - 2, name           # unique, or one equal maximum
        else:
            assert row[at] == 0 and (row == 0).sum() == 12 and (row[row != 0] < 0).all(), name
            zeros = row[row == 0]
            assert np.signbit(zeros).any() and not np.signbit(zeros).all()
            assert np.signbit(row[at]) == (name == "-0 before +0")
    row = dict((name, r) for name, r, _, _ in named)["equal maxima in two workgroups"]
    first, second = np.flatnonzero(row == row.max())
    assert first // (256 * V) == 0 and second // (256 * V) >= 1
    z = hc.heights(np.concatenate([r for _, r, _, neg in named if neg and np.isfinite(r).all()]), *cases.NEGATIVE_AMPLITUDE)
    assert (z > 0).all() and (z < 8).all()                                           # nothing clipped


def test_hist_key_restated_orders_as_argmax():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        row = cases.KEY_SPECIALS[rng.integers(0, cases.KEY_SPECIALS.size, 16)]
        assert cases.key_argmax(row) == int(np.argmax(row)), row
    keys = [cases.hist_key(v, 5) for v in cases.KEY_SPECIALS if not (v == 0 and np.signbit(v))]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys[0] > 0        # 0 is the untouched slot
    assert cases.hist_key(np.float32(-0.0), 5) == cases.hist_key(np.float32(0.0), 5)
    assert cases.hist_key(np.float32(-1.0), 4) > cases.hist_key(np.float32(-1.0), 5) > cases.hist_key(np.float32(-1.5), 0)


@pytest.mark.parametrize("n,columns", [(n, c) for n, by in cases.WIDTH_CASES.items() for c in by])
def test_width_cases_sit_on_the_group_thresholds(n, columns):
    G = cases.WIDTH_CASES[n][columns]
    cell = n // columns
    assert G == (64 if cell >= 32 else 16 if cell >= 8 else 4) == cases.reduce_group(n, columns)
    cells = hc.cells(n, columns)
    widths = {b - a for a, b in cells}
    assert widths == ({cell, cell + 1} if n % columns else {cell})                   # both widths where there are two
    rows, mn, plateaus, dead = cases.width_rows(n, columns)
    assert rows.shape == (cases.WIDTH_ROWS, n) and not np.isnan(rows).any() and cases.WIDTH_ROWS > cases.WIDTH_DEPTH
    assert _same(mn, rows.min(axis=0))
    lo, hi = cells[dead[1]]
    assert np.isneginf(rows[dead[0], lo:hi]).all() and cases.WIDTH_ROWS - 1 - dead[0] < cases.WIDTH_DEPTH
    if max(widths) >= 3:
        assert len(plateaus) >= cases.WIDTH_ROWS // 2
    for r, c, first, end in plateaus:
        lo, hi = cells[c]
        seg = rows[r, lo:hi]
        assert lo < first < hi and end > first + 1
        assert int(np.argmax(seg)) == first - lo and (seg[:first - lo] < rows[r, first]).all()
        assert (rows[r, first:min(end, hi)] == rows[r, first]).all()
        lanes = [(j - lo) % G for j in range(first, min(end, hi))]
        assert lanes[0] != 0 and len(set(lanes)) >= 2              # lane 0 holds a lower value, several lanes tie
        if hi - lo > G:
            assert min(lanes[1:]) < lanes[0]                       # a later bin of the plateau in a lower lane
        if end > hi and c + 1 < columns:
            assert int(np.argmax(rows[r, hi:cells[c + 1][1]])) == 0
    if n == 1000 and columns in (32, 126):
        assert any(cells[c][1] - cells[c][0] > G for _, c, _, _ in plateaus)


def test_arithmetic_edge_rows_hold_their_edges():
    row = cases.integer_edge_row(54)
    z = hc.heights(row, *cases.EXACT_AMPLITUDE)
    normal = (row == 0) | (np.abs(row) > 1e-30)
    assert _same(z[normal], np.clip(row, np.float32(0), np.float32(8))[normal]) and (z[~normal] == 0).all()
    for k in range(9):
        for v in (k, k + 0.5):
            below, above = np.nextafter(np.float32(v), np.float32(-9)), np.nextafter(np.float32(v), np.float32(9))
            assert (row == np.float32(v)).any() and (row == below).any() and (row == above).any()
    assert set(hc.line_index(z)) == set(range(9))
    assert _same(cases.integer_edge_row(56)[:54], row)
    pairs = cases.sextant_pairs()
    assert sorted(pairs) == [(0, 1), (1, 1), (14, 1), (14, 2), (29, 1), (29, 2), (29, 3)]
    for (r, s), (z_lo, z_hi) in pairs.items():
        assert z_lo.dtype == np.float32 and np.nextafter(z_lo, np.float32(9)) == z_hi and 0 < z_lo < 8
        assert cases.ribbon_sextant(r, z_lo) == s and cases.ribbon_sextant(r, z_hi) == s - 1
        _, lo_col = hc.ribbon_row(r, [z_lo], [0.0])                # the contract's colours: the one that is 0 changes
        _, hi_col = hc.ribbon_row(r, [z_hi], [0.0])
        zero = {0: 2, 1: 2, 2: 0, 3: 0}
        assert lo_col[0, zero[s]] == 0 and hi_col[0, zero[s - 1]] == 0
        val = np.float32(hc.ribbon_row_consts(r)[3])
        full = {0: 0, 1: 1, 2: 1, 3: 2}
        assert lo_col[0, full[s]] == val and hi_col[0, full[s - 1]] == val
    assert [float(v) for v in pairs[(29, 1)]] == [float(np.float32(5.979798)), float(np.float32(5.9797983))]
    srow = cases.sextant_row(113)
    assert _same(hc.heights(srow, *cases.EXACT_AMPLITUDE), srow)
    for k, (z_lo, z_hi) in enumerate(pairs.values()):
        block = srow[16 * k:16 * k + 16]
        assert block[7] == z_lo and block[8] == z_hi and (np.diff(block.view(np.uint32).astype(np.int64)) == 1).all()
    rows = cases.surface_edge_rows(24)
    for ref, rng_db in cases.SURFACE_AMPLITUDES:
        for v in (ref - rng_db, ref):
            f = np.float32(v)
            for x in (f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
                assert (rows[0] == x).any() and (rows[1] == x).any()
        t = hc.surface_normalise(rows, ref - rng_db, ref)
        assert not np.isnan(t).any() and (t == 0).any() and (t == 1).any()
    assert np.isposinf(rows[0]).any() and np.isneginf(rows[0]).any() and np.isfinite(rows[1]).all()
    assert ((rows[0] == 0) & np.signbit(rows[0])).any()


def test_nan_cases_name_the_lane_elements():
    assert cases.lane_width(cases.NAN_N) == 4
    assert [b % 4 for b in cases.NAN_BINS[:2]] == [0, 2] and cases.NAN_BINS[2] == cases.NAN_N - 1
    n, n_rows, depth = cases.NAN_CHUNK
    assert (n, n_rows) in cases.CHUNK_SHAPES and depth in cases.CHUNK_DEPTHS and cases.lane_width(n) == 4
    assert [cases.cell_of(1000, 7, j) for j in (0, 141, 142, 999)] == [0, 0, 1, 6]
