"""3-D history views on the device: ribbon, line stack, surface.

  TraceHistory   a ring of the last `depth` rows in HBM (tdsa_history_*), a running hold row, and the three view passes
                 that return what the reference's RibbonWidget, ThreeD and Surface hand their GL items - bit for bit at
                 full width, or reduced to `columns` screen columns (maximum and first bin of each cell)
  RibbonView, ThreeDView, SurfaceView
                 the data side of those widgets under the reference's method names: a DataProcessor drives them as
                 mw.ribbon_widget / mw.three_d_widget / mw.surface_widget

Rows are float32 dB without NaN (a NaN makes z NaN and its colour unspecified, as in the reference, whose
astype(int) of it is undefined); +-inf are fine.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat

Z_SCALE = 8
RIBBON_ROWS = 30
RIBBON_SPACING = 0.7
LINE_HUES = int(Z_SCALE * 1.4)
NEVER_PUSHED = 255
MAX_CELLS = 1 << 28
KINDS = {"heights": nat.HIST_HEIGHTS, "levels": nat.HIST_LEVELS}
MAX_HOLD_COLOUR = (1.0, 1.0, 0.0, 0.5)
MIN_HOLD_COLOUR = (0.2, 0.5, 1.0, 0.5)
_OUT_FIELDS = ("primary", "colours", "bins", "hold", "hold_bins", "min_row", "min_bins")


def ribbon_faces(n: int) -> np.ndarray:
    """Ribbon._make_faces: the uint32 [2 (n - 1)][3] triangles of an n-bin ribbon (2 n vertices)."""
    i = 2 * np.arange(int(n) - 1, dtype=np.uint32)
    return np.stack([np.stack([i, i + 1, i + 2], axis=1), np.stack([i + 1, i + 3, i + 2], axis=1)], axis=1).reshape(-1, 3)


def line_palette() -> np.ndarray:
    """float32 [11][4]: the colour of index k of the line stack, hsv_to_rgb([k / 11, 1, 1]) in float32, alpha 1."""
    h = np.arange(LINE_HUES, dtype=np.int32).astype(np.float32) / np.float32(LINE_HUES)
    one, six = np.float32(1), np.float32(6)
    i = (h * six).astype(int)
    f = (h * six) - i.astype(np.float32)
    v = np.ones_like(h)
    p, q, t = v * (one - one), v * (one - one * f), v * (one - one * (one - f))
    pal = np.ones((LINE_HUES, 4), dtype=np.float32)
    pal[:, 0] = np.choose(i % 6, [v, q, p, p, t, v])
    pal[:, 1] = np.choose(i % 6, [t, v, v, q, p, p])
    pal[:, 2] = np.choose(i % 6, [p, p, t, v, v, q])
    return pal


def _format_freq_hz(hz: float) -> str:
    hz = abs(hz)
    if hz >= 1e9:
        return f"{hz / 1e9:.3f} GHz"
    if hz >= 1e6:
        return f"{hz / 1e6:.3f} MHz"
    if hz >= 1e3:
        return f"{hz / 1e3:.3f} kHz"
    return f"{hz:.1f} Hz"


def _format_freq_mhz(mhz: float) -> str:
    if abs(mhz) >= 1.0:
        return f"{mhz:.3f} MHz"
    if abs(mhz) >= 0.001:
        return f"{mhz * 1000:.3f} kHz"
    return f"{mhz * 1e6:.1f} Hz"


def _row(a, n: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.float32)
    if a.size != n:
        raise ValueError(f"{what} has {a.size} bins, the history {n}")
    return a


class TraceHistory(nat._Handle, nat._Timer):
    """The last `depth` rows of `n_bins` bins on the device.  kind "heights": rows are stored as
    z = clip((dB - (ref - range)) / range * 8, 0, 8) with the amplitude in force at the push (ribbon, lines);
    "levels": as pushed, normalised at view time (surface)."""
    _destroy = "tdsa_history_destroy"
    _timer = ("tdsa_history_timer_begin", "tdsa_history_timer_end")

    def __init__(self, depth: int, n_bins: int, kind: str = "heights", device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind={kind!r}: one of {sorted(KINDS)}")
        self.depth, self.n_bins, self.kind, self.device = int(depth), int(n_bins), kind, int(device)
        self.ref_level, self.range_db = 0.0, 100.0
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_history_create(self.device, self.depth, self.n_bins, KINDS[kind], C.byref(self._h)))

    # ------------------------------------------------------------------ input
    def set_amplitude(self, ref_level: float, range_db: float) -> None:
        """For the rows pushed from now on (heights) / for the next view (levels)."""
        nat.check(nat.lib.tdsa_history_set_amplitude(self._h, float(ref_level), float(range_db)))
        self.ref_level, self.range_db = float(ref_level), float(range_db)

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_history_reset(self._h))

    def reset_hold(self) -> None:
        nat.check(nat.lib.tdsa_history_reset_hold(self._h))

    def push(self, live, max_trace=None, min_trace=None, hold: bool = True) -> None:
        """One host row.  The hold row follows z(max_trace), or the row itself without one; hold=False leaves it."""
        live = _row(live, self.n_bins, "the row")
        mx = None if max_trace is None else _row(max_trace, self.n_bins, "the max trace")
        mn = None if min_trace is None else _row(min_trace, self.n_bins, "the min trace")
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        nat.check(nat.lib.tdsa_history_push(self._h, p(live), p(mx), p(mn), int(bool(hold))))

    def push_rows(self, engine, rows_dev: int, n_rows: int) -> None:
        """n_rows rows already in device memory, in order, on `engine`'s stream after its work (None: the handle's
        own stream); no host wait."""
        nat.check(nat.lib.tdsa_history_push_dev(self._h, engine._h if engine is not None else None,
                                                C.c_void_p(int(rows_dev)), int(n_rows)))

    # ------------------------------------------------------------------ output
    def _columns(self, columns) -> int:
        if columns is None:
            return 0
        if not 1 <= int(columns) <= self.n_bins:
            raise ValueError(f"columns={columns}: 1 .. {self.n_bins}")
        return int(columns)

    @staticmethod
    def _out(host: dict, device_out: Optional[dict]):
        out = nat.HistoryOut()
        if device_out is not None:
            unknown = set(device_out) - set(_OUT_FIELDS)
            if unknown:
                raise ValueError(f"device_out: unknown destinations {sorted(unknown)}")
            out.on_device = 1
            for k, v in device_out.items():
                setattr(out, k, int(v))
            return out
        for k, a in host.items():
            setattr(out, k, a.ctypes.data)
        return out

    def ribbon(self, x, columns: Optional[int] = None, device_out: Optional[dict] = None) -> dict:
        """verts float32 [R][2 n][3], colours float32 [R][2 n][4] for rows 0 .. R - 1, R = min(30, depth); with
        columns=P also bins int32 [R][P].  device_out: {"primary": ptr, "colours": ptr, "bins": ptr} writes there."""
        P = self._columns(columns)
        x = _row(x, self.n_bins, "x")
        R, n = min(RIBBON_ROWS, self.depth), P or self.n_bins
        host = {}
        if device_out is None:
            host = dict(primary=np.empty((R, 2 * n, 3), np.float32), colours=np.empty((R, 2 * n, 4), np.float32))
            if P:
                host["bins"] = np.empty((R, P), np.int32)
        out, info = self._out(host, device_out), nat.HistoryInfo()
        nat.check(nat.lib.tdsa_history_ribbon(self._h, x.ctypes.data_as(C.c_void_p), P, C.byref(out), C.byref(info)))
        return dict(verts=host.get("primary"), colours=host.get("colours"), bins=host.get("bins"),
                    live_peak=(int(info.live_bin), np.float32(info.live_value)), pushed=int(info.pushed))

    def lines(self, first: int = 0, count: Optional[int] = None, colours: str = "index", columns: Optional[int] = None,
              device_out: Optional[dict] = None) -> dict:
        """Lines first .. first + count - 1 of the stack, newest first: z float32 [count][n]; index uint8 [count][n]
        (255: never pushed) or rgba float32 [count][n][4]; hold and min rows (min: None unless the newest push
        brought a min trace); live_peak and hold_peak as (bin, z)."""
        if colours not in ("index", "rgba"):
            raise ValueError(f"colours={colours!r}: 'index' or 'rgba'")
        P = self._columns(columns)
        first = int(first)
        count = self.depth - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.depth:
            raise ValueError(f"first={first}, count={count}: lines 0 .. {self.depth}")
        n = P or self.n_bins
        rgba = colours == "rgba"
        host = {}
        if device_out is None:
            host = dict(primary=np.empty((count, n), np.float32),
                        colours=np.empty((count, n, 4), np.float32) if rgba else np.empty((count, n), np.uint8),
                        hold=np.empty(n, np.float32), min_row=np.empty(n, np.float32))
            if P:
                host.update(bins=np.empty((count, P), np.int32), hold_bins=np.empty(P, np.int32),
                            min_bins=np.empty(P, np.int32))
        out, info = self._out(host, device_out), nat.HistoryInfo()
        pal = line_palette()
        nat.check(nat.lib.tdsa_history_lines(self._h, first, count, nat.HIST_COLOUR_RGBA if rgba else nat.HIST_COLOUR_INDEX,
                                             pal.ctypes.data_as(C.c_void_p), P, C.byref(out), C.byref(info)))
        has_min = bool(info.has_min)
        return dict(z=host.get("primary"), index=None if rgba else host.get("colours"),
                    rgba=host.get("colours") if rgba else None, bins=host.get("bins"), hold=host.get("hold"),
                    hold_bins=host.get("hold_bins"), min=host.get("min_row") if has_min else None,
                    min_bins=host.get("min_bins") if has_min else None, valid=int(info.valid_rows),
                    live_peak=(int(info.live_bin), np.float32(info.live_value)),
                    hold_peak=(int(info.hold_bin), np.float32(info.hold_value)), pushed=int(info.pushed))

    def surface(self, columns: Optional[int] = None, device_out: Optional[dict] = None) -> dict:
        """z float32 [depth][n] (normalised against the current amplitude), colours float32 [depth][n][3], live_peak
        (bin, level) and peak_norm, its normalised z."""
        P = self._columns(columns)
        n = P or self.n_bins
        host = {}
        if device_out is None:
            host = dict(primary=np.empty((self.depth, n), np.float32), colours=np.empty((self.depth, n, 3), np.float32))
            if P:
                host["bins"] = np.empty((self.depth, P), np.int32)
        out, info = self._out(host, device_out), nat.HistoryInfo()
        nat.check(nat.lib.tdsa_history_surface(self._h, P, C.byref(out), C.byref(info)))
        return dict(z=host.get("primary"), colours=host.get("colours"), bins=host.get("bins"),
                    live_peak=(int(info.live_bin), np.float32(info.live_value)), peak_norm=float(info.live_norm),
                    pushed=int(info.pushed))

    ribbon_faces = staticmethod(ribbon_faces)
    line_palette = staticmethod(line_palette)


# ---------------------------------------------------------------------------------------------------- the widgets
class _HistoryView:
    """What the three views share: the amplitude, the re-init rule (bin count or an end frequency changed, `!=` on the
    first and last bin) and the ring that goes with it."""

    KIND = "heights"

    def __init__(self, depth: int, device: int = 0, columns: Optional[int] = None):
        self.ref_level, self.range_db = 0.0, 100.0
        self.frequency_bins = None
        self.history: Optional[TraceHistory] = None
        self.peak_search_enabled = False
        self.max_peak_search_enabled = False
        self.min_hold_enabled = False
        self.log_freq = False
        self.columns = columns
        self.reinits = 0
        self._depth, self._device = int(depth), int(device)
        self._visible = True

    def isVisible(self) -> bool:
        return self._visible

    def setVisible(self, visible: bool) -> None:
        self._visible = bool(visible)

    def close(self) -> None:
        if self.history is not None:
            self.history.close()
            self.history = None

    def set_amplitude(self, ref_level: float, range_db: float) -> None:
        self.ref_level, self.range_db = ref_level, range_db
        if self.history is not None:
            self.history.set_amplitude(ref_level, range_db)

    def set_peak_search_enabled(self, enabled: bool) -> None:
        self.peak_search_enabled = enabled

    def set_max_peak_search_enabled(self, enabled: bool) -> None:
        self.max_peak_search_enabled = enabled

    def set_min_hold_enabled(self, enabled: bool) -> None:
        self.min_hold_enabled = enabled

    def set_log_freq(self, enabled: bool) -> None:
        self.log_freq = enabled

    def _bins_key(self, bins):
        return bins

    def _stale(self, bins) -> bool:
        fb = self.frequency_bins
        key = self._bins_key(bins)
        return fb is None or len(fb) != len(key) or fb[0] != key[0] or fb[-1] != key[-1]

    def _rebuild(self) -> None:
        self.close()
        self.history = TraceHistory(self._depth, len(self.frequency_bins), self.KIND, self._device)
        self.history.set_amplitude(self.ref_level, self.range_db)
        self.reinits += 1

    def update_frequency_bins(self, bins) -> None:
        if bins is None or len(bins) == 0:
            return
        self.frequency_bins = self._bins_key(np.asarray(bins)).copy()
        self._make_x()
        self._rebuild()

    def _cols(self):
        return None if self.columns is None else min(int(self.columns), len(self.frequency_bins))


class RibbonView(_HistoryView):
    """RibbonWidget: after a tick `verts` [30][2 n][3], `colours` [30][2 n][4] (and `bins` when reduced); `faces` and
    `x` change with the bins."""

    def __init__(self, device: int = 0, columns: Optional[int] = None):
        super().__init__(RIBBON_ROWS, device, columns)
        self.x = self.faces = self.verts = self.colours = self.bins = None

    def _make_x(self) -> None:
        fb = self.frequency_bins
        f0, f1 = float(fb[0]), float(fb[-1])
        span = f1 - f0 if f1 != f0 else 1.0
        self.x = (-10.0 + (fb.astype(np.float32) - f0) / span * 20.0)
        self.faces = ribbon_faces(self._cols() or len(fb))

    def update_frequency_bins(self, bins) -> None:
        if bins is None or len(bins) == 0:
            return
        if self.frequency_bins is None or len(self.frequency_bins) != len(bins):
            super().update_frequency_bins(bins)
        else:                                    # the widget keeps its heights when only the range moved
            self.frequency_bins = np.asarray(bins).copy()
            self._make_x()

    def update_widget_data(self, live_power_levels, max_power_levels, frequency_bins, min_power_levels=None) -> None:
        if live_power_levels is None or frequency_bins is None:
            return
        if isinstance(live_power_levels, tuple):
            live_power_levels = live_power_levels[0]
        if self._stale(frequency_bins):
            self.update_frequency_bins(frequency_bins)
        if self.history is None:
            return
        self.history.push(live_power_levels)
        v = self.history.ribbon(self.x, self._cols())
        self.verts, self.colours, self.bins = v["verts"], v["colours"], v["bins"]


class ThreeDView(_HistoryView):
    """ThreeD: after a tick `z` [L][n] and `index` [L][n] (palette: line_palette()), `x`, `y` (one per line), the hold
    row `max_hold_z` with `max_hold_colour` and `min_hold_z` with `min_hold_colour` (colour 0: hidden), `peak` /
    `max_peak` as (x, y, z) or None, and the read-outs `live_freq_text`, `live_power_text`, `max_freq_text`,
    `max_power_text`."""

    NUMBER_OF_LINES = 300

    def __init__(self, device: int = 0, columns: Optional[int] = None):
        super().__init__(self.NUMBER_OF_LINES, device, columns)
        self.num_history_lines = self.NUMBER_OF_LINES
        self.line_y_values = np.linspace(10, -10, self.num_history_lines)
        self.x = self.z = self.index = self.bins = None
        self.max_hold_z = self.min_hold_z = None
        self.max_hold_colour = self.min_hold_colour = (0, 0, 0, 0)
        self.peak = self.max_peak = None
        self.live_freq_text = self.live_power_text = self.max_freq_text = self.max_power_text = ""

    @property
    def y(self):
        return self.line_y_values

    def _make_x(self) -> None:
        fb = self.frequency_bins
        f0, f1 = float(np.min(fb)), float(np.max(fb))
        if f1 == f0:
            f1 = f0 + 1.0
        if self.log_freq:
            lb = np.log10(np.maximum(fb, 1.0))
            lf0, lf1 = np.log10(max(f0, 1.0)), np.log10(max(f1, 1.0))
            span = lf1 - lf0 if lf1 != lf0 else 1.0
            self.x = -10 + ((lb - lf0) / span) * 20
        else:
            self.x = -10 + ((fb - f0) / (f1 - f0)) * 20

    def update_frequency_bins(self, bins) -> None:
        if bins is None or len(bins) == 0 or not self._stale(bins):
            return
        super().update_frequency_bins(bins)

    def set_log_freq(self, enabled: bool) -> None:
        """Changes x on the host and, as the widget's re-initialisation does, empties the stack."""
        self.log_freq = enabled
        if self.frequency_bins is not None and len(self.frequency_bins) > 0:
            self._make_x()
            self.history.reset()

    def set_history_lines(self, n: int) -> None:
        if n == self.num_history_lines:
            return
        self.num_history_lines = self._depth = int(n)
        self.line_y_values = np.linspace(10, -10, n)
        if self.frequency_bins is not None and len(self.frequency_bins) > 0:
            self._rebuild()

    def set_peak_search_enabled(self, enabled: bool) -> None:
        self.peak_search_enabled = enabled
        if not enabled:
            self.peak = self.max_peak = None
            self.live_freq_text = self.live_power_text = self.max_freq_text = self.max_power_text = ""

    def set_max_peak_search_enabled(self, enabled: bool) -> None:
        self.max_peak_search_enabled = enabled
        if not enabled:
            if self.history is not None:
                self.history.reset_hold()
            self.max_hold_colour = (0, 0, 0, 0)

    def set_min_hold_enabled(self, enabled: bool) -> None:
        self.min_hold_enabled = enabled
        if not enabled:
            self.min_hold_colour = (0, 0, 0, 0)

    def update_widget_data(self, live_power_levels, max_power_levels, frequency_bins, min_power_levels=None) -> None:
        if live_power_levels is None or frequency_bins is None:
            return
        if max_power_levels is None:
            max_power_levels = live_power_levels
        if isinstance(live_power_levels, tuple):
            live_power_levels = live_power_levels[0]
        if isinstance(max_power_levels, tuple):
            max_power_levels = max_power_levels[0]
        if self._stale(frequency_bins):
            self.update_frequency_bins(frequency_bins)
        if self.history is None:
            return
        want_min = self.min_hold_enabled and min_power_levels is not None
        self.history.push(live_power_levels, max_power_levels if self.max_peak_search_enabled else None,
                          min_power_levels if want_min else None, hold=self.max_peak_search_enabled)
        v = self.history.lines(columns=self._cols())
        self.z, self.index, self.bins = v["z"], v["index"], v["bins"]
        if self.max_peak_search_enabled:
            self.max_hold_z, self.max_hold_colour = v["hold"], MAX_HOLD_COLOUR
        if want_min:
            self.min_hold_z, self.min_hold_colour = v["min"], MIN_HOLD_COLOUR
        if not self.peak_search_enabled:
            return
        fb, y0 = self.frequency_bins, float(self.line_y_values[0])
        li, lz = v["live_peak"]
        self.peak = (float(self.x[li]), y0, float(lz))
        self.live_freq_text = _format_freq_hz(float(fb[li]))
        self.live_power_text = f"{float(np.asarray(live_power_levels).reshape(-1)[li]):.1f} dBm"
        if self.max_peak_search_enabled:
            mi, mz = v["hold_peak"]
            self.max_peak = (float(self.x[mi]), y0, float(mz))
            self.max_freq_text = _format_freq_hz(float(fb[mi]))
            self.max_power_text = f"{float(np.asarray(max_power_levels).reshape(-1)[mi]):.1f} dBm"
        else:
            self.max_peak = None
            self.max_freq_text = self.max_power_text = ""


class SurfaceView(_HistoryView):
    """Surface: after a tick `z` [depth][n] (normalised) and `colours` [depth][n][3], the mesh axes `x`, `y`, `peak`
    (normalised x, 0, normalised z) or None, and the read-outs `peak_label_text`, `peak_info_text`."""

    KIND = "levels"

    def __init__(self, device: int = 0, columns: Optional[int] = None):
        super().__init__(100, device, columns)
        self.history_depth = 100
        self.x = self.y = self.z = self.colours = self.bins = None
        self.peak = None
        self.peak_label_text = self.peak_info_text = ""

    def _bins_key(self, bins):
        return np.asarray(bins) * 1e-6            # the widget keeps MHz, and compares in MHz

    def _make_x(self) -> None:
        self.x = np.linspace(0, 1, len(self.frequency_bins))
        self.y = np.linspace(0, 1, self.history_depth)

    def update_frequency_bins(self, bins) -> None:
        if bins is None or len(bins) == 0 or not np.all(np.isfinite(bins)):
            return
        super().update_frequency_bins(bins)

    def set_history_lines(self, n: int) -> None:
        self.history_depth = self._depth = int(n)
        if self.frequency_bins is not None:
            self._make_x()
            self._rebuild()

    def set_peak_search_enabled(self, enabled: bool) -> None:
        self.peak_search_enabled = enabled
        if not enabled:
            self.peak = None
            self.peak_label_text = self.peak_info_text = ""

    def update_widget_data(self, live_data, max_data, frequency_bins, min_power_levels=None) -> None:
        if live_data is None or frequency_bins is None:
            return
        if isinstance(live_data, tuple):
            live_data = live_data[0]
        if self._stale(frequency_bins):
            self.update_frequency_bins(frequency_bins)
        if self.history is None:
            return
        self.history.push(live_data)
        v = self.history.surface(self._cols())
        self.z, self.colours, self.bins = v["z"], v["colours"], v["bins"]
        if not self.peak_search_enabled:
            return
        fb = self.frequency_bins
        i, level = v["live_peak"]
        nx = (fb[i] - fb[0]) / (fb[-1] - fb[0]) if fb[-1] != fb[0] else 0.5
        self.peak = (float(nx), 0.0, v["peak_norm"])
        self.peak_label_text = "Live peak"
        self.peak_info_text = f"{_format_freq_mhz(fb[i])}\n{level:.1f} dBm"
