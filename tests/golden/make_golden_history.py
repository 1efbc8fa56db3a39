#!/usr/bin/env python3
"""Golden vectors for the 3-D history views from the *imported reference*.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_history.py

displays/ribbon.py, three_dimension.py and surface.py need PyQt6, pyqtgraph.opengl and vispy, which are absent here:
they are imported against stub modules (the make_golden_displays.py pattern), with recording stand-ins for GLMeshItem /
GLLinePlotItem / SurfacePlot that keep what setMeshData / setData / set_data receive.  The real RibbonWidget, ThreeD and
Surface objects are constructed and their own numpy and matplotlib code runs.  Writes tests/golden/history.npz: seeded
float32 dB rows and settings in, the captured arrays at a handful of steps out.  DATA only.

The rows hold values below and above the scale, +-inf and a run saturated at the top; NO NaN: np.clip passes a NaN into
an undefined astype(int), so a NaN in a row is outside the contract (z is NaN, the colour unspecified).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402


class Any:
    """A do-nothing GUI object that remembers: attribute assignments in `_set`, calls of its methods in `_calls`."""

    def __init__(self, *a, **k):
        self.__dict__.update(_set={}, _calls=[], _kids={}, _parent=None, _name=None, _args=(a, k))

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name in self._set:
            return self._set[name]
        if name not in self._kids:
            kid = Any()
            kid.__dict__.update(_parent=self, _name=name)
            self._kids[name] = kid
        return self._kids[name]

    def __setattr__(self, name, value):
        if not isinstance(value, str) or name != "camera":      # view.camera = 'turntable' keeps the camera object
            self._set[name] = value

    def __call__(self, *a, **k):
        if self._parent is not None:
            self._parent._calls.append((self._name, a, k))
        return Any()

    def __getitem__(self, key):
        return Any()


class Plain:
    """Base of the widgets themselves: ordinary attributes, any constructor arguments, unknown methods do nothing."""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


class GLViewWidget(Plain):
    def __init__(self, *a, **k):
        self.opts = {}


class Recorder(Plain):
    """GLMeshItem / GLLinePlotItem / SurfacePlot: keyword arguments become attributes, as the real items keep them."""

    def __init__(self, *a, **k):
        self.moved = None
        self._take(k)

    def _take(self, k):
        for key, v in k.items():
            setattr(self, key, v)

    def setMeshData(self, **k):
        self._take(k)

    def setData(self, **k):
        self._take(k)

    def set_data(self, **k):
        self._take(k)

    def translate(self, *a):
        self.moved = a

    @property
    def mesh_data(self):
        return Any()


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


qtwidgets = _module("PyQt6.QtWidgets", QWidget=type("QWidget", (Plain,), {}), QVBoxLayout=Any)
qtgui = _module("PyQt6.QtGui", QVector3D=Any)
_module("PyQt6", QtWidgets=qtwidgets, QtGui=qtgui)
gl = _module("pyqtgraph.opengl", GLViewWidget=GLViewWidget, GLMeshItem=type("GLMeshItem", (Recorder,), {}),
             GLLinePlotItem=type("GLLinePlotItem", (Recorder,), {}), GLTextItem=type("GLTextItem", (Recorder,), {}),
             GLGridItem=Any, MeshData=Any())
_module("pyqtgraph", opengl=gl)
visuals = _module("vispy.scene.visuals", SurfacePlot=type("SurfacePlot", (Recorder,), {}), Sphere=Any)
scene = _module("vispy.scene", SceneCanvas=Any, Text=Any, transforms=Any(), visuals=visuals)


class _Colormap:
    """vispy is absent: the colours of the surface are not recorded (DESIGN.md 4.11 pins them to the restatement)."""

    def __init__(self, *a, **k):
        pass

    def map(self, x):
        return np.zeros((len(x), 4), dtype=np.float32)


_module("vispy.color", Colormap=_Colormap)
_module("vispy", scene=scene)

from displays.ribbon import RibbonWidget  # noqa: E402
from displays.surface import Surface  # noqa: E402
from displays.three_dimension import ThreeD  # noqa: E402

N = 256


def db_rows(rng, n_rows, n):
    """float32 dB rows: a noise floor near -90 dBm with a slowly moving tone, and the awkward values: bins far below
    and above the scale, +-inf, and a run of bins saturated above the reference level (a plateau at z = 8)."""
    k = np.arange(n)
    rows = []
    for r in range(n_rows):
        p = rng.exponential(1.0, size=n) * 1e-9
        p += 1e-3 * np.sinc((k - n / 3 - 0.37 * r) / 1.4) ** 2
        row = (10 * np.log10(p + 1e-12)).astype(np.float32)
        if r % 7 == 2:
            row[rng.integers(0, n, 3)] = -250.0
            row[rng.integers(0, n, 3)] = 150.0
        if r % 9 == 4:
            row[rng.integers(0, n, 2)] = -np.inf
            row[rng.integers(0, n, 2)] = np.inf
        if r % 5 == 3:
            row[100 + r:141 + r] = np.float32(10.0 + 0.25 * r)
        if r % 6 == 1:
            row -= np.float32(70.0)                       # a whole row at and below the bottom of the scale
        rows.append(row)
    rows = np.stack(rows)
    assert not np.isnan(rows).any()
    return rows


def f32_exact(a):
    a = np.asarray(a)
    b = a.astype(np.float32)
    assert np.array_equal(b.astype(a.dtype), a), "the captured array is not float32-exact"
    return b


def main():
    rng = np.random.default_rng(20250311)
    out = {}
    fb = np.linspace(99e6, 101e6, N)
    out["freq_bins"] = fb

    # ---- ribbon: 40 rows through the 30-row history, the amplitude changes in mid-run ---------------------------------
    rows = db_rows(rng, 40, N)
    amp = np.array([[0.0, 100.0]] * 18 + [[-20.0, 70.0]] * 22)     # (ref_level, range_db) in force at each push
    steps = [0, 25, 39]
    w = RibbonWidget()
    verts, colours = [], []
    for i, row in enumerate(rows):
        w.set_amplitude(float(amp[i, 0]), float(amp[i, 1]))
        w.update_widget_data(row, None, fb)
        if i in steps:
            assert all(r.vertexes.dtype == np.float32 and r.vertexColors.dtype == np.float32 for r in w.ribbons)
            verts.append(np.stack([r.vertexes for r in w.ribbons]))
            colours.append(np.stack([r.vertexColors for r in w.ribbons]))
    out.update(ribbon_rows=rows, ribbon_amp=amp, ribbon_steps=np.array(steps), ribbon_verts=np.stack(verts),
               ribbon_colours=np.stack(colours), ribbon_x=w._x, ribbon_faces=w.faces)

    # ---- line stack: 12 lines, 20 rows, max / min hold toggled, the amplitude changes once ------------------------------
    rows = db_rows(rng, 20, N)
    max_tr = np.maximum.accumulate(rows, axis=0)
    min_tr = np.minimum.accumulate(rows, axis=0)
    amp = np.array([[0.0, 100.0]] * 9 + [[-10.0, 90.0]] * 11)
    max_on = np.array([i >= 3 and not 10 <= i < 12 for i in range(20)])    # switched off at 10 (clears the hold), on at 12
    min_on = np.array([5 <= i < 15 for i in range(20)])
    steps = [0, 4, 9, 11, 13, 19]
    t = ThreeD()
    t.set_history_lines(12)
    t.set_peak_search_enabled(True)
    rec = {k: [] for k in ("z", "rgba", "hold", "hold_rgba", "min", "min_rgba", "peak", "max_peak", "texts")}
    for i, row in enumerate(rows):
        t.set_amplitude(float(amp[i, 0]), float(amp[i, 1]))
        if bool(max_on[i]) != t.max_peak_search_enabled:
            t.set_max_peak_search_enabled(bool(max_on[i]))
        if bool(min_on[i]) != t.min_hold_enabled:
            t.set_min_hold_enabled(bool(min_on[i]))
        t.update_widget_data(row, max_tr[i], fb, min_tr[i])
        if i in steps:
            L = t.num_history_lines
            rec["z"].append(np.stack([f32_exact(t.traces[k].pos[:, 2]) for k in range(L)]))
            rec["rgba"].append(np.stack([f32_exact(t.traces[k].color) for k in range(L)]))
            rec["hold"].append(f32_exact(t.max_hold_trace.pos[:, 2]))
            rec["hold_rgba"].append(np.asarray(t.max_hold_trace.color, dtype=np.float64))
            rec["min"].append(f32_exact(t.min_hold_trace.pos[:, 2]))
            rec["min_rgba"].append(np.asarray(t.min_hold_trace.color, dtype=np.float64))
            rec["peak"].append(np.asarray(t.peak_sphere.moved, dtype=np.float64))
            rec["max_peak"].append(np.asarray(t.max_peak_sphere.moved, dtype=np.float64))
            rec["texts"].append([t._live_freq.text, t._live_power.text, t._max_freq.text, t._max_power.text])
    out.update(lines_rows=rows, lines_max_trace=max_tr, lines_min_trace=min_tr, lines_amp=amp, lines_max_on=max_on,
               lines_min_on=min_on, lines_steps=np.array(steps), lines_depth=np.int64(12), lines_x=t.x,
               lines_y=t.line_y_values)
    for k, v in rec.items():
        out["lines_" + k] = np.array(v) if k == "texts" else np.stack(v)

    # ---- surface: 10 rows of history, 16 rows, the amplitude changes once (one step with zmax == zmin) ----------------
    rows = db_rows(rng, 16, N)
    amp = np.array([[0.0, 100.0]] * 7 + [[-30.0, 60.0]] * 8 + [[-30.0, 0.0]])
    steps = [0, 6, 9, 14, 15]
    s = Surface()
    s.set_history_lines(10)
    s.set_peak_search_enabled(True)
    rec = {k: [] for k in ("z", "peak", "texts")}
    for i, row in enumerate(rows):
        s.set_amplitude(float(amp[i, 0]), float(amp[i, 1]))
        s.update_widget_data(row, None, fb)
        if i in steps:
            assert s.surface.z.dtype == np.float64
            rec["z"].append(s.surface.z.astype(np.float32))            # float32(reference)
            rec["peak"].append(np.asarray(s.peak_sphere.transform._calls[-1][1][0], dtype=np.float64))
            rec["texts"].append([s.annotation_peak_label.text, s.annotation_peak_info.text])
    out.update(surface_rows=rows, surface_amp=amp, surface_steps=np.array(steps), surface_depth=np.int64(10),
               surface_x=s._mesh_x[0], surface_y=s._mesh_y[:, 0])
    for k, v in rec.items():
        out["surface_" + k] = np.array(v) if k == "texts" else np.stack(v)

    path = os.path.join(HERE, "history.npz")
    np.savez_compressed(path, **out)
    print("wrote history.npz:", os.path.getsize(path), "bytes;", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
