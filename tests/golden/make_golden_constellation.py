#!/usr/bin/env python3
"""Golden vectors for the constellation analysis from the *imported reference*.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_constellation.py

displays/constellation_2d.py needs PyQt6 / pyqtgraph, which are absent here: it is imported against do-nothing
stub modules (as make_golden_displays.py does), so the real Constellation2D runs its own update_iq_data, and the
reference DataProcessor._process_constellation_data formats the EVM read-out.  Blocks reach the reference as
complex64, converted from int8 / uint8 pairs by the a1 conventions (the tick the source hands over).

Writes tests/golden/constellation.npz, DATA only.  Per case k:
  c{k}_raw       the input (int8 / uint8 interleaved pairs or complex64)
  c{k}_meta      [fmt, range, max_points, is_scatter] float64, c{k}_mod the modulation name
  c{k}_evm       last_evm_rms (NaN array + c{k}_evm_none = 1 when the reference gives None)
  c{k}_counts    uint32 [128][128] = round(expm1(image)) (density cases; log1p(counts) == image is asserted)
  c{k}_sx/_sy    the scatter arrays (scatter cases)
  c{k}_text      the read-out label text
  ref_{name}     the reference's _CONST_REFS tables (their dtypes included)
"""
import os
import sys
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
for _m in ("hackrf", "rtlsdr", "sounddevice"):
    sys.modules[_m] = MagicMock()
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402


class Stub:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: Stub()

    def __call__(self, *a, **k):
        return Stub()


class ImageItem(Stub):
    image = None

    def setImage(self, img, **k):
        self.image = np.array(img)


class ScatterPlotItem(Stub):
    x = y = None

    def setData(self, x=None, y=None, **k):
        self.x, self.y = np.array(x), np.array(y)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


qtcore = _module("PyQt6.QtCore", QRectF=type("QRectF", (Stub,), {}), QTimer=Stub, pyqtSignal=Stub, Qt=Stub())
qtwidgets = _module("PyQt6.QtWidgets", QWidget=type("QWidget", (Stub,), {}),
                    QVBoxLayout=type("QVBoxLayout", (Stub,), {}), QLabel=Stub)
_module("PyQt6", QtCore=qtcore, QtWidgets=qtwidgets, QtGui=_module("PyQt6.QtGui", QColor=Stub, QFont=Stub))
_module("pyqtgraph", PlotWidget=Stub, ImageItem=ImageItem, ScatterPlotItem=ScatterPlotItem, colormap=Stub(),
        mkPen=Stub(), mkBrush=Stub())

from displays.constellation_2d import Constellation2D, _CONST_REFS  # noqa: E402
from core.display_data_processor import DataProcessor  # noqa: E402
from utils.constants import DisplayMode  # noqa: E402

IN_I8, IN_U8, IN_C64 = 0, 1, 2


class Label:
    text = None

    def setText(self, s):
        self.text = s


def to_complex(raw, fmt):
    if fmt == IN_I8:
        v = raw.astype(np.float32) / np.float32(128.0)
    elif fmt == IN_U8:
        v = (raw.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    else:
        return raw.astype(np.complex64)
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)


def symbols(rng, mod, n, snr_sigma):
    pts = _CONST_REFS.get(mod)
    if pts is None:
        pts = _CONST_REFS["qpsk"]
    k = rng.integers(0, len(pts), n)
    s = pts[k, 0] + 1j * pts[k, 1]
    s = s + snr_sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return s * np.exp(1j * 0.03)


def raw_block(rng, mod, n, fmt, sigma=0.06, amp=0.45):
    s = symbols(rng, mod, n, sigma) * amp
    if fmt == IN_I8:
        v = np.empty(2 * n)
        v[0::2], v[1::2] = s.real, s.imag
        return np.clip(np.round(v * 128.0), -128, 127).astype(np.int8)
    if fmt == IN_U8:
        v = np.empty(2 * n)
        v[0::2], v[1::2] = s.real, s.imag
        return np.clip(np.round((v + 1.0) * 127.5), 0, 255).astype(np.uint8)
    return (np.round(s * 4096.0) / 4096.0).astype(np.complex64)      # 12 fractional bits: the fixture compresses


def run_reference(raw, fmt, mod, r, max_points, scatter):
    w = Constellation2D()
    w.set_mode("scatter" if scatter else "density")
    w.set_modulation(mod)
    w.set_range(r)
    w.set_max_points(max_points)
    label = Label()
    src = types.SimpleNamespace(read_samples_only=lambda: to_complex(raw, fmt))
    mw = types.SimpleNamespace(current_source=src, current_stacked_index=DisplayMode.CONSTELLATION_2D,
                               constellation_2d_widget=w, marker_readout_label=label)
    dp = DataProcessor.__new__(DataProcessor)
    dp.mw, dp.dm = mw, types.SimpleNamespace(constellation_modulation=mod)
    with np.errstate(all="ignore"):
        dp._process_constellation_data()
    return w, label.text


def cases(rng):
    c = []
    # (modulation, fmt, n, range, max_points, scatter, raw)
    for mod, fmt, n, r in [("qpsk", IN_I8, 16384, 1.5), ("64qam", IN_I8, 16384, 1.5), ("64qam", IN_C64, 16384, 2.0),
                           ("16qam", IN_U8, 16384, 1.5), ("8psk", IN_C64, 8192, 1.5), ("bpsk", IN_I8, 8191, 0.7),
                           ("qpsk", IN_U8, 8193, 2.0), ("16qam", IN_C64, 127, 1.5), ("64qam", IN_I8, 5, 1.5),
                           ("ofdm", IN_I8, 16384, 1.5), ("qpsk", IN_I8, 100003, 1.5), ("8psk", IN_U8, 16384, 0.7),
                           ("bpsk", IN_C64, 4099, 2.0), ("16qam", IN_I8, 8192, 2.0)]:
        c.append((mod, fmt, n, r, 2000, False, raw_block(rng, mod, n, fmt)))
    for mod, fmt, n, mp in [("64qam", IN_U8, 30011, 2000), ("qpsk", IN_C64, 6000, 2000), ("8psk", IN_I8, 8193, 10000),
                            ("16qam", IN_I8, 5, 2000)]:
        c.append((mod, fmt, n, 1.5, mp, True, raw_block(rng, mod, n, fmt)))
    # exactly on the edges: a cross of (+-1, 0) / (0, +-1) has rms exactly 1, so the values stay -1, 0, 1: the first
    # and last edges (r = 1) and interior edges (r = 2, r = 0.5 with +-1 outside the range)
    k = rng.integers(0, 4, 16384)
    cross = np.array([1, -1, 1j, -1j], dtype=np.complex64)[k]
    for r in (1.0, 2.0, 0.5):
        c.append(("qpsk", IN_C64, 16384, r, 2000, False, cross))
    c.append(("qpsk", IN_I8, 8192, 1.5, 2000, False, np.zeros(2 * 8192, np.int8)))            # all zero: no AGC
    nanb = raw_block(rng, "qpsk", 8192, IN_C64)
    nanb[777] = np.complex64(complex(np.nan, 0.25))
    c.append(("qpsk", IN_C64, 8192, 1.5, 2000, False, nanb))
    c.append(("64qam", IN_C64, 4096, 1.5, 2000, True, nanb[:4096]))
    return c


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    cs = cases(rng)
    for k, (mod, fmt, n, r, mp, scatter, raw) in enumerate(cs):
        w, text = run_reference(raw, fmt, mod, r, mp, scatter)
        out[f"c{k}_raw"] = raw
        out[f"c{k}_mod"] = np.array(mod)
        out[f"c{k}_meta"] = np.array([fmt, r, mp, 1.0 if scatter else 0.0])
        out[f"c{k}_evm_none"] = np.int8(w.last_evm_rms is None)
        out[f"c{k}_evm"] = np.float64(np.nan if w.last_evm_rms is None else w.last_evm_rms)
        out[f"c{k}_text"] = np.array("" if text is None else text)
        if scatter:
            out[f"c{k}_sx"], out[f"c{k}_sy"] = w._scatter.x.astype(np.float32), w._scatter.y.astype(np.float32)
            assert w._scatter.x.dtype == np.float32
        else:
            img = w._img.image
            counts = np.rint(np.expm1(img)).astype(np.uint32)              # [q][i], as the image is laid out
            assert np.array_equal(np.log1p(counts.astype(np.float64)), img)
            out[f"c{k}_counts"] = counts
    for name, pts in _CONST_REFS.items():
        out[f"ref_{name}"] = pts
    out["n_cases"] = np.int64(len(cs))
    np.savez_compressed(os.path.join(HERE, "constellation.npz"), **out)
    print("wrote constellation.npz:", len(cs), "cases")


if __name__ == "__main__":
    main()
