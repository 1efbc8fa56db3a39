"""Device-side trace analytics and display accumulators.

Everything here consumes dB rows that already sit in HBM (the output of SpectrumEngine.process_device /
HostPipe) and returns scalars or a small image, so a batch user never reads the [frames, N] block back:

  rows_stats        np.max / np.argmax per row (DutyCycleAnalyser.update_from_power, core/duty_cycle.py:36;
                    marker snap fallback core/marker_manager.py:97) + MarkerManager._band_power (:308-319)
  rows_top_peaks    DataProcessor._find_top_peaks (core/display_data_processor.py:432-471)
  rows_marker_peaks MarkerManager.snap_to_peak / snap_to_next_peak (core/marker_manager.py:74-127): scipy's
                    find_peaks(height, prominence, distance) per row + the bin each method would move the marker to
  DutyCycle         DutyCycleAnalyser (core/duty_cycle.py) fed with device-computed per-frame peaks
  DensityHistogram  DensityDisplay._hist (displays/density_display.py:300-320)
  WaterfallRing     Waterfall._buf / _add_row / _display_view (displays/waterfall.py:163-180, 330-336)
  Constellation     Constellation2D.update_iq_data (displays/constellation_2d.py:104-160): AGC, EVM, IQ density, on raw
                    IQ blocks from the host or captures in HBM; ConstellationView is the widget's data side
"""
import ctypes as C
import logging
from collections import deque
from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from ._native import _Handle
from .engine import SpectrumEngine

AMP_BINS = 512
AMP_MIN = -200.0
AMP_RNG = 300.0


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def band_bin_range(freq_bins: np.ndarray, f_start: float, f_stop: float) -> Tuple[int, int]:
    """Inclusive bin range selected by `(bins >= lo) & (bins <= hi)` on an increasing axis; (0, -1) if empty."""
    lo, hi = min(f_start, f_stop), max(f_start, f_stop)
    a = int(np.searchsorted(freq_bins, lo, side="left"))
    b = int(np.searchsorted(freq_bins, hi, side="right")) - 1
    return (a, b) if a <= b else (0, -1)


def rows_stats(engine: SpectrumEngine, rows_dev: int, n_rows: int, n_bins: Optional[int] = None,
               freq_bins: Optional[np.ndarray] = None, band: Optional[Tuple[float, float]] = None):
    """(peak_db[n_rows] f32, peak_bin[n_rows] i32, band_db[n_rows] f64 or None).  `band` = (f_start, f_stop) on
    `freq_bins`; rows whose band holds no bin report NaN (the reference returns None)."""
    n = int(n_bins or engine.nfft)
    peak = np.empty(n_rows, dtype=np.float32)
    pbin = np.empty(n_rows, dtype=np.int32)
    bdb = None
    lo, hi, width = 0, -1, 0.0
    if band is not None:
        if freq_bins is None:
            raise ValueError("band power needs the frequency axis")
        lo, hi = band_bin_range(freq_bins, *band)
        width = float((freq_bins[-1] - freq_bins[0]) / max(len(freq_bins) - 1, 1))
        bdb = np.empty(n_rows, dtype=np.float64)
    nat.check(nat.lib.tdsa_rows_stats(engine._h, C.c_void_p(rows_dev), int(n_rows), n, lo, hi, width,
                                      _p(peak), _p(pbin), _p(bdb) if bdb is not None else None))
    return peak, pbin, bdb


def rows_top_peaks(engine: SpectrumEngine, rows_dev: int, n_rows: int, n_bins: Optional[int] = None, n: int = 5,
                   min_sep_bins: Optional[int] = None, min_excursion_db: float = 10.0):
    """(bins[n_rows, n] i32 padded with -1, db[n_rows, n] f32 padded with NaN); min_sep_bins defaults to the
    reference's max(10, n_bins // 50) (display_data_processor.py:416); below 1 it means "no separation rule".
    min_excursion_db is a float32 on the device: the result is the reference's for float(np.float32(min_excursion_db))
    (6.3 means 6.30000019...); NaN is refused.  A NaN between two peaks never rejects, as in the reference.  Equal
    candidates are visited larger bin first."""
    nb = int(n_bins or engine.nfft)
    sep = max(10, nb // 50) if min_sep_bins is None else int(min_sep_bins)
    bins = np.empty((n_rows, n), dtype=np.int32)
    db = np.empty((n_rows, n), dtype=np.float32)
    nat.check(nat.lib.tdsa_rows_top_peaks(engine._h, C.c_void_p(rows_dev), int(n_rows), nb, int(n), sep,
                                          float(min_excursion_db), _p(bins), _p(db)))
    return bins, db


def rows_marker_peaks(engine: SpectrumEngine, rows_dev: int, n_rows: int, n_bins: Optional[int] = None,
                      peak_threshold: float = -200.0, peak_excursion: float = 6.0, distance: int = 3,
                      current_idx: int = -1, max_list: int = 0):
    """The marker peak search of core/marker_manager.py:74-127 on device rows.  Defaults are the reference's
    (getattr(main_window, 'peak_threshold', -200.0), 'peak_excursion' 6.0, distance=3).  Returns a dict:
      n_peaks[n_rows]   how many peaks find_peaks(levels, height, prominence, distance) reports
      snap_bin[n_rows]  where snap_to_peak puts the marker: the highest peak, or np.argmax(levels) without one
      next_bin[n_rows]  where snap_to_next_peak puts it from bin `current_idx` (= np.searchsorted(bins, position)):
                        next peak to the right, wrapping; -1 = no peak, the marker stays
      peaks[n_rows, max_list] / prominences   (max_list > 0) the first peaks in bin order, padded with -1 / NaN"""
    nb = int(n_bins or engine.nfft)
    cnt = np.empty(n_rows, dtype=np.int32)
    snap = np.empty(n_rows, dtype=np.int32)
    nxt = np.empty(n_rows, dtype=np.int32)
    bins = np.empty((n_rows, max_list), dtype=np.int32) if max_list > 0 else None
    prom = np.empty((n_rows, max_list), dtype=np.float64) if max_list > 0 else None
    nat.check(nat.lib.tdsa_rows_marker_peaks(engine._h, C.c_void_p(rows_dev), int(n_rows), nb, float(peak_threshold),
                                             float(peak_excursion), int(distance), int(current_idx), int(max_list),
                                             _p(cnt), _p(snap), _p(nxt), _p(bins) if bins is not None else None,
                                             _p(prom) if prom is not None else None))
    out = {"n_peaks": cnt, "snap_bin": snap, "next_bin": nxt}
    if max_list > 0:
        out["peaks"], out["prominences"] = bins, prom
    return out


def peaks_as_reference(freq_bins: np.ndarray, bins_row: np.ndarray, db_row: np.ndarray) -> List[Tuple[float, float]]:
    """One row of rows_top_peaks in the reference's return shape: [(freq, power), ...]."""
    return [(float(freq_bins[b]), float(p)) for b, p in zip(bins_row, db_row) if b >= 0]


from .core.duty_cycle import DutyCycleAnalyser  # noqa: E402


class DutyCycle(DutyCycleAnalyser):
    """The analyser of core/duty_cycle.py under the name earlier callers of this module use."""


class DensityHistogram(_Handle):
    """DensityDisplay._hist on the device: [n_bins, 512] float32."""
    _destroy = "tdsa_density_destroy"

    def __init__(self, n_bins: int, decay: float = 0.96, device: int = 0):
        self.n_bins = int(n_bins)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_density_create(int(device), self.n_bins, float(decay), C.byref(self._h)))

    def set_decay(self, decay: float) -> None:
        nat.check(nat.lib.tdsa_density_set_decay(self._h, float(decay)))

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_density_reset(self._h))

    def update(self, live_db: np.ndarray) -> None:
        row = np.ascontiguousarray(live_db, dtype=np.float32)
        nat.check(nat.lib.tdsa_density_update(self._h, _p(row), int(row.size)))

    def update_rows(self, engine: Optional[SpectrumEngine], rows_dev: int, n_rows: int) -> None:
        nat.check(nat.lib.tdsa_density_update_dev(self._h, engine._h if engine is not None else None,
                                                  C.c_void_p(rows_dev), int(n_rows)))

    def hist(self) -> np.ndarray:
        out = np.empty((self.n_bins, AMP_BINS), dtype=np.float32)
        nat.check(nat.lib.tdsa_density_read(self._h, _p(out), 0))
        return out

    def image(self) -> np.ndarray:
        """np.log1p(hist): what the reference hands to setImage (density_display.py:320)."""
        out = np.empty((self.n_bins, AMP_BINS), dtype=np.float32)
        nat.check(nat.lib.tdsa_density_read(self._h, _p(out), 1))
        return out


    def image_u8(self):
        """(uint8 [n_bins, 512], (lo, hi)): np.log1p(hist) as setImage(..., autoLevels=True) quantises it for its colour
        table (density_display.py:318), levels = the image's minimum / maximum; a quarter of the bytes of image()."""
        out = np.empty((self.n_bins, AMP_BINS), dtype=np.uint8)
        lv = np.empty(2, dtype=np.float32)
        nat.check(nat.lib.tdsa_density_read_u8(self._h, _p(out), _p(lv)))
        return out, (float(lv[0]), float(lv[1]))


class WaterfallRing(_Handle):
    """Waterfall._buf on the device ([H, n_bins] float32, every line once; the reference doubles it to make the view one
    slice) with the reference's pointer walk and dedup."""
    _destroy = "tdsa_waterfall_destroy"

    def __init__(self, history_lines: int, n_bins: int, min_db: float, device: int = 0):
        self.history_lines = int(history_lines)
        self.n_bins = int(n_bins)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_waterfall_create(int(device), self.history_lines, self.n_bins, float(min_db),
                                                C.byref(self._h)))

    def push(self, live_power_levels) -> bool:
        row = np.ascontiguousarray(live_power_levels, dtype=np.float32)
        new = C.c_int()
        nat.check(nat.lib.tdsa_waterfall_push(self._h, _p(row), int(row.size), C.byref(new)))
        return bool(new.value)

    def push_rows(self, engine: Optional[SpectrumEngine], rows_dev: int, n_rows: int) -> int:
        new = C.c_int()
        nat.check(nat.lib.tdsa_waterfall_push_dev(self._h, engine._h if engine is not None else None,
                                                  C.c_void_p(rows_dev), int(n_rows), C.byref(new)))
        return new.value

    @property
    def ptr(self) -> int:
        v = C.c_int()
        nat.check(nat.lib.tdsa_waterfall_view(self._h, None, C.byref(v)))
        return v.value

    def view(self) -> np.ndarray:
        out = np.empty((self.history_lines, self.n_bins), dtype=np.float32)
        nat.check(nat.lib.tdsa_waterfall_view(self._h, _p(out), None))
        return out

    def view_u8(self, min_db: float, max_db: float) -> np.ndarray:
        """uint8 [history_lines, n_bins]: the view as setImage(img, autoLevels=False, levels=(wf_min_db, wf_max_db))
        quantises it (displays/waterfall.py:353-356)."""
        out = np.empty((self.history_lines, self.n_bins), dtype=np.uint8)
        nat.check(nat.lib.tdsa_waterfall_view_u8(self._h, float(min_db), float(max_db), _p(out)))
        return out


# ---- constellation analysis (displays/constellation_2d.py:104-160) --------------------------
CONSTELLATION_BINS = 128           # Constellation2D._resolution
_log = logging.getLogger(__name__)


def constellation_points(name: str) -> Optional[np.ndarray]:
    """The reference point table of a modulation ([M, 2], the reference's dtype: float64 for qpsk, float32 otherwise), or
    None for a name the reference does not know (its EVM is then None)."""
    name = str(name)
    if name == "bpsk":
        return np.array([[-1.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    if name == "qpsk":     # a float32 table divided by the float64 sqrt(2): float64 under NEP 50
        return np.array([[-1, -1], [-1, 1], [1, -1], [1, 1]], dtype=np.float32) / np.sqrt(2.0)
    if name == "8psk":     # cos / sin of k * pi / 4 in double, stored as float32
        return np.array([[np.cos(a), np.sin(a)] for a in (k * np.pi / 4 for k in range(8))], dtype=np.float32)
    if name in ("16qam", "64qam"):   # the odd-integer grid, scaled by its own float32 rms
        side = 4 if name == "16qam" else 8
        lv = np.arange(1 - side, side, 2, dtype=np.float32)
        grid = np.stack([np.repeat(lv, side), np.tile(lv, side)], axis=1)
        rms = np.sqrt(np.mean(grid[:, 0] ** 2 + grid[:, 1] ** 2))
        return grid / rms if rms > 0 else grid
    return None


def _iq_input(samples, fmt: Optional[int]):
    """(contiguous array, TDSA_IN_* format, sample count) of a host block."""
    a = np.asarray(samples)
    if fmt is None:
        if np.iscomplexobj(a):
            fmt = nat.IN_C64
        elif a.dtype == np.int8:
            fmt = nat.IN_I8
        elif a.dtype == np.uint8:
            fmt = nat.IN_U8
        else:
            raise ValueError(f"real input ({a.dtype}, shape {a.shape}): the device constellation pass takes complex IQ "
                             "(complex, or interleaved int8 / uint8 pairs); the reference's Hilbert path is not supported")
    if fmt == nat.IN_C64:
        a = np.ascontiguousarray(a.reshape(-1), dtype=np.complex64)
        return a, fmt, a.size
    if fmt in (nat.IN_I8, nat.IN_U8):
        a = np.ascontiguousarray(a.reshape(-1), dtype=np.int8 if fmt == nat.IN_I8 else np.uint8)
        if a.size % 2:
            raise ValueError("interleaved I/Q bytes of odd length")
        return a, fmt, a.size // 2
    return a, int(fmt), a.size      # the library refuses it


class ConstellationResult:
    """One block's analysis: rms (float32), evm_rms (float, None where the reference gives None), counts
    ([bins][bins] uint32 in image layout [q_bin][i_bin], or None), and the scatter tail."""

    def __init__(self, rms, evm_rms, counts, tail_i, tail_q):
        self.rms, self.evm_rms, self.counts = rms, evm_rms, counts
        self._ti, self._tq = tail_i, tail_q

    def image(self) -> np.ndarray:
        """np.log1p(hist).T of the reference: what setImage receives (float64 [q_bin][i_bin])."""
        return np.log1p(self.counts.astype(np.float64))

    def scatter(self, n: Optional[int] = None):
        """(i, q) float32 of the last n normalised samples (n <= the n_tail processed; default all of them)."""
        if n is None:
            return self._ti, self._tq
        n = int(n)
        return self._ti[self._ti.size - n:], self._tq[self._tq.size - n:]


class Constellation(_Handle):
    """Constellation2D.update_iq_data on the device: RMS AGC, nearest-symbol EVM and the 2-D IQ density histogram, bit
    for bit the reference's numpy."""
    _destroy = "tdsa_constellation_destroy"

    def __init__(self, max_host_samples: int = 1 << 20, device: int = 0, modulation: str = "qpsk",
                 range_: float = 1.5, bins: int = CONSTELLATION_BINS):
        self.max_host_samples = int(max_host_samples)
        self.device = int(device)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_constellation_create(self.device, self.max_host_samples, C.byref(self._h)))
        self.bins, self.range = int(bins), float(range_)
        nat.check(nat.lib.tdsa_constellation_set_density(self._h, self.range, self.bins))
        self.set_modulation(modulation)

    def set_modulation(self, name: str) -> None:
        pts = constellation_points(name)
        if pts is None:
            nat.check(nat.lib.tdsa_constellation_set_refs(self._h, None, 0, 0))
        else:
            xy = np.ascontiguousarray(pts)
            nat.check(nat.lib.tdsa_constellation_set_refs(self._h, _p(xy), int(len(xy)), int(xy.dtype == np.float64)))
        self.modulation = name

    def set_range(self, r: float) -> None:
        nat.check(nat.lib.tdsa_constellation_set_density(self._h, float(r), self.bins))
        self.range = float(r)

    def set_bins(self, n: int) -> None:
        nat.check(nat.lib.tdsa_constellation_set_density(self._h, self.range, int(n)))
        self.bins = int(n)

    def process(self, samples, fmt: Optional[int] = None, n_tail: int = 0, counts: bool = True) -> ConstellationResult:
        """One host block (complex, or interleaved int8 / uint8 pairs; fmt overrides the dtype's format)."""
        a, fmt, n = _iq_input(samples, fmt)
        rms = C.c_float()
        evm = C.c_double()
        has = C.c_int()
        cnt = np.empty((self.bins, self.bins), dtype=np.uint32) if counts else None
        nt = max(0, min(int(n_tail), n))
        tail = np.empty(2 * nt, dtype=np.float32)
        nat.check(nat.lib.tdsa_constellation_process(self._h, fmt, _p(a), n, nt, C.byref(rms), C.byref(evm),
                                                     C.byref(has), _p(cnt) if cnt is not None else None,
                                                     _p(tail) if nt else None))
        return ConstellationResult(np.float32(rms.value), float(evm.value) if has.value else None, cnt, tail[:nt],
                                   tail[nt:])

    def process_segments(self, engine: Optional[SpectrumEngine], ptr: int, fmt: int, seg_len: int, hop: int,
                         n_seg: int, counts_dev: Optional[int] = None):
        """A capture already on the device (ptr): n_seg segments of seg_len samples every hop samples, each analysed as
        its own block.  Returns (rms[n_seg] float32, evm[n_seg] float64, NaN without a table); counts_dev (a device
        buffer of n_seg * bins * bins uint32) receives every segment's histogram.  engine = the producer, or None."""
        rms = np.empty(int(n_seg), dtype=np.float32)
        evm = np.empty(int(n_seg), dtype=np.float64)
        nat.check(nat.lib.tdsa_constellation_process_dev(self._h, engine._h if engine is not None else None, int(fmt),
                                                         C.c_void_p(ptr), int(seg_len), int(hop), int(n_seg), _p(rms),
                                                         _p(evm), C.c_void_p(counts_dev) if counts_dev else None))
        return rms, evm


class ConstellationView:
    """The data side of the reference's Constellation2D widget (same method names): a DataProcessor drives it as
    mw.constellation_2d_widget.  After update_iq_data: last_evm_rms, and `image` (density mode: np.log1p(hist).T,
    float64 [q_bin][i_bin]) or `scatter_xy` (scatter mode: the last max_points normalised (i, q))."""

    def __init__(self, device: int = 0, max_host_samples: int = 1 << 17):
        self._mode = "density"
        self._range = 1.5
        self._max_points = 2000
        self._modulation = "qpsk"
        self.last_evm_rms: Optional[float] = None
        self.image: Optional[np.ndarray] = None
        self.scatter_xy = None
        self._device = int(device)
        self._c = Constellation(max_host_samples, device, self._modulation, self._range)

    def set_mode(self, mode: str) -> None:
        if mode in ("density", "scatter"):
            self._mode = mode

    def set_modulation(self, mod: str) -> None:
        self._modulation = mod
        self._c.set_modulation(mod)

    def set_range(self, r: float) -> None:
        self._range = r

    def set_max_points(self, n: int) -> None:
        self._max_points = n

    def update_iq_data(self, samples) -> None:
        if samples is None or len(samples) == 0:
            return
        try:
            n = len(samples)
            if n > self._c.max_host_samples:           # a larger tick: a handle that stages it
                old = self._c
                self._c = Constellation(max(n, 2 * old.max_host_samples), self._device, self._modulation, old.range)
                old.close()
            density = self._mode == "density"
            start = slice(-min(self._max_points, n), None).indices(n)[0]   # i_data[-n:] of the reference
            range_error = None
            if density and float(self._range) != self._c.range:
                try:
                    self._c.set_range(self._range)
                except nat.TdsaError as e:             # the reference measures the EVM before histogram2d raises
                    range_error = e
            res = self._c.process(samples, n_tail=0 if density else n - start,
                                  counts=density and range_error is None)
            self.last_evm_rms = res.evm_rms
            if range_error is not None:
                raise range_error
            if density:
                self.image = res.image()
            else:
                self.scatter_xy = res.scatter()
        except Exception as e:
            _log.error(f"Constellation2D update error: {e}")
