"""Channel measurements on the device: channel power, ACPR, occupied bandwidth, x-dB width, limit mask (DESIGN.md
section 4.16).

What a spectrum analyser user reaches for once a signal is on screen.  Per float32 dB row in HBM, in one HIP pass
(tdsa_meas_*): the linear power, peak and NaN count of up to 16 channels (channel 0 is the main channel, the rest its
adjacent and alternate channels); the occupied bandwidth of a range by power fraction, its two edges interpolated
inside their bins; the x-dB width of the same range; and a pass / fail test of the whole row against a limit line,
absolute or relative to the main channel's peak.  A few dozen bytes per row come back; no row leaves the device.  The
detector's records (centre, width) are the natural input of the channel plan: channels_from_emission.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from ._inputs import _DbRows

MAX_BINS = 16384
MAX_CHANNELS = 16
FLAG_EMPTY, FLAG_INF, FLAG_MASK_FAIL = nat.MEAS_EMPTY, nat.MEAS_INF, nat.MEAS_MASK_FAIL

ROW_RECORD = np.dtype([("obw_total", np.float64), ("x_lo", np.float64), ("x_hi", np.float64), ("k_lo", np.int32),
                       ("k_hi", np.int32), ("xdb_lo", np.int32), ("xdb_hi", np.int32), ("peak_bin", np.int32),
                       ("n_nan", np.int32), ("n_fail", np.int32), ("worst_bin", np.int32), ("first_fail", np.int32),
                       ("last_fail", np.int32), ("flags", np.int32), ("peak_db", np.float32),
                       ("worst_margin", np.float32), ("reserved", np.int32)])
CHANNEL_RECORD = np.dtype([("power", np.float64), ("peak_db", np.float32), ("peak_bin", np.int32), ("n_nan", np.int32),
                           ("reserved", np.int32)])
assert ROW_RECORD.itemsize == 80 and CHANNEL_RECORD.itemsize == 24

ROW_FIELDS = tuple(f for f in ROW_RECORD.names if f != "reserved")


def _axis(freq_bins, n_min: int = 1) -> np.ndarray:
    f = np.asarray(freq_bins, dtype=np.float64)
    if f.ndim != 1 or f.size < n_min:
        raise ValueError(f"freq_bins of shape {f.shape}: one value per bin of the rows")
    return f


def _bin_width(f: np.ndarray) -> float:
    return float((f[-1] - f[0]) / max(f.size - 1, 1))


def channel_plan(freq_bins, centre_hz: float, bandwidth_hz: float, spacing_hz: Optional[float] = None,
                 n_adjacent: int = 0) -> List[Tuple[int, int]]:
    """The inclusive bin ranges of a main channel of bandwidth_hz around centre_hz and n_adjacent channels of the same
    bandwidth on either side, spacing_hz apart (default: the bandwidth): [(lo, hi), ...] in the order main, lower 1,
    upper 1, lower 2, upper 2, ...  A channel holds the bins MarkerManager._band_power would add up: bins >= f_lo and
    bins <= f_hi.  ValueError where a channel holds no bin or leaves the row."""
    f = _axis(freq_bins)
    bw, c = float(bandwidth_hz), float(centre_hz)
    sp = bw if spacing_hz is None else float(spacing_hz)
    if not (math.isfinite(bw) and bw > 0.0):
        raise ValueError(f"bandwidth_hz={bandwidth_hz}: finite and above 0")
    if not (math.isfinite(sp) and sp > 0.0):
        raise ValueError(f"spacing_hz={spacing_hz}: finite and above 0")
    if not math.isfinite(c):
        raise ValueError(f"centre_hz={centre_hz}: finite")
    if not 0 <= int(n_adjacent) <= (MAX_CHANNELS - 1) // 2:
        raise ValueError(f"n_adjacent={n_adjacent}: 0 .. {(MAX_CHANNELS - 1) // 2}")
    centres = [c]
    for k in range(1, int(n_adjacent) + 1):
        centres += [c - k * sp, c + k * sp]
    plan = []
    for cc in centres:
        f_lo, f_hi = cc - 0.5 * bw, cc + 0.5 * bw
        if f_lo < f[0] or f_hi > f[-1]:
            raise ValueError(f"channel {f_lo:.6g} .. {f_hi:.6g} Hz leaves the row's {f[0]:.6g} .. {f[-1]:.6g} Hz")
        idx = np.flatnonzero((f >= f_lo) & (f <= f_hi))
        if idx.size == 0:
            raise ValueError(f"channel {f_lo:.6g} .. {f_hi:.6g} Hz holds no bin")
        plan.append((int(idx[0]), int(idx[-1])))
    return plan


def limit_line(freq_bins, points: Sequence[Tuple[float, float]], centre_hz: float = 0.0) -> np.ndarray:
    """A limit line for the axis freq_bins from (offset Hz, dB) points, offsets relative to centre_hz and ascending:
    np.interp between the points, float32, NaN (not tested) outside them."""
    f = _axis(freq_bins)
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
        raise ValueError(f"points of shape {pts.shape}: (offset Hz, dB) pairs")
    if not np.all(np.isfinite(pts[:, 0])) or np.any(np.diff(pts[:, 0]) < 0):
        raise ValueError("points: offsets finite and ascending")
    x = f - float(centre_hz)
    out = np.interp(x, pts[:, 0], pts[:, 1]).astype(np.float32)
    out[(x < pts[0, 0]) | (x > pts[-1, 0])] = np.nan
    return out


def channels_from_emission(emission, freq_bins, spacing_hz: Optional[float] = None, n_adjacent: int = 0,
                           bandwidth_hz: Optional[float] = None) -> List[Tuple[int, int]]:
    """A channel plan from one entry of Detections.to_hz: the main channel around the emission's centre_hz, as wide as
    the emission (or bandwidth_hz), with n_adjacent channels on either side."""
    bw = float(emission["bandwidth_hz"]) if bandwidth_hz is None else float(bandwidth_hz)
    return channel_plan(freq_bins, float(emission["centre_hz"]), bw, spacing_hz, n_adjacent)


@dataclass
class Measurements:
    """One call's result.  The row fields (ROW_RECORD's, [n_rows] each) as attributes; channels: the channel records, a
    structured array [n_rows][C] (CHANNEL_RECORD); rows: the row records as the library gave them."""
    obw_total: np.ndarray
    x_lo: np.ndarray
    x_hi: np.ndarray
    k_lo: np.ndarray
    k_hi: np.ndarray
    xdb_lo: np.ndarray
    xdb_hi: np.ndarray
    peak_bin: np.ndarray
    n_nan: np.ndarray
    n_fail: np.ndarray
    worst_bin: np.ndarray
    first_fail: np.ndarray
    last_fail: np.ndarray
    flags: np.ndarray
    peak_db: np.ndarray
    worst_margin: np.ndarray
    channels: np.ndarray
    rows: np.ndarray

    def __len__(self) -> int:
        return int(self.rows.shape[0])

    @property
    def mask_failed(self) -> np.ndarray:
        """[n_rows] bool: the row has a bin above its limit."""
        return (self.flags & FLAG_MASK_FAIL) != 0

    def channel_power_db(self, bin_width: float) -> np.ndarray:
        """[n_rows][C]: 10 log10(max(power bin_width, 1e-30)), as MarkerManager._band_power forms it."""
        with np.errstate(all="ignore"):
            return 10.0 * np.log10(np.maximum(self.channels["power"] * float(bin_width), 1e-30))

    def acpr_db(self) -> np.ndarray:
        """[n_rows][C]: every channel's power against channel 0's, in dB (column 0 is 0)."""
        with np.errstate(all="ignore"):
            p = np.maximum(self.channels["power"], 1e-300)
            return 10.0 * np.log10(p / p[:, :1])

    def obw_hz(self, freq_bins, row: int = -1) -> Tuple[float, float]:
        """(width, centre) in Hz of a row's occupied bandwidth on the evenly spaced axis freq_bins: the positions x_lo
        and x_hi interpolated on it.  (NaN, NaN) for a row flagged EMPTY or INF."""
        f = _axis(freq_bins, int(max(self.k_hi[row], 0)) + 1)
        a, b = float(self.x_lo[row]), float(self.x_hi[row])
        if math.isnan(a) or math.isnan(b):
            return float("nan"), float("nan")
        bw = _bin_width(f)
        return (b - a) * bw, f[0] + 0.5 * (a + b) * bw

    def xdb_hz(self, freq_bins, row: int = -1) -> Tuple[float, float]:
        """(width, centre) in Hz of a row's x-dB width: (xdb_hi - xdb_lo + 1) bins around their middle.  (NaN, NaN)
        where the range holds no number."""
        f = _axis(freq_bins, int(max(self.xdb_hi[row], 0)) + 1)
        a, b = int(self.xdb_lo[row]), int(self.xdb_hi[row])
        if a < 0:
            return float("nan"), float("nan")
        bw = _bin_width(f)
        return (b - a + 1) * bw, f[0] + 0.5 * (a + b) * bw


def measurements_from(rows: np.ndarray, channels: np.ndarray) -> Measurements:
    return Measurements(*(rows[f].copy() for f in ROW_FIELDS), channels, rows)


class ChannelMeasure(_DbRows, nat._Handle, nat._Timer):
    """Channel power, occupied bandwidth, x-dB width and limit mask of [n_rows][n_bins] float32 dB rows, 1 <= n_bins <=
    16384.

    channels: [(lo, hi), ...], 1 .. 16 inclusive bin ranges, channel 0 the main channel (channel_plan makes them from
    frequencies).  obw=(lo, hi): the range of the occupied bandwidth and of the x-dB width (default: the whole row);
    fraction: the power fraction between the two edges; xdb: the depth of the x-dB width.  limit: float32 [n_bins] or
    None, NaN = bin not tested; limit_relative: the line is relative to channel 0's peak."""
    _destroy = "tdsa_meas_destroy"
    _timer = ("tdsa_meas_timer_begin", "tdsa_meas_timer_end")
    _process = ("tdsa_meas_process", "tdsa_meas_process_dev")
    _result = staticmethod(measurements_from)

    def __init__(self, n_bins: int, channels, obw: Optional[Tuple[int, int]] = None, fraction: float = 0.99,
                 xdb: float = 26.0, limit=None, limit_relative: bool = False, device: int = 0,
                 max_host_rows: Optional[int] = None):
        self.n_bins = int(n_bins)
        if not 1 <= self.n_bins <= MAX_BINS:
            raise ValueError(f"n_bins={n_bins}: 1 .. {MAX_BINS}")
        cfg = self._checked(channels, obw, fraction, xdb)
        lim = self._checked_limit(limit)
        self._stage(max_host_rows)
        self.device = int(device)
        self.limit, self.limit_relative = None, False
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_meas_create(self.device, self.n_bins, self.max_host_rows, C.byref(self._h)))
        self._apply(cfg)
        if lim is not None:
            self._apply_limit(lim, limit_relative)

    def _checked(self, channels, obw, fraction, xdb) -> dict:
        """The parameters as the library takes them; ValueError before it is called."""
        try:
            ch = [(int(a), int(b)) for a, b in channels]
        except (TypeError, ValueError):
            raise ValueError(f"channels={channels!r}: (lo, hi) pairs of bins") from None
        if not 1 <= len(ch) <= MAX_CHANNELS:
            raise ValueError(f"{len(ch)} channels: 1 .. {MAX_CHANNELS}")
        for c, (a, b) in enumerate(ch):
            if not 0 <= a <= b < self.n_bins:
                raise ValueError(f"channel {c}=({a}, {b}): 0 <= lo <= hi < {self.n_bins}")
        lo, hi = (0, self.n_bins - 1) if obw is None else (int(obw[0]), int(obw[1]))
        if not 0 <= lo <= hi < self.n_bins:
            raise ValueError(f"obw=({lo}, {hi}): 0 <= lo <= hi < {self.n_bins}")
        f, x = float(fraction), float(np.float32(xdb))
        if not (math.isfinite(f) and 0.0 < f < 1.0):
            raise ValueError(f"fraction={fraction}: above 0 and below 1")
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError(f"xdb={xdb}: finite and not negative")
        return dict(channels=ch, obw=(lo, hi), fraction=f, xdb=x)

    def _checked_limit(self, limit) -> Optional[np.ndarray]:
        if limit is None:
            return None
        a = np.asarray(limit)
        if a.dtype.kind not in "fiu" or a.shape != (self.n_bins,):
            raise ValueError(f"limit of dtype {a.dtype} and shape {a.shape}: [{self.n_bins}] real values")
        return np.ascontiguousarray(a, dtype=np.float32)

    def _apply(self, cfg: dict) -> None:
        n = len(cfg["channels"])
        lo = (C.c_int * n)(*[a for a, _ in cfg["channels"]])
        hi = (C.c_int * n)(*[b for _, b in cfg["channels"]])
        nat.check(nat.lib.tdsa_meas_configure(self._h, n, lo, hi, cfg["obw"][0], cfg["obw"][1], cfg["fraction"],
                                              cfg["xdb"]))
        self.__dict__.update(cfg)

    def _apply_limit(self, lim: Optional[np.ndarray], relative: bool) -> None:
        if lim is None:
            nat.check(nat.lib.tdsa_meas_set_limit(self._h, None, 0, 0))
            self.limit, self.limit_relative = None, False
        else:
            nat.check(nat.lib.tdsa_meas_set_limit(self._h, lim.ctypes.data_as(C.c_void_p), lim.size, int(bool(relative))))
            self.limit, self.limit_relative = lim.copy(), bool(relative)

    def configure(self, *, channels=None, obw: Optional[Tuple[int, int]] = None, fraction: Optional[float] = None,
                  xdb: Optional[float] = None) -> None:
        """New parameters for the calls that follow; what is not named stays.  The totals are not touched."""
        self._apply(self._checked(self.channels if channels is None else channels, self.obw if obw is None else obw,
                                  self.fraction if fraction is None else fraction, self.xdb if xdb is None else xdb))

    def set_limit(self, limit, relative: bool = False) -> None:
        """A new limit line (float32 [n_bins], NaN = bin not tested), absolute or relative to channel 0's peak; None
        removes it."""
        self._apply_limit(self._checked_limit(limit), relative)

    def _records(self, n_rows: int):
        return np.zeros(n_rows, dtype=ROW_RECORD), np.zeros((n_rows, len(self.channels)), dtype=CHANNEL_RECORD)

    def totals(self) -> Tuple[int, int]:
        """(rows seen, rows whose mask test failed) since the last reset."""
        seen, failed = C.c_uint64(), C.c_uint64()
        nat.check(nat.lib.tdsa_meas_read_totals(self._h, C.byref(seen), C.byref(failed)))
        return int(seen.value), int(failed.value)

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_meas_reset(self._h))
