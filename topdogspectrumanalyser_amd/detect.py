"""Signal detection on the device: noise floor, emissions, occupancy.

What the peak searches and the band power leave open: which emissions a row holds, where each starts and stops, how
strong it is, and how much of the time each bin was occupied.  Per float32 dB row in HBM: the noise floor as an order
statistic of the search range, a threshold `margin_db` above it, the runs of bins above the threshold (gaps of up to
`max_gap` bins bridged, runs narrower than `min_width` dropped), and per run its edges, peak, x-dB edges, linear power
and first moment - one HIP pass, tdsa_detect_*.  The handle also counts, per bin, the rows in which it was occupied.
The records are what the channelizer, the zoom front end, the demodulator and the symbol recovery ask for: a centre and
a bandwidth.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._inputs import _DbRows

MAX_BINS = 16384
MAX_SIGNALS = 64
FLAG_NAN_FLOOR = nat.DETECT_NAN_FLOOR

ROW_RECORD = np.dtype([("floor", np.float32), ("thr", np.float32), ("n_found", np.int32), ("n_over", np.int32),
                       ("flags", np.int32), ("reserved", np.int32, (3,))])
SIGNAL_RECORD = np.dtype([("start", np.int32), ("stop", np.int32), ("peak_bin", np.int32), ("x_lo", np.int32),
                          ("x_hi", np.int32), ("peak_db", np.float32), ("power", np.float64), ("moment", np.float64)])
assert ROW_RECORD.itemsize == 32 and SIGNAL_RECORD.itemsize == 40

EMISSION = np.dtype([("centre_hz", np.float64), ("bandwidth_hz", np.float64), ("xdb_bandwidth_hz", np.float64),
                     ("power_db", np.float64), ("peak_db", np.float32), ("peak_hz", np.float64),
                     ("start", np.int32), ("stop", np.int32)])


def quantile_rank(q: float, n_eff: int) -> int:
    """The order statistic a quantile names among n_eff bins: min(n_eff - 1, floor(q (n_eff - 1) + 0.5))."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"floor_quantile={q}: 0 .. 1")
    return int(min(n_eff - 1, math.floor(q * (n_eff - 1) + 0.5)))


@dataclass
class Detections:
    """One call's result.  floor, thr (float32), n_found, n_over, flags (int32): [n_rows]; signals: the signal records,
    a structured array [n_rows][max_signals] (SIGNAL_RECORD), rows padded with start = -1; rows: the row records as the
    library gave them."""
    floor: np.ndarray
    thr: np.ndarray
    n_found: np.ndarray
    n_over: np.ndarray
    flags: np.ndarray
    signals: np.ndarray
    rows: np.ndarray

    def __len__(self) -> int:
        return int(self.rows.shape[0])

    def count(self, row: int = -1) -> int:
        """Signals of a row that have a record: min(n_found, max_signals)."""
        return int(min(int(self.n_found[row]), self.signals.shape[1]))

    def to_hz(self, freq_bins, row: int = -1) -> np.ndarray:
        """A row's signals on the frequency axis `freq_bins` ([n_bins], evenly spaced): centre_hz interpolated at bin
        position start + moment / power, bandwidth_hz = (stop - start + 1) bin_width, the x-dB width the same way,
        power_db = 10 log10(max(power bin_width, 1e-30)) as MarkerManager._band_power forms it, peak_db / peak_hz."""
        f = np.asarray(freq_bins, dtype=np.float64)
        s = self.signals[row][:self.count(row)]
        if f.ndim != 1 or (s.size and f.size <= int(s["stop"].max())):
            raise ValueError(f"freq_bins of shape {f.shape}: one value per bin of the rows")
        bin_width = (f[-1] - f[0]) / max(f.size - 1, 1)
        out = np.zeros(s.size, dtype=EMISSION)
        with np.errstate(all="ignore"):
            pos = s["start"] + np.where(s["power"] > 0, s["moment"] / np.where(s["power"] > 0, s["power"], 1.0), 0.0)
            out["centre_hz"] = np.interp(pos, np.arange(f.size, dtype=np.float64), f)
            out["bandwidth_hz"] = (s["stop"] - s["start"] + 1) * bin_width
            out["xdb_bandwidth_hz"] = (s["x_hi"] - s["x_lo"] + 1) * bin_width
            out["power_db"] = 10.0 * np.log10(np.maximum(s["power"] * bin_width, 1e-30))
        out["peak_db"] = s["peak_db"]
        out["peak_hz"] = f[s["peak_bin"]] if s.size else 0.0
        out["start"], out["stop"] = s["start"], s["stop"]
        return out


def detections_from(rows: np.ndarray, signals: np.ndarray) -> Detections:
    return Detections(rows["floor"].copy(), rows["thr"].copy(), rows["n_found"].copy(), rows["n_over"].copy(),
                      rows["flags"].copy(), signals, rows)


class SignalDetector(_DbRows, nat._Handle, nat._Timer):
    """Emissions of [n_rows][n_bins] float32 dB rows, 1 <= n_bins <= 16384.

    floor_quantile: which order statistic of the search range is the noise floor (0.5: the median); rank= names it
    directly.  bins=(lo, hi): the inclusive search range (default: the whole row).  margin_db above the floor is the
    threshold; gaps of up to max_gap bins are bridged, runs narrower than min_width dropped; xdb is the depth of the
    x-dB width; max_signals records per row (1 .. 64)."""
    _destroy = "tdsa_detect_destroy"
    _timer = ("tdsa_detect_timer_begin", "tdsa_detect_timer_end")
    _process = ("tdsa_detect_process", "tdsa_detect_process_dev")
    _result = staticmethod(detections_from)

    def __init__(self, n_bins: int, *, floor_quantile: float = 0.5, margin_db: float = 10.0, min_width: int = 1,
                 max_gap: int = 0, xdb: float = 3.0, max_signals: int = 16, bins: Optional[Tuple[int, int]] = None,
                 rank: Optional[int] = None, device: int = 0, max_host_rows: Optional[int] = None):
        self.n_bins = int(n_bins)
        if not 1 <= self.n_bins <= MAX_BINS:
            raise ValueError(f"n_bins={n_bins}: 1 .. {MAX_BINS}")
        cfg = self._checked(floor_quantile, margin_db, min_width, max_gap, xdb, max_signals, bins, rank)
        self._stage(max_host_rows)
        self.device = int(device)
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_detect_create(self.device, self.n_bins, self.max_host_rows, C.byref(self._h)))
        self._apply(cfg)

    def _checked(self, floor_quantile, margin_db, min_width, max_gap, xdb, max_signals, bins, rank) -> dict:
        """The parameters as the library takes them; ValueError before it is called."""
        lo, hi = (0, self.n_bins - 1) if bins is None else (int(bins[0]), int(bins[1]))
        if not 0 <= lo <= hi < self.n_bins:
            raise ValueError(f"bins=({lo}, {hi}): 0 <= lo <= hi < {self.n_bins}")
        n_eff = hi - lo + 1
        r = quantile_rank(floor_quantile, n_eff) if rank is None else int(rank)
        if not 0 <= r < n_eff:
            raise ValueError(f"rank={rank}: 0 .. {n_eff - 1}")
        margin, x = float(np.float32(margin_db)), float(np.float32(xdb))
        if not math.isfinite(margin):
            raise ValueError(f"margin_db={margin_db}: finite")
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError(f"xdb={xdb}: finite and not negative")
        if not 1 <= int(min_width) <= self.n_bins:
            raise ValueError(f"min_width={min_width}: 1 .. {self.n_bins}")
        if not 0 <= int(max_gap) <= self.n_bins:
            raise ValueError(f"max_gap={max_gap}: 0 .. {self.n_bins}")
        if not 1 <= int(max_signals) <= MAX_SIGNALS:
            raise ValueError(f"max_signals={max_signals}: 1 .. {MAX_SIGNALS}")
        return dict(bins=(lo, hi), n_eff=n_eff, rank=r, margin_db=margin, xdb=x, min_width=int(min_width),
                    max_gap=int(max_gap), max_signals=int(max_signals), floor_quantile=float(floor_quantile))

    def _apply(self, cfg: dict) -> None:
        nat.check(nat.lib.tdsa_detect_configure(self._h, cfg["bins"][0], cfg["bins"][1], cfg["rank"], cfg["margin_db"],
                                                cfg["min_width"], cfg["max_gap"], cfg["xdb"], cfg["max_signals"]))
        self.__dict__.update(cfg)

    def configure(self, *, floor_quantile: Optional[float] = None, margin_db: Optional[float] = None,
                  min_width: Optional[int] = None, max_gap: Optional[int] = None, xdb: Optional[float] = None,
                  max_signals: Optional[int] = None, bins: Optional[Tuple[int, int]] = None,
                  rank: Optional[int] = None) -> None:
        """New parameters for the calls that follow; what is not named stays (a rank given as a quantile follows a new
        range).  The occupancy counts are not touched: reset() them when the threshold's meaning changes."""
        keep = rank is None and floor_quantile is None and bins is None
        self._apply(self._checked(
            self.floor_quantile if floor_quantile is None else floor_quantile,
            self.margin_db if margin_db is None else margin_db, self.min_width if min_width is None else min_width,
            self.max_gap if max_gap is None else max_gap, self.xdb if xdb is None else xdb,
            self.max_signals if max_signals is None else max_signals, self.bins if bins is None else bins,
            self.rank if keep else rank))

    def _records(self, n_rows: int):
        return np.zeros(n_rows, dtype=ROW_RECORD), np.zeros((n_rows, self.max_signals), dtype=SIGNAL_RECORD)

    def occupancy(self) -> Tuple[np.ndarray, int, int]:
        """(counts uint32 [n_bins], rows seen, rows flagged) since the last reset: counts[i] rows had bin i above their
        threshold; flagged rows (a NaN floor) add to no bin."""
        counts = np.zeros(self.n_bins, dtype=np.uint32)
        seen, flagged = C.c_uint64(), C.c_uint64()
        nat.check(nat.lib.tdsa_detect_read_occupancy(self._h, counts.ctypes.data_as(C.c_void_p), C.byref(seen),
                                                     C.byref(flagged)))
        return counts, int(seen.value), int(flagged.value)

    def reset(self) -> None:
        nat.check(nat.lib.tdsa_detect_reset(self._h))
