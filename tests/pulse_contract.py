"""The contract of the pulse analysis (tdsa_pulse_*) in numpy: what the device must return.  The
integer fields - toa, width, peak_index, peak_bits, flags, the summary, which pulses are stored - bit for bit, for any
split of a stream into calls: feed() may be called once or many times.  energy, acc_re and acc_im are float64 sums whose
order of addition the device is free in; here they are math.fsum, the correctly rounded sum, and within_bounds() is the
distance the device may keep from it."""
import math

import numpy as np

from pstat_contract import C64, I8, U8, power, unpack  # noqa: F401  (the same samples, the same power)

RECORD = np.dtype([("toa", np.int64), ("width", np.int64), ("peak_index", np.int64), ("peak_bits", np.uint32),
                   ("flags", np.uint32), ("energy", np.float64), ("acc_re", np.float64), ("acc_im", np.float64),
                   ("reserved", np.uint64)])
COUNTS = ("n_total", "n_on", "n_pulses", "n_short", "n_lost", "n_nan")
SUMMARY = np.dtype([(f, np.uint64) for f in COUNTS] + [("open_toa", np.int64), ("open_width", np.int64),
                                                        ("open", np.int32), ("reserved", np.int32)])
INTEGER_FIELDS = ("toa", "width", "peak_index", "peak_bits", "flags")
FLAG_INF = 1
A, B, C = 1, 2, 0


def classes(p, on_level, off_level):
    """A = 1: p >= on_level.  B = 2: p < off_level, or NaN.  C = 0: anything else.  float32 compares."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = p >= np.float32(on_level)
        b = (p < np.float32(off_level)) | np.isnan(p)
    return np.where(a, A, np.where(b, B, C)).astype(np.int8)


def states(code, on_before):
    """[n] bool: the state at every sample: the class of the last sample up to it that is not C, else the state before."""
    n = code.size
    idx = np.where(code != C, np.arange(n), -1)
    last = np.maximum.accumulate(idx) if n else idx
    return np.where(last >= 0, code[np.maximum(last, 0)] == A, bool(on_before))


def _fsum(parts):
    try:
        return math.fsum(np.concatenate(parts).tolist())
    except (ValueError, OverflowError):       # inf - inf: unspecified by the contract
        return math.nan


class Stream:
    """One stream's state across calls."""

    def __init__(self, on_level, off_level=None, min_width=1, capacity=1 << 22):
        self.on_level = np.float32(on_level)
        self.off_level = self.on_level if off_level is None else np.float32(off_level)
        assert 0 < self.off_level <= self.on_level < np.inf and 1 <= min_width < 1 << 31 and capacity >= 1
        self.min_width, self.capacity = int(min_width), int(capacity)
        self.sum = {f: 0 for f in COUNTS}
        self.on = False
        self.prev = (np.float32(0), np.float32(0))
        self.open = None                       # toa, width, peak_bits, peak_index, flags, and the terms of the three sums
        self.pulses = []                       # the stored ones, as tuples in RECORD's order

    # a stretch of on samples as the pieces a pulse is joined from
    @staticmethod
    def _piece(toa, p, tre, tim):
        bits = p.view(np.uint32)
        k = int(np.argmax(bits))               # the first index that attains the maximum
        return dict(toa=toa, width=p.size, peak_bits=int(bits[k]), peak_index=toa + k,
                    flags=FLAG_INF if np.isinf(p).any() else 0, e=[p.astype(np.float64)], re=[tre], im=[tim])

    @staticmethod
    def _join(a, b):
        later = b["peak_bits"] > a["peak_bits"]
        return dict(toa=a["toa"], width=a["width"] + b["width"], peak_bits=b["peak_bits"] if later else a["peak_bits"],
                    peak_index=b["peak_index"] if later else a["peak_index"], flags=a["flags"] | b["flags"],
                    e=a["e"] + b["e"], re=a["re"] + b["re"], im=a["im"] + b["im"])

    def _complete(self, q):
        if q["width"] < self.min_width:
            self.sum["n_short"] += 1
            return
        k = self.sum["n_pulses"]
        self.sum["n_pulses"] += 1
        if k >= self.capacity:
            self.sum["n_lost"] += 1
            return
        self.pulses.append((q["toa"], q["width"], q["peak_index"], q["peak_bits"], q["flags"], _fsum(q["e"]), _fsum(q["re"]),
                            _fsum(q["im"]), 0))

    def feed(self, samples, fmt):
        return self.feed_iq(*unpack(samples, fmt))

    def feed_iq(self, re, im):
        re, im = np.ascontiguousarray(re, dtype=np.float32), np.ascontiguousarray(im, dtype=np.float32)
        n, n0 = re.size, self.sum["n_total"]
        if n == 0:
            return self
        p = power(re, im)
        code = classes(p, self.on_level, self.off_level)
        on = states(code, self.on)
        self.sum["n_total"] += n
        self.sum["n_on"] += int(np.count_nonzero(on))
        self.sum["n_nan"] += int(np.count_nonzero(np.isnan(p)))
        r = np.concatenate([[self.prev[0]], re]).astype(np.float64)
        i = np.concatenate([[self.prev[1]], im]).astype(np.float64)
        with np.errstate(all="ignore"):        # term k: x[k] conj(x[k - 1]), the products exact in float64
            tre = r[1:] * r[:-1] + i[1:] * i[:-1]
            tim = i[1:] * r[:-1] - r[1:] * i[:-1]
        d = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
        starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        if self.open is not None and not on[0]:
            self._complete(self.open)
            self.open = None
        for s, e in zip(starts.tolist(), ends.tolist()):
            if s == 0 and self.open is not None:
                q = self._join(self.open, self._piece(n0, p[:e], tre[:e], tim[:e]))
                self.open = None
            else:
                q = self._piece(n0 + s, p[s:e], tre[s + 1:e], tim[s + 1:e])
            if e < n:                          # the sample behind it is off, and only a B sample switches off
                self._complete(q)
            else:
                self.open = q
        self.on = bool(on[-1])
        self.prev = (re[-1], im[-1])
        return self

    def summary(self):
        out = np.zeros((), dtype=SUMMARY)
        for f in COUNTS:
            out[f] = self.sum[f]
        if self.open is not None:
            out["open"], out["open_toa"], out["open_width"] = 1, self.open["toa"], self.open["width"]
        return out

    def records(self):
        return np.array(self.pulses, dtype=RECORD)


def run(streams, fmt, on_level, off_level=None, min_width=1, capacity=1 << 22):
    """[C] Stream, each stream given whole."""
    return [Stream(on_level, off_level, min_width, capacity).feed(s, fmt) for s in streams]


def within_bounds(got, want):
    """The first violation as a string, or None: the integer fields equal; |energy - fsum| <= width 2^-52 energy, twice
    the first-order bound of width - 1 additions of non-negative terms in any order; |acc - fsum| <= width 2^-50 energy:
    the sum of |term| is at most the energy up to p's float32 rounding, and the factor 4 covers that and each term's own
    rounding.  A pulse with an infinite sample: energy +inf, acc_* unspecified."""
    if got.shape != want.shape:
        return f"{got.shape[0]} records, the contract has {want.shape[0]}"
    for f in INTEGER_FIELDS:
        if not np.array_equal(got[f], want[f]):
            k = int(np.flatnonzero(got[f] != want[f])[0])
            return f"{f}[{k}] = {got[f][k]}, the contract has {want[f][k]}"
    inf = (want["flags"] & FLAG_INF) != 0
    if not np.array_equal(got["energy"][inf], want["energy"][inf]):
        return "energy of a pulse with an infinite sample is not +inf"
    g, w = got[~inf], want[~inf]
    width = w["width"].astype(np.float64)
    bad = np.flatnonzero(~(np.abs(g["energy"] - w["energy"]) <= width * 2.0 ** -52 * w["energy"]))
    if bad.size:
        return f"energy[{bad[0]}] = {g['energy'][bad[0]]!r}, the contract has {w['energy'][bad[0]]!r} (width {w['width'][bad[0]]})"
    for f in ("acc_re", "acc_im"):
        bad = np.flatnonzero(~(np.abs(g[f] - w[f]) <= width * 2.0 ** -50 * w["energy"]))
        if bad.size:
            return f"{f}[{bad[0]}] = {g[f][bad[0]]!r}, the contract has {w[f][bad[0]]!r} (width {w['width'][bad[0]]})"
    return None
