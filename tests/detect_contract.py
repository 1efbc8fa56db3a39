"""The signal detection's contract in numpy: what tdsa_detect_* computes for one float32 dB row,
step by step.  The floor is an order statistic (an exact float32 of the row), the threshold one float32 addition, the
runs integer; only the two power sums carry a tolerance (POWER_RTOL, the figure tests/test_gpu_analytics.py holds for
the same expression: exp10f on the device, float32 10 ** x here, a float64 sum)."""
import numpy as np

ROW = np.dtype([("floor", "<f4"), ("thr", "<f4"), ("n_found", "<i4"), ("n_over", "<i4"), ("flags", "<i4"),
                ("reserved", "<i4", (3,))])
SIGNAL = np.dtype([("start", "<i4"), ("stop", "<i4"), ("peak_bin", "<i4"), ("x_lo", "<i4"), ("x_hi", "<i4"),
                   ("peak_db", "<f4"), ("power", "<f8"), ("moment", "<f8")])
FLAG_NAN_FLOOR = 1
MAX_BINS = 16384
MAX_SIGNALS = 64
POWER_RTOL = 1e-6


def keys(x):
    """float32 -> uint32 keys that sort as np.sort sorts the values: the sign bit flipped for non-negatives, every bit
    for negatives, and every NaN (of either sign) the largest key.  +0 and -0 get different keys."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == np.uint32(0xFFFFFFFF), np.float32(np.nan), b.view(np.float32))


def rank_of(q, n_eff):
    """The integer rank of a quantile: min(n_eff - 1, floor(q (n_eff - 1) + 0.5))."""
    return int(min(n_eff - 1, np.floor(float(q) * (n_eff - 1) + 0.5)))


def padding(S):
    rec = np.zeros(S, dtype=SIGNAL)
    for f in ("start", "stop", "peak_bin", "x_lo", "x_hi"):
        rec[f] = -1
    rec["peak_db"] = np.nan
    return rec


def runs_of(mask, max_gap, min_width):
    """(start, stop) of the runs of a boolean mask, inclusive and relative to it: set bins more than max_gap + 1 apart
    end one run and begin the next, then runs narrower than min_width (bridged bins counted) are dropped."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    brk = np.flatnonzero(np.diff(idx) > max_gap + 1)
    start = idx[np.concatenate(([0], brk + 1))]
    stop = idx[np.concatenate((brk, [idx.size - 1]))]
    keep = stop - start + 1 >= min_width
    return np.stack([start[keep], stop[keep]], axis=1)


def linear(v):
    """p_i: float32 10 ** (v / 10), widened."""
    with np.errstate(all="ignore"):
        return (np.float32(10.0) ** (np.asarray(v, dtype=np.float32) / np.float32(10.0))).astype(np.float64)


def detect_row(row, lo, hi, rank, margin_db, min_width=1, max_gap=0, xdb=3.0, S=16):
    """One row: (row record, [S] signal records, the boolean mask over the whole row)."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    assert 0 <= lo <= hi < row.size and 0 <= rank <= hi - lo and 1 <= S <= MAX_SIGNALS
    seg = row[lo:hi + 1]
    rr = np.zeros((), dtype=ROW)
    sig = padding(S)
    full = np.zeros(row.size, dtype=bool)
    floor = np.sort(seg)[rank]
    rr["floor"] = floor
    if np.isnan(floor):
        rr["thr"] = np.nan
        rr["flags"] = FLAG_NAN_FLOOR
        return rr, sig, full
    with np.errstate(all="ignore"):
        thr = np.float32(floor) + np.float32(margin_db)
        m = seg > thr
    rr["thr"] = thr
    rr["n_over"] = int(m.sum())
    full[lo:hi + 1] = m
    runs = runs_of(m, max_gap, min_width) + lo
    rr["n_found"] = len(runs)
    for k, (a, b) in enumerate(runs[:S]):
        v = row[a:b + 1]
        ok = ~np.isnan(v)
        peak = np.max(v[ok])
        with np.errstate(all="ignore"):
            edge = np.float32(peak) - np.float32(xdb)
            at = np.flatnonzero(v >= edge)
        p = np.where(ok, linear(np.where(ok, v, 0)), 0.0)
        with np.errstate(all="ignore"):                               # a +inf bin: 0 * inf at the run's first bin
            moment = (np.arange(v.size, dtype=np.float64) * p).sum()
        sig[k] = (a, b, a + int(np.flatnonzero(v == peak)[0]), a + at[0], a + at[-1], peak, p.sum(), moment)
    return rr, sig, full


def detect(rows, lo, hi, rank, margin_db, min_width=1, max_gap=0, xdb=3.0, S=16):
    """Rows [n_rows][n_bins]: (row records [n_rows], signal records [n_rows][S], occupancy uint32 [n_bins], rows seen,
    rows flagged)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float32))
    rr = np.zeros(rows.shape[0], dtype=ROW)
    sig = np.zeros((rows.shape[0], S), dtype=SIGNAL)
    occ = np.zeros(rows.shape[1], dtype=np.uint32)
    for r, row in enumerate(rows):
        rr[r], sig[r], m = detect_row(row, lo, hi, rank, margin_db, min_width, max_gap, xdb, S)
        occ += m
    return rr, sig, occ, rows.shape[0], int(np.count_nonzero(rr["flags"]))


def planted_row(n=1000, seed=1):
    """The row of the issue's check: noise around -100 dB, a 40-bin signal that holds a NaN, three single-bin spikes 3
    and 7 bins apart, and a signal that touches the last bin.  Returns (row, the planted (start, stop) pairs)."""
    rng = np.random.default_rng(seed)
    row = (-100.0 + rng.standard_normal(n)).astype(np.float32)
    row[200:240] = -60.0 + rng.standard_normal(40).astype(np.float32)
    row[220] = np.nan
    for b in (500, 503, 510):
        row[b] = -55.0
    row[n - 12:] = -65.0
    return row, [(200, 239), (500, 500), (503, 503), (510, 510), (n - 12, n - 1)]
