"""The channel measurements' contract in numpy: what tdsa_meas_* computes for one float32 dB
row, step by step.  Peaks, NaN counts, the x-dB edges and every figure of the limit test are exact (float32 compares and
one float32 subtraction or addition); the power sums carry POWER_RTOL, the figure tests/detect_contract.py holds for the
same expression (exp10f on the device, float32 10 ** x here, a float64 sum).

Throughout p_i = float32 10 ** (row[i] / 10) widened to float64, 0 for a NaN bin.  A caller that has the device's own
p_i (a channel of one bin returns it) passes them as `p`: the sums are then those of the same terms."""
import numpy as np

from detect_contract import POWER_RTOL, linear  # noqa: F401

ROW = np.dtype([("obw_total", "<f8"), ("x_lo", "<f8"), ("x_hi", "<f8"), ("k_lo", "<i4"), ("k_hi", "<i4"),
                ("xdb_lo", "<i4"), ("xdb_hi", "<i4"), ("peak_bin", "<i4"), ("n_nan", "<i4"), ("n_fail", "<i4"),
                ("worst_bin", "<i4"), ("first_fail", "<i4"), ("last_fail", "<i4"), ("flags", "<i4"), ("peak_db", "<f4"),
                ("worst_margin", "<f4"), ("reserved", "<i4")])
CHANNEL = np.dtype([("power", "<f8"), ("peak_db", "<f4"), ("peak_bin", "<i4"), ("n_nan", "<i4"), ("reserved", "<i4")])
FLAG_EMPTY, FLAG_INF, FLAG_MASK_FAIL = 1, 2, 4
MAX_BINS = 16384
MAX_CHANNELS = 16
f32 = np.float32


def powers(row, p=None):
    """p_i of a row: 0 where the bin is a NaN."""
    row = np.asarray(row, dtype=f32)
    ok = ~np.isnan(row)
    if p is None:
        p = linear(np.where(ok, row, f32(0.0)))
    return np.where(ok, np.asarray(p, dtype=np.float64), 0.0)


def peak_of(v, offset=0):
    """(peak_db, peak_bin): the largest non-NaN value and the first bin that holds it; (NaN, -1) if there is none."""
    v = np.asarray(v, dtype=f32)
    ok = ~np.isnan(v)
    if not ok.any():
        return f32(np.nan), -1
    at = int(np.flatnonzero(v == np.max(v[ok]))[0])
    return v[at], offset + at


def channel(row, lo, hi, p=None):
    """One channel's record (p: the row's powers(), where the caller has them)."""
    row = np.asarray(row, dtype=f32)
    assert 0 <= lo <= hi < row.size
    rec = np.zeros((), dtype=CHANNEL)
    seg = row[lo:hi + 1]
    with np.errstate(all="ignore"):
        rec["power"] = (powers(row) if p is None else p)[lo:hi + 1].sum()
    rec["peak_db"], rec["peak_bin"] = peak_of(seg, lo)
    rec["n_nan"] = int(np.isnan(seg).sum())
    return rec


def crossing(S, pw, t, lo):
    """(k, x) of the target t on the inclusive prefix sums S of the powers pw, both over the range that starts at bin
    lo: the first k with S[k] >= t, and x = k - 1/2 + (t - S[k - 1]) / p_k with S[lo - 1] = 0."""
    j = int(np.searchsorted(S, t, side="left"))
    assert j < S.size
    below = S[j - 1] if j > 0 else 0.0
    k = lo + j
    return k, (k - 0.5) + ((t - below) / pw[j] if pw[j] > 0 else 0.0)


def cumulative(S, lo, x):
    """C(x): the piecewise-linear cumulative power of a range that starts at bin lo, with C(k + 1/2) = S[k]."""
    edges = lo - 0.5 + np.arange(S.size + 1)
    return float(np.interp(x, edges, np.concatenate(([0.0], S))))


def measure_row(row, channels, obw, fraction, xdb, limit=None, relative=False, p=None):
    """One row: (row record, [C] channel records)."""
    row = np.ascontiguousarray(row, dtype=f32)
    n = row.size
    lo, hi = obw
    assert 1 <= len(channels) <= MAX_CHANNELS and 0 <= lo <= hi < n and 0.0 < fraction < 1.0 and xdb >= 0
    ch = np.zeros(len(channels), dtype=CHANNEL)
    pw_row = powers(row, p)
    for c, (a, b) in enumerate(channels):
        ch[c] = channel(row, a, b, pw_row)
    rr = np.zeros((), dtype=ROW)
    # occupied bandwidth
    seg = row[lo:hi + 1]
    pw = pw_row[lo:hi + 1]
    with np.errstate(all="ignore"):
        S = np.cumsum(pw)
    T = S[-1]
    rr["obw_total"] = T
    rr["n_nan"] = int(np.isnan(seg).sum())
    rr["k_lo"] = rr["k_hi"] = -1
    rr["x_lo"] = rr["x_hi"] = np.nan
    flags = 0
    if not T > 0:
        flags = FLAG_EMPTY
    elif np.isinf(T):
        flags = FLAG_INF
    else:
        f = float(fraction)
        t_lo, t_hi = T * (1.0 - f) / 2.0, T * (1.0 + f) / 2.0
        rr["k_lo"], rr["x_lo"] = crossing(S, pw, t_lo, lo)
        rr["k_hi"], rr["x_hi"] = crossing(S, pw, t_hi, lo)
    # x-dB width of the same range
    rr["peak_db"], rr["peak_bin"] = peak_of(seg, lo)
    rr["xdb_lo"] = rr["xdb_hi"] = -1
    if rr["peak_bin"] >= 0:
        with np.errstate(all="ignore"):
            edge = f32(f32(rr["peak_db"]) - f32(xdb))
            at = np.flatnonzero(seg >= edge)
        rr["xdb_lo"], rr["xdb_hi"] = lo + at[0], lo + at[-1]
    # limit line
    rr["worst_bin"] = rr["first_fail"] = rr["last_fail"] = -1
    rr["worst_margin"] = np.nan
    if limit is not None:
        limit = np.asarray(limit, dtype=f32)
        assert limit.shape == (n,)
        with np.errstate(all="ignore"):
            lim = (limit + f32(ch[0]["peak_db"])).astype(f32) if relative else limit
            fails = np.flatnonzero(row > lim)
            margin = (row - lim).astype(f32)
        rr["n_fail"] = fails.size
        if fails.size:
            rr["first_fail"], rr["last_fail"] = fails[0], fails[-1]
            flags |= FLAG_MASK_FAIL
        rr["worst_margin"], rr["worst_bin"] = peak_of(margin)
    rr["flags"] = flags
    return rr, ch


def measure(rows, channels, obw, fraction, xdb, limit=None, relative=False, p=None):
    """Rows [n_rows][n_bins]: (row records [n_rows], channel records [n_rows][C])."""
    rows = np.atleast_2d(np.asarray(rows, dtype=f32))
    rr = np.zeros(rows.shape[0], dtype=ROW)
    ch = np.zeros((rows.shape[0], len(channels)), dtype=CHANNEL)
    for r, row in enumerate(rows):
        rr[r], ch[r] = measure_row(row, channels, obw, fraction, xdb, limit, relative, None if p is None else p[r])
    return rr, ch


def raised_cosine_row(n=2048, centre=1000, half=200, top=-30.0, floor=-300.0):
    """A row whose only power is a raised-cosine emission: linear power cos^2 over centre - half .. centre + half, the
    rest at `floor` dB (1e-30 of nothing).  Returns (row, the emission's linear powers in float64)."""
    k = np.arange(-half, half + 1)
    shape = np.cos(0.5 * np.pi * k / (half + 1)) ** 2
    row = np.full(n, floor, dtype=f32)
    row[centre + k] = (top + 10.0 * np.log10(shape)).astype(f32)
    return row, 10.0 ** (top / 10.0) * shape


def acpr_row(n=1024, main=(400, 499), adj=((300, 399), (500, 599)), main_db=-20.0, acpr_db=-40.0, floor=-200.0):
    """A row with a flat main channel and flat adjacent channels acpr_db below it, bin for bin."""
    row = np.full(n, floor, dtype=f32)
    row[main[0]:main[1] + 1] = main_db
    for a, b in adj:
        row[a:b + 1] = main_db + acpr_db
    return row
