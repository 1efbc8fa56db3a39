"""Zero span, restated in numpy (include/tdsa_hip.h, tdsa_zspan_*).

Everything here works on the WHOLE detected history e[0 : total] with absolute indices: the ring of the device is
`history[base:]`, and a test that keeps the full history never has to model the wrap.  The float32 restatement of the
detectors is what the kernels compute operation by operation; the float64 forms are what their tolerances refer to.
"""
import numpy as np

F32 = np.float32
LOG2_TO_DB = F32(3.0102999566398120)          # float32(10 / log2(10))


# ---------------------------------------------------------------------------------------------------- the recorded run
def golden_ticks(path):
    """(rate, [dict(raw, block, mode, level, window, shown)]) of the recorded run."""
    z = np.load(path)
    rate = float(z["rate"])
    raw_at = np.concatenate([[0], np.cumsum(2 * z["block_len"])])
    shown_at = np.concatenate([[0], np.cumsum(z["shown_len"])])
    ticks = []
    for i in range(len(z["block_len"])):
        raw = z["raw"][raw_at[i]:raw_at[i + 1]]
        v = raw.reshape(-1, 2).astype(np.float32) / np.float32(128.0)
        ticks.append(dict(raw=raw, block=(v[:, 0] + 1j * v[:, 1]).astype(np.complex64), mode=str(z["modes"][i]),
                          level=float(z["levels"][i]), window=float(z["windows"][i]),
                          shown=z["shown_i8"][shown_at[i]:shown_at[i + 1]].astype(np.float32) / np.float32(128.0)))
    return rate, ticks


# ---------------------------------------------------------------------------------------------------- samples
def unpack(samples, fmt):
    """(re, im) float32 of one block.  fmt: "i8" (I + jQ) / 128; "u8" (float32(u) - 127.5) * float32(1 / 127.5), the
    frame kernels' unpack; "c64" as is; "f32r" real float32 (im = 0)."""
    a = np.asarray(samples)
    if fmt == "i8":
        v = a.reshape(-1, 2).astype(F32) * F32(1.0 / 128.0)
        return v[:, 0].copy(), v[:, 1].copy()
    if fmt == "u8":
        v = (a.reshape(-1, 2).astype(F32) - F32(127.5)) * (F32(1.0) / F32(127.5))
        return v[:, 0].copy(), v[:, 1].copy()
    if fmt == "c64":
        a = a.reshape(-1).astype(np.complex64)
        return a.real.copy(), a.imag.copy()
    if fmt == "f32r":
        a = a.reshape(-1).astype(F32)
        return a, np.zeros_like(a)
    raise ValueError(fmt)


def detect(re, im, detector="real", log_floor=0.0, offset_db=0.0):
    """float32 e per sample, every operation rounded to float32 (what the push kernel does)."""
    re, im = np.asarray(re, dtype=F32), np.asarray(im, dtype=F32)
    if detector == "real":
        return re.copy()
    p = re * re + im * im
    if detector == "mag":
        return np.sqrt(p)
    if detector == "db":
        return np.log2(p + F32(log_floor)) * LOG2_TO_DB + F32(offset_db)
    raise ValueError(detector)


def detect64(re, im, detector="real", log_floor=0.0, offset_db=0.0):
    """The float64 formulas the MAG and DB tolerances are stated against."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    if detector == "real":
        return re.copy()
    if detector == "mag":
        return np.hypot(re, im)
    return 10.0 * np.log10(re * re + im * im + float(F32(log_floor))) + float(F32(offset_db))


# ---------------------------------------------------------------------------------------------------- ring and view
def view_plan(total, capacity, n_display, mode):
    """The host half: dict(held, base, length, free_start, search) with search = (ss, se) ring-relative or None."""
    total, capacity, n_display = int(total), int(capacity), int(n_display)
    held = min(total, capacity)
    base = total - held
    if held < n_display:
        return dict(held=held, base=base, length=held, free_start=base, search=None)
    search = None
    if mode != "free_run":
        se = held - n_display
        ss = max(0, se - 8 * n_display)
        if se - 2 >= ss:
            search = (ss, se)
    return dict(held=held, base=base, length=n_display, free_start=total - n_display, search=search)


def view(history, capacity, n_display, mode="free_run", level=0.0):
    """(start, triggered, chunk) over the full detected history (absolute indices)."""
    e = np.asarray(history, dtype=F32)
    plan = view_plan(e.size, capacity, n_display, mode)
    start, triggered = plan["free_start"], 0
    if plan["search"] is not None:
        ss, se = plan["search"]
        seg = e[plan["base"] + ss: plan["base"] + se]
        lv = F32(level)                          # numpy compares a float32 array with a Python float in float32
        hit = (seg[:-1] < lv) & (seg[1:] >= lv) if mode == "rise" else (seg[:-1] >= lv) & (seg[1:] < lv)
        where = np.flatnonzero(hit)
        if where.size:
            start, triggered = plan["base"] + ss + int(where[-1]) + 1, 1
    return start, triggered, e[start:start + plan["length"]]


def cells(length, n_points):
    """(P, bounds): column c covers chunk indices [bounds[c], bounds[c + 1]), in exact integers."""
    P = min(int(n_points), int(length))
    return P, [(c * int(length)) // P for c in range(P + 1)]


def columns(chunk, n_points, column="minmax"):
    """[2][P] (minmax) or [P] float32; `mean` is returned in float64 (the device rounds it once to float32)."""
    chunk = np.asarray(chunk, dtype=F32)
    P, b = cells(chunk.size, n_points)
    if column == "minmax":
        out = np.empty((2, P), dtype=F32)
        for c in range(P):
            out[0, c], out[1, c] = np.min(chunk[b[c]:b[c + 1]]), np.max(chunk[b[c]:b[c + 1]])
        return out
    if column == "sample":
        return chunk[np.asarray(b[:-1], dtype=np.int64)].copy()
    if column == "mean":
        return np.array([np.sum(chunk[b[c]:b[c + 1]], dtype=np.float64) / (b[c + 1] - b[c]) for c in range(P)])
    raise ValueError(column)


def statistics(chunk, level):
    """dict(min, max, mean (float64), n_at_or_above, n_rise, n_fall) of a chunk."""
    chunk = np.asarray(chunk, dtype=F32)
    if chunk.size == 0:
        return dict(min=F32(np.nan), max=F32(np.nan), mean=float("nan"), n_at_or_above=0, n_rise=0, n_fall=0)
    lv = F32(level)
    a, b = chunk[:-1], chunk[1:]
    return dict(min=np.min(chunk), max=np.max(chunk), mean=float(np.sum(chunk, dtype=np.float64) / chunk.size),
                n_at_or_above=int(np.count_nonzero(chunk >= lv)),
                n_rise=int(np.count_nonzero((a < lv) & (b >= lv))), n_fall=int(np.count_nonzero((a >= lv) & (b < lv))))
