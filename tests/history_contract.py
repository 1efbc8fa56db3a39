"""3-D history views, restated in numpy (include/tdsa_hip.h, tdsa_history_*).

What the reference's Ribbon, ThreeD and Surface widgets hand their GL items, as plain functions of the pushed float32
dB rows, plus the screen reduction (`columns`), which the reference does not have.  Importable without the library.

Rows are float32 and hold no NaN: np.clip passes a NaN on into an `astype(int)` whose result is undefined, so with a NaN
in a row z is NaN and the colour is unspecified - outside the contract.  +-inf are inside it (z = 0 / 8).

A NaN dB row is nevertheless what a non-finite capture produces, so what it may touch is bounded.  A NaN at bin j of a
pushed row (or of the max or min trace that came with it) leaves unspecified
  - that row's z, colour and colour index at j - with `columns`, the value, colour, index and bin of the cell that
    holds j (one NaN among a cell's bins makes every comparison of its maximum search false);
  - the hold row at j (the hold cell holding j and its bin), from a NaN in the row or in the max trace;
  - the min row at j (its cell and bin) while the min trace with the NaN is the newest;
  - live_peak, and the peak_norm that follows from it, while that row is the newest;
  - hold_peak until reset_hold.
Everything else - the other bins and cells of that row, every other row, the keys of the other slots (so live_peak
again after the next NaN-free push), the rest of the hold and min rows, and hold_peak after reset_hold and a NaN-free
push - has the bits of the same run with the NaN replaced by -inf.
"""
import numpy as np

F32 = np.float32
Z_SCALE = 8
RIBBON_ROWS = 30
RIBBON_SPACING = 0.7
LINE_HUES = int(Z_SCALE * 1.4)          # 11
NEVER_PUSHED = 255                      # colour index of a line no row has reached yet: RGBA 0, as the widget leaves it
MAX_HOLD_COLOUR = (1.0, 1.0, 0.0, 0.5)
MIN_HOLD_COLOUR = (0.2, 0.5, 1.0, 0.5)


# ---------------------------------------------------------------------------------------------------- arithmetic
def heights(row, ref_level, range_db):
    """z of a dB row: clip((dB - (ref - range)) / range * 8, 0, 8), every operation in float32; the three scalars are
    doubles rounded once."""
    row = np.asarray(row, dtype=F32)
    bottom, rng = F32(float(ref_level) - float(range_db)), F32(float(range_db))
    with np.errstate(invalid="ignore", over="ignore"):
        z = (row - bottom) / rng * F32(Z_SCALE)
    return np.clip(z, F32(0), F32(Z_SCALE))


def hsv_to_rgb(h, s, v):
    """The usual sextant formula (as matplotlib.colors.hsv_to_rgb evaluates it), in the dtype of its arguments."""
    h, s, v = np.broadcast_arrays(np.asarray(h), np.asarray(s), np.asarray(v))
    dt = np.result_type(h, s, v)
    h, s, v = h.astype(dt), s.astype(dt), v.astype(dt)
    one, six = dt.type(1), dt.type(6)
    i = (h * six).astype(int)
    f = (h * six) - i.astype(dt)
    p = v * (one - s)
    q = v * (one - s * f)
    t = v * (one - s * (one - f))
    k = i % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    grey = s == 0
    r, g, b = np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)
    return np.stack([r, g, b], axis=-1)


def ribbon_row_consts(row_idx):
    """(y_front, y_back, hue_scale, val, alpha) of ribbon row `row_idx`: float32, float32, float32, double, float32."""
    age = row_idx / max(RIBBON_ROWS - 1, 1)
    y_front = row_idx * RIBBON_SPACING
    y_back = y_front + RIBBON_SPACING * 0.85
    val = float(np.clip(1.0 - age * 0.6, 0.3, 1.0))
    return F32(y_front), F32(y_back), F32(0.3 + 0.7 * age), val, F32(max(0.3, 1.0 - age * 0.5))


def ribbon_row(row_idx, z, x):
    """(verts [2n][3], colours [2n][4]) float32 of one ribbon row, Ribbon._row_verts_colors."""
    z, x = np.asarray(z, dtype=F32), np.asarray(x, dtype=F32)
    n = z.size
    y_front, y_back, hue_scale, val, alpha = ribbon_row_consts(row_idx)
    verts = np.empty((2 * n, 3), dtype=F32)
    verts[0::2, 0], verts[0::2, 1], verts[0::2, 2] = x, y_front, z
    verts[1::2, 0], verts[1::2, 1], verts[1::2, 2] = x, y_back, z
    t = np.clip(z / F32(Z_SCALE), F32(0), F32(1))
    hue = (F32(1) - t) * F32(0.66) * hue_scale                        # float32
    rgb = hsv_to_rgb(hue.astype(np.float64), np.float64(1.0), np.float64(val)).astype(F32)   # float64, rounded once
    per_v = np.concatenate([rgb, np.full((n, 1), alpha, dtype=F32)], axis=1)
    colours = np.empty((2 * n, 4), dtype=F32)
    colours[0::2] = per_v
    colours[1::2] = per_v
    return verts, colours


def ribbon_faces(n):
    """Ribbon._make_faces: uint32 [2 (n - 1)][3]."""
    i = 2 * np.arange(n - 1, dtype=np.uint32)
    return np.stack([np.stack([i, i + 1, i + 2], axis=1), np.stack([i + 1, i + 3, i + 2], axis=1)], axis=1).reshape(-1, 3)


def line_index(z):
    """uint8 colour index of ThreeD: int32(8 - z) % 11."""
    return ((F32(Z_SCALE) - np.asarray(z, dtype=F32)).astype(np.int32) % LINE_HUES).astype(np.uint8)


def line_palette():
    """float32 [11][4]: hsv_to_rgb([k / 11, 1, 1]) in float32, alpha 1."""
    h = np.arange(LINE_HUES, dtype=np.int32).astype(F32) / F32(LINE_HUES)
    pal = np.ones((LINE_HUES, 4), dtype=F32)
    pal[:, :3] = hsv_to_rgb(h, F32(1), F32(1))
    return pal


def line_rgba(index):
    """float32 [...][4] of colour indices; NEVER_PUSHED -> 0."""
    index = np.asarray(index)
    pal = np.concatenate([line_palette(), np.zeros((256 - LINE_HUES, 4), dtype=F32)])
    return pal[index]


def surface_normalise(levels, zmin, zmax):
    """float32(reference): clip((level - zmin) / (zmax - zmin), 0, 1) in float64, 0.5 everywhere when zmax == zmin."""
    lv = np.asarray(levels, dtype=F32).astype(np.float64)
    zmin, zmax = float(zmin), float(zmax)
    if zmax == zmin:
        return np.full(lv.shape, 0.5, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip((lv - zmin) / (zmax - zmin), 0.0, 1.0).astype(F32)


def surface_colours(norm):
    """float32 [...][3] = (t, 0, 1 - t): linear interpolation from blue to red, on the float32 normalised value."""
    t = np.asarray(norm, dtype=F32)
    return np.stack([t, np.zeros_like(t), F32(1) - t], axis=-1)


def cells(n, P):
    """[(first, end)] of the P exact-integer cells of n bins (zero_span_contract.cells)."""
    return [((c * n) // P, ((c + 1) * n) // P) for c in range(P)]


def reduce_columns(rows, P):
    """(values [R][P] float32, bins [R][P] int32): the maximum of each cell and the bin of its first maximum."""
    rows = np.atleast_2d(np.asarray(rows, dtype=F32))
    n = rows.shape[1]
    vals = np.empty((rows.shape[0], P), dtype=F32)
    bins = np.empty((rows.shape[0], P), dtype=np.int32)
    for c, (a, b) in enumerate(cells(n, P)):
        k = np.argmax(rows[:, a:b], axis=1)
        bins[:, c] = a + k
        vals[:, c] = rows[np.arange(rows.shape[0]), a + k]
    return vals, bins


def first_peak(row):
    """(bin, value) of np.argmax."""
    row = np.asarray(row)
    i = int(np.argmax(row))
    return i, row[i]


# ---------------------------------------------------------------------------------------------------- the history
class HistoryModel:
    """What a tdsa_history handle holds, newest row first."""

    def __init__(self, depth, n_bins, kind):
        assert kind in ("heights", "levels")
        self.depth, self.n, self.kind = int(depth), int(n_bins), kind
        self.ref_level, self.range_db = 0.0, 100.0
        self.reset()

    def reset(self):
        self.rows = np.zeros((self.depth, self.n), dtype=F32)
        self.hold = np.zeros(self.n, dtype=F32)
        self.min_row = None
        self.pushed = 0

    def set_amplitude(self, ref_level, range_db):
        self.ref_level, self.range_db = float(ref_level), float(range_db)

    def reset_hold(self):
        self.hold[:] = 0

    def _store(self, row):
        row = np.asarray(row, dtype=F32)
        return heights(row, self.ref_level, self.range_db) if self.kind == "heights" else row.copy()

    def push(self, live, max_trace=None, min_trace=None, hold=True):
        z = self._store(live)
        self.rows[1:] = self.rows[:-1].copy()
        self.rows[0] = z
        self.pushed += 1
        if self.kind == "heights":
            if hold:
                self.hold = np.maximum(self.hold, z if max_trace is None else self._store(max_trace))
            self.min_row = None if min_trace is None else self._store(min_trace)

    def push_rows(self, rows):
        for r in np.atleast_2d(rows):
            self.push(r)

    # ---- views
    def _source(self, rows, columns):
        if columns is None:
            return rows, None
        return reduce_columns(rows, columns)

    def ribbon(self, x, columns=None):
        x = np.asarray(x, dtype=F32)
        R = min(RIBBON_ROWS, self.depth)
        src, bins = self._source(self.rows[:R], columns)
        out = [ribbon_row(r, src[r], x if bins is None else x[bins[r]]) for r in range(R)]
        return dict(verts=np.stack([o[0] for o in out]), colours=np.stack([o[1] for o in out]), bins=bins)

    def lines(self, first=0, count=None, columns=None):
        count = self.depth - first if count is None else count
        src, bins = self._source(self.rows[first:first + count], columns)
        index = line_index(src)
        valid = min(self.pushed, self.depth)
        index[max(valid - first, 0):] = NEVER_PUSHED
        hold, hold_bins = self._source(self.hold[None], columns)
        res = dict(z=src, index=index, rgba=line_rgba(index), bins=bins, hold=hold[0],
                   hold_bins=None if hold_bins is None else hold_bins[0],
                   live_peak=first_peak(self.rows[0]), hold_peak=first_peak(self.hold), min=None, min_bins=None)
        if self.min_row is not None:
            m, mb = self._source(self.min_row[None], columns)
            res["min"], res["min_bins"] = m[0], None if mb is None else mb[0]
        return res

    def surface(self, columns=None):
        zmin, zmax = self.ref_level - self.range_db, self.ref_level
        src, bins = self._source(self.rows, columns)
        norm = surface_normalise(src, zmin, zmax)
        bin_, level = first_peak(self.rows[0])
        # the widget normalises the marker from the float32 live row, so in float32 (the grid, from its float64 history)
        with np.errstate(invalid="ignore", over="ignore"):
            peak_norm = 0.5 if zmax == zmin else float(np.clip((F32(level) - F32(zmin)) / F32(zmax - zmin), F32(0), F32(1)))
        return dict(z=norm, colours=surface_colours(norm), bins=bins, live_peak=(bin_, level), peak_norm=peak_norm)


# ---------------------------------------------------------------------------------------------------- read-outs
def format_freq_hz(hz):
    """ThreeD._format_freq."""
    hz = abs(hz)
    if hz >= 1e9:
        return f"{hz / 1e9:.3f} GHz"
    if hz >= 1e6:
        return f"{hz / 1e6:.3f} MHz"
    if hz >= 1e3:
        return f"{hz / 1e3:.3f} kHz"
    return f"{hz:.1f} Hz"


def format_freq_mhz(mhz):
    """Surface._format_freq."""
    if abs(mhz) >= 1.0:
        return f"{mhz:.3f} MHz"
    if abs(mhz) >= 0.001:
        return f"{mhz * 1000:.3f} kHz"
    return f"{mhz * 1e6:.1f} Hz"


def ribbon_x(bins):
    """Ribbon._make_x: float32."""
    bins = np.asarray(bins)
    f0, f1 = float(bins[0]), float(bins[-1])
    span = f1 - f0 if f1 != f0 else 1.0
    return -10.0 + (bins.astype(F32) - f0) / span * 20.0


def line_x(bins, log_freq=False):
    """ThreeD.initialise_traces: float64, linear or log10."""
    bins = np.asarray(bins)
    f0, f1 = float(np.min(bins)), float(np.max(bins))
    if f1 == f0:
        f1 = f0 + 1.0
    if log_freq:
        lb = np.log10(np.maximum(bins, 1.0))
        lf0, lf1 = np.log10(max(f0, 1.0)), np.log10(max(f1, 1.0))
        span = lf1 - lf0 if lf1 != lf0 else 1.0
        return -10 + ((lb - lf0) / span) * 20
    return -10 + ((bins - f0) / (f1 - f0)) * 20
