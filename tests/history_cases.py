"""Input builders of the shape-driven history tests (tests/test_gpu_history_shapes.py) and of the host checks that prove
their preconditions (tests/test_history_host.py).  Importable without the library: numpy, history_contract and the text
of tdsa_history.hpp only.

Every builder returns, next to its rows, the facts a case relies on (where a maximum was planted, which rows a push
skips, which floats straddle a sextant boundary), so that the host checks can prove them from the rows themselves and a
later change cannot quietly empty a GPU case."""
import os
import re

import numpy as np

import history_contract as hc

F32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "topdogspectrumanalyser_amd", "csrc")
BLOCK = 256                                       # kBlock of tdsa_history.hip
WAVE = 64


def header_const(name):
    """An integer constexpr of tdsa_history.hpp."""
    src = open(os.path.join(CSRC, "tdsa_history.hpp")).read()
    expr = re.search(r"constexpr (?:int|long long) %s = ([^;]+);" % name, src).group(1)
    return int(eval(re.sub(r"(\d)ll\b", r"\1", expr)))


# ---------------------------------------------------------------------------------------------------- the launchers
def lane_width(n, aligned=True):
    """Bins per lane of the push and view passes: 4 with a bin count that is a multiple of 4 and 16-byte pointers."""
    return 4 if n % 4 == 0 and aligned else 1


def push_geometry(n, n_rows, aligned=True, max_wgs=None):
    """launch_hist_push's grid: (gx, gy, rows_per_wg, rows_in_last_chunk)."""
    max_wgs = header_const("kHistPushMaxWgs") if max_wgs is None else max_wgs
    gx = (n // lane_width(n, aligned) + BLOCK - 1) // BLOCK
    gy = min(max(max_wgs // gx, 1), n_rows)
    rows_per_wg = (n_rows + gy - 1) // gy
    gy = (n_rows + rows_per_wg - 1) // rows_per_wg
    return gx, gy, rows_per_wg, n_rows - (gy - 1) * rows_per_wg


def reduce_group(n, columns):
    """launch_hist_reduce's lanes per cell."""
    cell = n // columns
    return 64 if cell >= 32 else 16 if cell >= 8 else 4


def cell_of(n, columns, j):
    """The cell of hc.cells(n, columns) that holds bin j."""
    for c, (a, b) in enumerate(hc.cells(n, columns)):
        if a <= j < b:
            return c
    raise ValueError((n, columns, j))


def hist_key(v, index):
    """hist_key of tdsa_history.hip on a float32 and a bin: the larger key is the larger value, then the smaller bin."""
    v = F32(0) if v == 0 else F32(v)
    b = int(np.array(v, dtype=F32).view(np.uint32))
    b = (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    return (b << 32) | (~int(index) & 0xFFFFFFFF)


def key_argmax(row):
    """The bin the device reports for a row: the maximum of hist_key."""
    keys = [hist_key(v, i) for i, v in enumerate(np.asarray(row, dtype=F32))]
    return int(np.argmax(np.array(keys, dtype=object)))


KEY_SPECIALS = np.array([-np.inf, -300.0, -80.5, -80.25, -1e-30, -0.0, 0.0, 1e-30, 3.0, np.inf], dtype=F32)


def generic_rows(rng, n_rows, n):
    """float32 dB rows without NaN: noise around -80 dBm, bins off the scale on both sides, +-inf, a plateau."""
    rows = rng.normal(-80.0, 12.0, size=(n_rows, n)).astype(F32)
    for r in range(n_rows):
        rows[r, rng.integers(0, n)] = 40.0
        rows[r, rng.integers(0, n)] = -300.0
        if r % 3 == 1:
            rows[r, rng.integers(0, n)] = np.inf
            rows[r, rng.integers(0, n)] = -np.inf
        if r % 4 == 2 and n >= 8:
            a = int(rng.integers(0, n - n // 4))
            rows[r, a:a + max(n // 4, 2)] = 25.0
    return rows


# ---------------------------------------------------------------------------------------------------- row chunks
CHUNK_SHAPES = [(8192, 257), (4099, 250), (1001, 2051), (1024, 2049)]       # (n, rows of the batch)
CHUNK_DEPTHS = (30, 7)
CHUNK_AMPLITUDE = (-10.0, 90.0)
CHUNK_COLUMNS = 129
CEILING = -30.0                                   # the noise stays below it, what is planted lies above it


def chunk_case(n, n_rows, depth):
    """One host row, then a batch of n_rows rows for a history of `depth` lines.

    Three classes of columns carry a planted maximum over everything pushed (all other bins of those columns stay
    below CEILING; the rows between are noise with the usual off-scale bins elsewhere):
      "skipped"     in a row the ring is too shallow for (k < skip): it reaches the hold row and no line
      "chunk_end"   in the last row of a chunk, with the next highest value in the first row of the following chunk
      "chunk_start" the other way round
    so the hold of such a column crosses the workgroups of two chunks."""
    rng = np.random.default_rng(n * 131 + n_rows * 7 + depth)
    gx, gy, rpw, last = push_geometry(n, n_rows)
    skip = n_rows - depth
    first = np.minimum(rng.normal(-80.0, 12.0, n), CEILING - 1).astype(F32)
    batch = np.minimum(rng.normal(-80.0, 12.0, (n_rows, n)), CEILING - 1).astype(F32)
    per = min(200, n // 5)
    cols = rng.permutation(n)[:3 * per]
    classes = dict(skipped=np.sort(cols[:per]), chunk_end=np.sort(cols[per:2 * per]), chunk_start=np.sort(cols[2 * per:]))
    free = np.setdiff1d(np.arange(n), cols)
    for k in range(n_rows):                       # off-scale bins and infinities, away from the planted columns
        batch[k, free[rng.integers(0, free.size)]] = 40.0
        batch[k, free[rng.integers(0, free.size)]] = -300.0
        if k % 3 == 1:
            batch[k, free[rng.integers(0, free.size)]] = np.inf
            batch[k, free[rng.integers(0, free.size)]] = -np.inf
    stored_chunks = np.arange((skip + rpw - 1) // rpw, gy - 1)               # chunks stored whole, with a successor
    planted = {}
    for i, c in enumerate(classes["skipped"]):
        k = int(rng.integers(0, skip))
        batch[k, c] = F32(-12.0 - 0.01 * i)
        planted[int(c)] = k
    for name in ("chunk_end", "chunk_start"):
        for i, c in enumerate(classes[name]):
            g = int(stored_chunks[rng.integers(0, stored_chunks.size)])
            end, start = g * rpw + rpw - 1, (g + 1) * rpw
            hi, lo = (end, start) if name == "chunk_end" else (start, end)
            batch[hi, c] = F32(-12.0 - 0.01 * i)
            batch[lo, c] = F32(-20.0 - 0.01 * i)
            planted[int(c)] = hi
    return dict(n=n, n_rows=n_rows, depth=depth, first=first, batch=batch, classes=classes, planted=planted, skip=skip,
                geometry=(gx, gy, rpw, last))


# ---------------------------------------------------------------------------------------------------- one-bin lanes
ONE_BIN_N = (5, 63, 65, 257, 1001, 4099)
ONE_BIN_DEPTH = 5


def one_bin_columns(n):
    """A column count that is no multiple of 4, so that the views of the reduced rows take one-bin lanes too."""
    return 129 if n > 129 else 3 if n < 7 else 7


MISALIGNED_N = (1000, 1028)
MISALIGNED_OFFSETS = (4, 8, 12)
PAD = 4                                           # floats of +inf before and after the rows, beside the offset


def misaligned_buffer(rows, offset):
    """(float32 array for a 16-byte aligned device buffer, byte offset of the rows in it): +inf wherever no row is."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    at = PAD + offset // 4
    buf = np.full(at + rows.size + PAD + 4, np.inf, dtype=F32)
    buf[at:at + rows.size] = rows.reshape(-1)
    return buf, 4 * at


# ---------------------------------------------------------------------------------------------------- maxima below zero
NEGATIVE_AMPLITUDE = (-20.0, 100.0)               # heights: -120 .. -20 dBm fill the scale
NEGATIVE_N = (1500, 515)                          # 16-byte lanes in two workgroups, one-bin lanes in three


def negative_rows(n):
    """[(name, row, bin of the maximum, all below zero)]: what a row claims is proved by the host checks."""
    rng = np.random.default_rng(n)
    V = lane_width(n)
    second_wg = BLOCK * V                         # first bin of the second workgroup of a push
    assert second_wg < n
    out = []

    def noise():
        return rng.uniform(-110.0, -30.0, n).astype(F32)

    for name, at in (("bin 0", 0), ("last bin", n - 1), ("last lane of a wave", WAVE * V - 1),
                     ("first bin of the second workgroup", second_wg)):
        row = noise()
        row[at] = -25.5
        out.append((name, row, at, True))
    out.append(("nothing but -inf", np.full(n, -np.inf, dtype=F32), 0, True))
    for name, zeros in (("-0 before +0", (-0.0, 0.0)), ("+0 before -0", (0.0, -0.0))):
        row = noise()
        at = np.sort(rng.permutation(np.arange(3, n))[:12])
        row[at] = np.resize(np.array(zeros, dtype=F32), at.size)
        out.append((name, row, int(at[0]), False))
    row = noise()
    a, b = second_wg // 3, second_wg + (n - second_wg) // 2
    row[a] = row[b] = -25.5
    out.append(("equal maxima in two workgroups", row, a, True))
    row = noise()
    row[b] = -25.5
    row[a] = -25.75
    out.append(("the maximum in the higher workgroup", row, b, True))
    return out


# ---------------------------------------------------------------------------------------------------- cell widths
WIDTH_CASES = {1000: {31: 64, 32: 16, 33: 16, 124: 16, 125: 16, 126: 4, 127: 4},      # n -> columns -> lanes per cell
               64: {2: 64, 3: 16, 8: 16, 9: 4, 63: 4, 64: 4}}
WIDTH_DEPTH = 7
WIDTH_ROWS = 9


def width_rows(n, columns):
    """(rows [WIDTH_ROWS][n], min trace, plateaus, cell of -inf): noise, and in every row a few cells with a plateau
    above it.  In a cell wider than its group the plateau starts in lane G / 4 of one stride and reaches lane 0 of the
    next; in a narrower cell it starts at the cell's second bin.  It runs on into the following cell, whose first
    maximum is then its first bin.  plateaus: [(row, cell, first, end)]; (row, cell) of the cell that is -inf
    throughout."""
    rng = np.random.default_rng(n * 1009 + columns)
    G = reduce_group(n, columns)
    cells = hc.cells(n, columns)
    rows = rng.normal(-80.0, 12.0, (WIDTH_ROWS, n)).astype(F32)
    plateaus = []
    for r in range(WIDTH_ROWS):
        for c in range(r % 3, columns, 3):
            lo, hi = cells[c]
            w = hi - lo
            if w > G:
                b = (w - 1) // G * G              # lane 0 of the last stride
                a = b - G + max(G // 4, 1)
            elif w >= 3:
                a, b = 1, w - 1
            else:
                continue
            end = min(lo + b + 3, n)
            rows[r, lo + a:end] = F32(-10.0 - r)
            plateaus.append((r, c, lo + a, end))
    dead = (WIDTH_ROWS - 2, columns // 2)
    lo, hi = cells[dead[1]]
    rows[dead[0], lo:hi] = -np.inf
    plateaus = [p for p in plateaus if not (p[0] == dead[0] and p[2] < hi and p[3] > lo)]
    min_trace = np.minimum.reduce(rows)
    return rows, min_trace, plateaus, dead


# ---------------------------------------------------------------------------------------------------- arithmetic edges
EXACT_AMPLITUDE = (8.0, 8.0)                      # bottom 0, range 8: z == clip(dB, 0, 8) exactly


def _neighbours(v, steps=1):
    v = F32(v)
    out, lo, hi = [v], v, v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return out


def integer_edge_row(n):
    """A row of n >= 54 bins: every k in 0 .. 8, k + 0.5 and the float32 neighbours on both sides of each."""
    vals = [x for k in range(9) for v in (k, k + 0.5) for x in _neighbours(v)]
    row = np.full(n, 3.25, dtype=F32)
    row[:len(vals)] = np.array(vals, dtype=F32)
    return row


SEXTANT_ROWS = (0, 1, 14, 29)
SEXTANTS = (1, 2, 3)


def ribbon_sextant(row_idx, z):
    """int(hue * 6) of hc.ribbon_row for height z in ribbon row row_idx, by the contract's own arithmetic."""
    hue_scale = hc.ribbon_row_consts(row_idx)[2]
    t = np.clip(F32(z) / F32(hc.Z_SCALE), F32(0), F32(1))
    hue = (F32(1) - t) * F32(0.66) * hue_scale
    return int(np.float64(hue) * np.float64(6))


def sextant_pairs():
    """{(ribbon row, sextant): (z_lo, z_hi)}: adjacent float32 heights with int(hue * 6) == sextant at z_lo and
    sextant - 1 at z_hi, found by bisection over the bit patterns of [0, 8] (the hue falls as z grows)."""
    out = {}
    for r in SEXTANT_ROWS:
        for s in SEXTANTS:
            lo, hi = 0, int(F32(8).view(np.uint32))             # bit patterns of +0 and 8: ordered as their values
            f = lambda b: ribbon_sextant(r, np.uint32(b).view(F32))   # noqa: E731
            if f(lo) < s:
                continue                                        # the row's hue never reaches this sextant
            assert f(hi) < s
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if f(mid) >= s:
                    lo = mid
                else:
                    hi = mid
            out[(r, s)] = (np.uint32(lo).view(F32), np.uint32(hi).view(F32))
    return out


def sextant_row(n):
    """A row of n >= 112 bins: the eight float32 either side of every boundary of sextant_pairs()."""
    vals = []
    for z_lo, z_hi in sextant_pairs().values():
        b = int(F32(z_lo).view(np.uint32))
        vals += [np.uint32(b + d).view(F32) for d in range(-7, 9)]
    row = np.full(n, 3.25, dtype=F32)
    row[:len(vals)] = np.array(vals, dtype=F32)
    return row


SURFACE_AMPLITUDES = ((0.0, 100.0), (-3.7, 0.1), (1e30, 2e30))


def surface_edge_rows(n):
    """Two rows of n >= 24 bins: for each amplitude float32(zmin) and float32(zmax) with one float32 step either side of
    each; the first row also holds +-inf and both zeros."""
    vals = []
    for ref, rng_db in SURFACE_AMPLITUDES:
        for v in (ref - rng_db, ref):
            vals += _neighbours(v)
    rows = np.full((2, n), -50.0, dtype=F32)
    rows[:, :len(vals)] = np.array(vals, dtype=F32)
    rows[0, len(vals):len(vals) + 4] = [np.inf, -np.inf, 0.0, -0.0]
    return rows


# ---------------------------------------------------------------------------------------------------- NaN
NAN_N = 1000
NAN_BINS = (496, 498, NAN_N - 1)                  # a first lane element, a middle lane element, the last bin
NAN_CHUNK = (1024, 2049, 30)                      # the chunk case the NaN batch borrows: (n, rows, depth)
