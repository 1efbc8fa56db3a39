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


def view(history, capacity, n_display, mode="free_run", level=0.0, origin=0):
    """(start, triggered, chunk) over the detected history (absolute indices).  `origin` is the absolute index of
    history[0]: a test that only knows the end of a long stream passes that end (at least everything the ring holds)
    and where it begins; 0 means the full history."""
    e = np.asarray(history, dtype=F32)
    origin = int(origin)
    plan = view_plan(origin + e.size, capacity, n_display, mode)
    if origin < 0 or plan["base"] < origin:
        raise ValueError(f"origin={origin}: the history must reach back to base={plan['base']}")
    start, triggered = plan["free_start"], 0
    if plan["search"] is not None:
        ss, se = plan["search"]
        seg = e[plan["base"] - origin + ss: plan["base"] - origin + se]
        lv = F32(level)                          # numpy compares a float32 array with a Python float in float32
        hit = (seg[:-1] < lv) & (seg[1:] >= lv) if mode == "rise" else (seg[:-1] >= lv) & (seg[1:] < lv)
        where = np.flatnonzero(hit)
        if where.size:
            start, triggered = plan["base"] + ss + int(where[-1]) + 1, 1
    return start, triggered, e[start - origin:start - origin + plan["length"]]


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


# ---------------------------------------------------------------------------------------------------- test inputs
def sum_is_exact(values, unit=2.0 ** -7):
    """True when every float64 sum over `values`, in any order and of any subset, is exact: all are integer multiples
    of `unit` and the largest possible partial sum, in units, needs no more than 53 bits."""
    v = np.asarray(values, dtype=np.float64) / unit
    if v.size == 0:
        return True
    if not np.all(np.isfinite(v)) or not np.array_equal(v, np.rint(v)):
        return False
    return int(np.sum(np.abs(v).astype(np.int64))) < 2 ** 53      # int64: exact for any test-sized input


def crossing_train(n, rng, first_above=False, unit=2.0 ** -7):
    """n float32 values that alternate below / above the level 0.0 at every sample: multiples of `unit` with
    magnitudes 1 .. 127 units drawn from rng, so that neighbours, cells and sums all tell samples apart."""
    mag = rng.integers(1, 128, int(n)).astype(np.float64) * unit
    sign = np.where((np.arange(int(n)) + (1 if first_above else 0)) % 2 == 1, 1.0, -1.0)
    return (mag * sign).astype(F32)


def crossings(values, level=0.0):
    """(n_rise, n_fall) between neighbours, as `statistics` counts them."""
    st = statistics(values, level)
    return st["n_rise"], st["n_fall"]


def db_spacing(re, im, log_floor):
    """Smallest |difference| in dB between neighbouring samples of the float64 DB detector (inf for fewer than two)."""
    d = detect64(re, im, "db", log_floor, 0.0)
    return float(np.min(np.abs(np.diff(d)))) if d.size > 1 else float("inf")


def spaced_samples(rng, n, fmt, log_floor=1e-12, min_db=0.1):
    """n raw samples of one input format whose neighbours differ by at least `min_db` in the DB detector and are not
    equal in Re x, with re^2 + im^2 + log_floor inside [1e-12, 32]: a sample stored one slot off cannot pass any of the
    three detectors.  Returned in the layout `unpack` takes (interleaved bytes, complex64 or float32)."""
    n = int(n)

    def draw(k):
        if fmt == "i8":
            return rng.integers(-128, 128, (k, 2)).astype(np.int8)
        if fmt == "u8":
            return rng.integers(0, 256, (k, 2)).astype(np.uint8)
        amp = (10.0 ** rng.uniform(-3.0, 0.3, k)) * rng.choice([-1.0, 1.0], k)
        if fmt == "c64":
            return (amp * np.exp(1j * rng.uniform(0, 2 * np.pi, k))).astype(np.complex64)
        return amp.astype(F32)

    a = draw(n)
    for _ in range(200):
        re, im = unpack(a, fmt)
        d = detect64(re, im, "db", log_floor, 0.0)
        bad = np.flatnonzero((np.abs(np.diff(d)) < min_db) | (re[1:] == re[:-1])) + 1
        if bad.size == 0:
            break
        a[bad] = draw(bad.size)
    else:
        raise RuntimeError("no spaced sequence found")
    return a.reshape(-1)


# ---------------------------------------------------------------------------------------------------- the shapes suite
# Inputs of tests/test_gpu_zero_span_shapes.py; tests/test_zero_span_host.py asserts without a GPU that they discriminate.
GROUP = {"i8": 8, "u8": 8, "c64": 4, "f32r": 4}                  # samples per lane of the push kernel's body
LOG_FLOOR, OFFSET_DB = 1e-12, -12.5
PUSH_CAPS = (61, 1021)                                           # not multiples of 4: the ring position takes every residue


def push_lengths(cap):
    rng = np.random.default_rng(cap)
    lengths = [int(v) for v in rng.permutation(41)]
    for at, n in ((7, cap - 1), (16, cap), (25, cap + 1), (34, 3 * cap + 5)):
        lengths.insert(at, n)
    return lengths


def push_pieces(cap, lengths, group):
    """(head, groups, tail, n) of every launch the host makes for this stream of pushes (tdsa_capi_zspan.cpp)."""
    out, total = [], 0
    for n in lengths:
        skip = max(0, n - cap)
        t, left = total + skip, n - skip
        while left > 0:
            pos = t % cap
            piece = min(left, cap - pos)
            head = min((4 - pos % 4) & 3, piece)
            groups = (piece - head) // group
            out.append((head, groups, piece - head - groups * group, piece))
            t, left = t + piece, left - piece
        total += n
    return out


def push_stream(fmt, cap):
    lengths = push_lengths(cap)
    raw = spaced_samples(np.random.default_rng(cap + len(fmt)), sum(lengths), fmt, LOG_FLOOR)
    return lengths, raw


def extreme_parts():
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x000ABCDE, 0x007FFFFF, 0x00800000,   # zeros, denormals
                     0x1E3CE508,                 # 1e-20: the square is a denormal
                     0x0DA24260, 0x1A000000,     # 1e-30: the square underflows to 0; 2^-75: exactly the smallest denormal / 2
                     0x5F000000, 0xDF000000,     # +-2^63: one square fits, the sum of two is 2^127
                     0x5F800000, 0x60AD78EC,     # 2^64 and 1e20: the square overflows
                     0x3F800000, 0xBFC00000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0xFFC12345, 0x7FA00001], dtype=np.uint32)   # NaNs with payloads, one signalling
    return bits.view(F32)


PAD = 64                                                          # the ring is the window and this many samples


def train_case(length, seed):
    """(history, cap, start): an alternating train around level 0.0 in a ring just large enough; the rise-triggered
    window of `length` starts a few samples before the physical end of the ring and ends before the history does."""
    cap = length + PAD
    total = cap + (length - 3) % cap
    rng = np.random.default_rng(seed)
    e = crossing_train(total, rng)
    start, trig, chunk = view(e, cap, length, "rise", 0.0)
    assert trig == 1 and chunk.size == length and 1 <= total - (start + length) <= 2
    assert cap - 8 <= start % cap < cap and (length < 8 or start % cap + length > cap)   # laid across the physical wrap
    assert sum_is_exact(e) and sum(crossings(chunk)) == length - 1
    assert (e[start - 1] < 0) != (e[start] < 0) and (e[start + length - 1] < 0) != (e[start + length] < 0)
    return e, cap, start


def nan_positions(length, points):
    """Chunk indices for NaNs: first and last sample of a cell and of a workgroup's share (never 0 or 1, which would
    move the trigger)."""
    if points:
        P, b = cells(length, points)
        pos = {b[c] for c in (1, P // 2, P - 1) if c < P} | {b[c + 1] - 1 for c in (0, P // 2, P - 2) if 0 <= c < P}
        team = 256 if length // P >= 1024 else 64
        pos |= {b[P // 2] + team - 1, b[P // 2] + team}          # a lane's second sample of a long cell
    else:
        stride = min(1024, -(-length // 1024)) * 256
        pos = {255, 256, 1023, 1024, stride - 1, stride, length - 1}
    return sorted(k for k in pos if 2 <= k < length)


VIEW_SHAPES = [(1024 * 3 - 1, 3), (1024 * 3, 3), (1024 * 3 + 1, 3), (2 * 16384 + 5, 16384), (2 * 16384 + 5, 4097),
               (1025 * 1024 + 7, 1025), (1024 * 1024 + 3, None), (4 * 256 * 3 + 1, None),
               (1, 1), (2, 2), (3, 2), (64, 1), (65, 1), (255, 4), (257, 4), (5, 7), (100, 16384), (3, None)]
