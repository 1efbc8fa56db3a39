"""Zero span (tdsa_zerospan.hip, tdsa_capi_zspan.cpp, zerospan.py) pinned against tests/zero_span_contract.py at small
shapes and at the edges where a kernel goes wrong: every head, body and tail of a push in every format and detector and
by every route, extreme samples, a trigger crossing at every position of a small ring, views whose cells, waves,
workgroups and stride loops all have seams inside an alternating train with exact sums, `out_dev` and the read-back
threshold through the C-ABI, absolute indices past 2^31 and 2^32, and the Python layer at the smallest rings.

Every comparison is against the numpy contract over the full detected history.  Raw chunks, SAMPLE columns and ring
contents are compared as uint32 bit patterns; MINMAX columns and info.min / info.max by value with NaN equal to NaN,
because numpy does not define the sign of a zero that ties in np.min / np.max.  Every family first asserts on the CPU
that its inputs discriminate."""
import ctypes as C

import numpy as np
import pytest

import zero_span_contract as zc
from topdogspectrumanalyser_amd import DeviceBuffer

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]        # every test under a time limit of its own

F32 = np.float32
ERR_ARG = -1
BYTES = {"i8": 2, "u8": 2, "c64": 8, "f32r": 4}
ITEMS = {"i8": 2, "u8": 2, "c64": 1, "f32r": 1}                  # array elements per sample
SENTINEL = F32(-12345.678)
LOG_FLOOR, OFFSET_DB, PAD = zc.LOG_FLOOR, zc.OFFSET_DB, zc.PAD


def _nat():
    from topdogspectrumanalyser_amd import _native as nat
    return nat


def _fmt(fmt):
    nat = _nat()
    return {"i8": nat.IN_I8, "u8": nat.IN_U8, "c64": nat.IN_C64, "f32r": nat.IN_F32R}[fmt]


def _aligned(nbytes):
    """A DeviceBuffer whose base is aligned to at least 256 bytes."""
    buf = DeviceBuffer(nbytes)
    assert buf.ptr % 256 == 0
    return buf


class _Zs:
    """tdsa_zspan_* through ctypes: capacity, max_host_samples and out_dev are arguments here."""

    def __init__(self, capacity, max_host=1 << 16, detector="real", log_floor=0.0, offset_db=0.0):
        nat = _nat()
        self.capacity, self.h = int(capacity), C.c_void_p()
        nat.check(nat.lib.tdsa_zspan_create(0, self.capacity, int(max_host), C.byref(self.h)))
        det = {"real": nat.ZS_DET_REAL, "mag": nat.ZS_DET_MAG, "db": nat.ZS_DET_DB}[detector]
        nat.check(nat.lib.tdsa_zspan_set_detector(self.h, det, log_floor, offset_db))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _nat().lib.tdsa_zspan_destroy(self.h)

    def reset(self):
        _nat().check(_nat().lib.tdsa_zspan_reset(self.h))

    def push(self, raw, fmt):
        raw = np.ascontiguousarray(raw)
        _nat().check(_nat().lib.tdsa_zspan_push(self.h, _fmt(fmt), raw.ctypes.data_as(C.c_void_p), raw.size // ITEMS[fmt]))

    def push_dev(self, ptr, fmt, n):
        _nat().check(_nat().lib.tdsa_zspan_push_dev(self.h, None, _fmt(fmt), C.c_void_p(int(ptr)), int(n)))

    def view(self, mode="free_run", level=0.0, n_display=None, points=0, column="minmax", host=True, dev_ptr=None):
        """(info, host floats or None).  The host buffer carries a sentinel behind what the view may write."""
        nat = _nat()
        n_display = self.capacity if n_display is None else int(n_display)
        rows = 2 if column == "minmax" else 1
        room = min(n_display, self.capacity) if points == 0 else rows * points
        out = np.full(room + 4, SENTINEL, dtype=F32) if host else None
        info = nat.ZspanInfo()
        rc = nat.lib.tdsa_zspan_view(
            self.h, {"free_run": nat.ZS_FREE_RUN, "rise": nat.ZS_RISE, "fall": nat.ZS_FALL}[mode], float(level),
            n_display, int(points), {"minmax": nat.ZS_COL_MINMAX, "sample": nat.ZS_COL_SAMPLE, "mean": nat.ZS_COL_MEAN}[column],
            C.byref(info), out.ctypes.data_as(C.c_void_p) if host else None, C.c_void_p(dev_ptr) if dev_ptr else None)
        nat.check(rc)
        if not host:
            return info, None
        n_out = info.length if points == 0 else rows * info.n_columns
        assert np.all(out[n_out:] == SENTINEL), "the view wrote behind its output"
        return info, out[:n_out]

    def ring(self):
        """Everything held, oldest first."""
        return self.view()[1]


def _u32(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


def _same_bits(a, b):
    a, b = _u32(a), _u32(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _same_values(a, b):
    """By value, NaN equal to NaN (and so -0.0 equal to 0.0: numpy leaves the sign of a tied zero in np.min open)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _check_info(info, chunk, level, exact_mean):
    st = zc.statistics(chunk, level)
    got = (info.n_at_or_above, info.n_rise, info.n_fall)
    assert got == (st["n_at_or_above"], st["n_rise"], st["n_fall"]), (got, st)
    assert _same_values(info.min, st["min"]) and _same_values(info.max, st["max"]), (info.min, info.max, st)
    if not np.isfinite(st["mean"]):
        assert np.array_equal(info.mean, st["mean"], equal_nan=True), (info.mean, st["mean"])
    elif exact_mean:
        assert info.mean == st["mean"], (info.mean, st["mean"])
    else:
        assert abs(info.mean - st["mean"]) <= 2.0 ** -24 * float(np.mean(np.abs(chunk.astype(np.float64)))) + 1e-300


def _check_view(zs, history, mode, level, n_display, points=0, column="minmax", origin=0, exact_mean=False, tag=""):
    """One view against the contract: start, triggered, length, total, the trace and the statistics."""
    with np.errstate(over="ignore"):
        start, trig, chunk = zc.view(history, zs.capacity, n_display, mode, level, origin=origin)
    info, out = zs.view(mode, level, n_display, points, column)
    got = (info.total, info.start, info.triggered, info.length)
    assert got == (origin + len(history), start, trig, chunk.size), (tag, got, (origin + len(history), start, trig, chunk.size))
    if points == 0:
        assert info.n_columns == 0 and _same_bits(out, chunk), (tag, mode, level, n_display)
    elif chunk.size:
        P, bounds = zc.cells(chunk.size, points)
        assert info.n_columns == P
        want = zc.columns(chunk, points, column)
        if column == "minmax":
            assert _same_values(out.reshape(2, P), want), (tag, "minmax")
        elif column == "sample":
            assert _same_bits(out, want), (tag, "sample")
        elif exact_mean:
            assert _same_bits(out, want.astype(F32)), (tag, "mean")        # the exact float64 mean, rounded once
        else:
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(out), nan), (tag, "mean")
            peak = np.array([np.max(np.abs(chunk[bounds[c]:bounds[c + 1]])) for c in range(P)], dtype=np.float64)
            assert np.all(np.abs(out.astype(np.float64) - want)[~nan] <= 2.0 ** -23 * peak[~nan]), (tag, "mean")
    else:
        assert info.n_columns == 0 and out.size == 0
    with np.errstate(over="ignore"):
        _check_info(info, chunk, level, exact_mean)
    return info, out


# ---------------------------------------------------------------------------------------------------- 1. push
def _check_ring(got, want, want64, detector, tag):
    if detector != "db":
        assert _same_bits(got, want), tag                         # REAL and MAG: the float32 restatement bit for bit
        return 0.0
    assert got.shape == want.shape and np.all(np.isfinite(got)), tag      # these streams have no non-finite value
    off = float(np.max(np.abs(got.astype(np.float64) - want64), initial=0.0))
    assert off <= 1e-3, (tag, off)
    return off


@pytest.mark.parametrize("cap", zc.PUSH_CAPS)
@pytest.mark.parametrize("detector", ["real", "mag", "db"])
@pytest.mark.parametrize("fmt", ["i8", "u8", "c64", "f32r"])
def test_push_every_head_body_and_tail_by_every_route(fmt, detector, cap):
    lengths, raw = zc.push_stream(fmt, cap)
    item, bps = ITEMS[fmt], BYTES[fmt]
    # that the stream discriminates (every head, tail and piece length, a launch across the wrap, neighbours apart in
    # every detector) is asserted without a GPU: test_zero_span_host.py::test_inputs_of_the_shapes_suite_discriminate
    re, im = zc.unpack(raw, fmt)
    want = zc.detect(re, im, detector, LOG_FLOOR, OFFSET_DB)
    want64 = zc.detect64(re, im, detector, LOG_FLOOR, OFFSET_DB)
    kw = dict(detector=detector, log_floor=LOG_FLOOR, offset_db=OFFSET_DB)
    worst = 0.0
    with _Zs(cap, **kw) as host, _Zs(cap, **kw) as d1, _Zs(cap, **kw) as d2, _Zs(cap, **kw) as d3, \
            _Zs(cap, 1, **kw) as c1, _Zs(cap, 3, **kw) as c3, _Zs(cap, 8, **kw) as c8, _aligned(raw.nbytes + 64) as dev:
        # one copy of the stream per source offset: 1, 2 and 3 samples into the 16-byte-aligned allocation
        with _aligned(raw.nbytes + 64) as dev2, _aligned(raw.nbytes + 64) as dev3:
            devs = ((d1, dev, 1), (d2, dev2, 2), (d3, dev3, 3))
            for _, buf, s in devs:
                buf.put(raw, s * bps)
            done = 0
            for n in lengths:
                piece = raw[item * done:item * (done + n)]
                for zs in (host, c1, c3, c8):
                    zs.push(piece, fmt)
                for zs, buf, s in devs:
                    assert buf.at(s * bps) % 16 != 0 or fmt == "c64"
                    zs.push_dev(buf.at((s + done) * bps, n * bps), fmt, n)
                done += n
                lo = max(0, done - cap)
                ring = host.ring()
                worst = max(worst, _check_ring(ring, want[lo:done], want64[lo:done], detector, (fmt, detector, cap, n, "host")))
                for name, zs in (("dev+1", d1), ("dev+2", d2), ("dev+3", d3), ("max_host=1", c1), ("max_host=3", c3),
                                 ("max_host=8", c8)):
                    other = zs.ring()
                    _check_ring(other, want[lo:done], want64[lo:done], detector, (fmt, detector, cap, n, name))
                    assert _same_bits(other, ring), (fmt, detector, cap, n, name)       # in addition to the contract
            assert host.view()[0].total == done == sum(lengths)
    print(f"[{fmt} {detector} cap={cap}] {len(lengths)} pushes, 7 routes"
          + (f", worst DB error {worst:.2e} dB" if detector == "db" else ", bit for bit"))


# ---------------------------------------------------------------------------------------------------- 2. extremes
def _extreme_blocks():
    parts = zc.extreme_parts()
    re, im = np.meshgrid(parts, parts, indexing="ij")
    c64 = np.empty(re.size, dtype=np.complex64)
    c64.real, c64.imag = re.reshape(-1), im.reshape(-1)
    f32r = np.concatenate([parts, parts[::-1], np.roll(parts, 5)])
    return {"c64": c64, "f32r": f32r}


@pytest.mark.parametrize("fmt", ["c64", "f32r"])
def test_extreme_samples_through_each_detector(fmt):
    raw = _extreme_blocks()[fmt]
    re, im = zc.unpack(raw, fmt)
    assert _same_bits(re, raw.real if fmt == "c64" else raw)       # the unpack of the contract keeps NaN payloads
    n = re.size
    assert n >= 3 + 16 + 7                                        # head, several groups and a tail
    with np.errstate(all="ignore"):
        mag = zc.detect(re, im, "mag")
        db = zc.detect(re, im, "db", 0.0, 0.0)
        p32 = re * re + im * im
    tiny = np.finfo(F32).tiny
    assert np.isnan(mag).any() and np.isinf(mag).any() and ((p32 > 0) & (p32 < tiny)).any() and (p32 == 0).any()
    assert np.isneginf(db).any() and np.isposinf(db).any() and np.isnan(db).any()
    cap, worst = 1021, 0.0
    for lead in (1, 2, 3, 4):                                     # the block starts at every 16-byte residue of the ring
        with _Zs(cap, detector="real") as zs:
            zs.push(np.zeros(lead * ITEMS[fmt], dtype=raw.dtype), fmt)
            zs.push(raw[:5], fmt)
            zs.push(raw[5:], fmt)
            assert np.array_equal(_u32(zs.ring()[lead:]), _u32(re)), (fmt, lead, "REAL: the input bits, NaN payloads included")
        with _Zs(cap, detector="mag") as zs:
            zs.push(np.zeros(lead * ITEMS[fmt], dtype=raw.dtype), fmt)
            zs.push(raw, fmt)
            got = zs.ring()[lead:]
            nan = np.isnan(mag)
            assert np.array_equal(np.isnan(got), nan) and _same_bits(got[~nan], mag[~nan]), (fmt, lead, "MAG")
        with _Zs(cap, detector="db", log_floor=0.0, offset_db=0.0) as zs:
            zs.push(np.zeros(lead * ITEMS[fmt], dtype=raw.dtype), fmt)
            zs.push(raw, fmt)
            got = zs.ring()[lead:]
            fin = np.isfinite(db)
            nan = np.isnan(db)
            assert np.array_equal(np.isnan(got), nan) and _same_bits(got[~fin & ~nan], db[~fin & ~nan]), (fmt, lead, "DB")
            # finite ones: the float32 power is the restatement's, bit for bit; the logarithm of it within 1e-3 dB
            want = 10.0 * np.log10(p32[fin].astype(np.float64))
            off = np.abs(got[fin].astype(np.float64) - want)
            assert off.max() <= 1e-3, (fmt, lead, off.max())
            worst = max(worst, float(off.max()))
    print(f"[{fmt}] {n} extreme samples: REAL bits, MAG bit for bit ({int(((p32 > 0) & (p32 < tiny)).sum())} denormal "
          f"powers), DB -inf / inf / NaN in place, worst finite DB error {worst:.2e} dB")


# ---------------------------------------------------------------------------------------------------- 3. trigger
LO, HI, LEVEL = F32(-0.25), F32(0.5), 0.1


def _wrap_total(cap, nd):
    """A total that puts the physical wrap in the middle of the search range."""
    se = cap - nd
    ss = max(0, se - 8 * nd)
    return cap + (cap - (ss + se) // 2)


SWEEPS = [(97, 5, "short"), (97, 5, "full"), (97, 5, "wrap"), (97, 5, 5), (97, 5, 6), (97, 5, 7),
          (389, 20, "short"), (389, 20, "full"), (389, 20, "wrap"),
          (4096, 100, "short"), (4096, 100, "full"), (4096, 100, "wrap")]


@pytest.mark.parametrize("mode", ["rise", "fall"])
@pytest.mark.parametrize("cap,nd,which", SWEEPS)
def test_one_crossing_at_every_position(cap, nd, which, mode):
    total = {"short": cap - 3, "full": cap, "wrap": _wrap_total(cap, nd)}.get(which, which)
    plan = zc.view_plan(total, cap, nd, mode)
    held, base = plan["held"], plan["base"]
    a, b = (LO, HI) if mode == "rise" else (HI, LO)
    both = np.concatenate([np.full(total, a, dtype=F32), np.full(total, b, dtype=F32)])
    if which == "wrap":                                           # ring pair (cap - 1, 0) lies inside the search range
        ss, se = plan["search"]
        assert ss < cap - total % cap - 1 < se - 2
    starts, hits = set(), {}
    with _Zs(cap) as zs, _aligned(both.nbytes) as dev:
        dev.put(both)
        for i in range(held - 1):
            k = base + i + 1                                      # the history: k samples before the step, the rest after
            history = both[total - k:2 * total - k]
            assert history[base + i] == a and history[base + i + 1] == b
            zs.reset()
            src = 4 * (total - k)
            zs.push_dev(dev.at(src, 4 * (total - held)), "f32r", total - held)     # the part that has left the ring,
            zs.push_dev(dev.at(src + 4 * (total - held), 4 * held), "f32r", held)  # then the ring: two launches when it starts inside
            info, _ = _check_view(zs, history, mode, LEVEL, nd, tag=(cap, nd, total, mode, i))
            starts.add(info.start)
            hits[i] = info.triggered
            if info.triggered:
                assert info.start == base + i + 1
    # what the sweep must have met (section 4.10): first and last pair of the range, the pair that must not count, a
    # pair beyond the look-back
    if plan["search"] is None:
        assert held - nd in (0, 1) and not any(hits.values()) and starts == {plan["free_start"]}
    else:
        ss, se = plan["search"]
        assert hits[ss] == 1 and hits[se - 2] == 1 and hits[se - 1] == 0 and all(hits[i] for i in range(ss, se - 1))
        assert not any(hits[i] for i in range(se - 1, held - 1)) and not any(hits[i] for i in range(0, ss))
        assert plan["free_start"] in starts and len(starts) == se - 1 - ss + 1
        if which in (5, 6, 7):
            assert se == 2 and (ss, len(starts)) == (0, 2)
        elif cap > 9 * nd + 2:
            assert ss > 0
    print(f"cap={cap} n_display={nd} total={total} {mode}: {held - 1} positions, {sum(hits.values())} triggered, "
          f"search {plan['search']}")


def test_the_last_of_many_crossings_in_each_workgroups_share():
    cap, nd = 6000, 600
    se = cap - nd
    ss = se - 8 * nd
    n_pairs = se - 1 - ss
    grid = -(-n_pairs // 1024)
    assert n_pairs > 4 * 1024 and grid == 5                       # several workgroups, about four pairs per lane
    stride = grid * 256
    # the pair index j (from ss) of the last hit: first, last and seam lanes of the first and of the last workgroup
    last_js = [0, 1, 255, 256, stride - 256, stride - 1, stride, stride + 255, 2 * stride - 1, 2 * stride + 1024,
               n_pairs - 2, n_pairs - 1]
    for total in (cap, cap + 1234):                               # the second puts the physical wrap inside the range
        base = total - cap
        for mode in ("rise", "fall"):
            with _Zs(cap) as zs:
                for j in last_js:
                    i = ss + j
                    e = np.where(np.arange(total) % 2 == (base + i) % 2, LO, HI).astype(F32)   # a crossing at every pair
                    if mode == "fall":
                        e = np.where(e == LO, HI, LO).astype(F32)
                    e[base + i + 1:] = e[base + i + 1]            # ... and none behind pair i
                    seg = e[base + ss:base + se]
                    want = zc.crossings(seg[:i - ss + 2], LEVEL)[0 if mode == "rise" else 1]
                    assert want == (j + 2) // 2 and zc.crossings(seg[i - ss + 1:], LEVEL) == (0, 0)
                    zs.reset()
                    zs.push(e[:base], "f32r")
                    zs.push(e[base:], "f32r")
                    info, _ = _check_view(zs, e, mode, LEVEL, nd, tag=(total, mode, j))
                    assert info.triggered == 1 and info.start == base + i + 1
    print(f"{len(last_js)} last hits over {n_pairs} pairs in {grid} workgroups, rise and fall, with and without the wrap")


def test_trigger_levels_equal_rounded_infinite_and_nan():
    inf, nan = F32(np.inf), F32(np.nan)
    s7 = F32(0.7)
    pad = [0.0] * 9                                               # the window (n_display 4) and what lies behind it
    cases = [
        ("level equals the upper sample", [0, 0.25, 0.5, 0.25] + pad, 0.5),
        ("level equals the lower sample", [0, 0.5, 0.75, 0.5, 0.25] + pad, 0.5),
        ("0.7 against float32(0.7)", [0, s7, 0, s7] + pad, 0.7),
        ("a level that is a sample only after rounding", [0, 0.5, 0] + pad, 0.5 + 1e-12),
        ("0.0 against -0.0", [-1, -0.0, -1, 0.0, -0.0, -1] + pad, 0.0),
        ("-0.0 against 0.0", [-1, 0.0, -1] + pad, -0.0),
        ("+inf against an inf sample", [0, inf, 0, 1e38, 0] + pad, float("inf")),
        ("-inf", [0, -inf, 0, -inf, -inf, 1] + pad, float("-inf")),
        ("NaN", [0, 1, 0, 1, nan, 0] + pad, float("nan")),
        ("1e39 rounds to inf", [0, inf, 3e38, inf, 0] + pad, 1e39),
        ("-1e39 rounds to -inf", [0, -inf, 0] + pad, -1e39),
        ("NaN samples beside a crossing", [0, nan, 1, 0, 1, nan, 0, nan, nan, 1, 0] + pad, 0.5),
        ("NaN below, then a real crossing", [0, 1, 0, nan, 1, 0] + pad, 0.5),
    ]
    met = set()
    with _Zs(97) as zs:
        for name, values, level in cases:
            e = np.array(values, dtype=F32)
            for mode in ("rise", "fall"):
                for nd in (4, 3):
                    zs.reset()
                    zs.push(e, "f32r")
                    info, _ = _check_view(zs, e, mode, level, nd, tag=(name, mode))
                    met.add((name, mode, info.triggered))
                    # the statistics over everything held, at the same level
                    full, _ = _check_view(zs, e, "free_run", level, e.size, tag=(name, "statistics"))
                    if np.isnan(level):
                        assert (info.triggered, full.n_at_or_above, full.n_rise, full.n_fall) == (0, 0, 0, 0)
            print(f"{name}: level {level!r}, start {info.start}, triggered {info.triggered}")
    # the cases discriminate: each level triggers in at least one direction, except NaN and -inf (nothing lies below
    # -inf), which never do
    for name, _, level in cases:
        fired = {m for (nm, m, t) in met if nm == name and t}
        assert bool(fired) != bool(np.isnan(level) or level < -3.5e38), (name, fired)


# ---------------------------------------------------------------------------------------------------- 4. view
def _as_i8(e, rng):
    """Interleaved int8 whose REAL detector is e exactly (multiples of 2^-7 below 1)."""
    raw = np.empty((e.size, 2), dtype=np.int8)
    raw[:, 0] = np.rint(e.astype(np.float64) * 128.0).astype(np.int8)
    raw[:, 1] = rng.integers(-128, 128, e.size)
    assert np.array_equal(zc.detect(*zc.unpack(raw, "i8"), "real"), e)
    return raw.reshape(-1)


@pytest.mark.parametrize("length,points", zc.VIEW_SHAPES)
def test_view_seams_teams_and_strides(length, points):
    rng = np.random.default_rng(length + (points or 0))
    e, cap, start = zc.train_case(length, length)
    columns = ("minmax", "sample", "mean") if points else ("minmax",)
    with _Zs(cap) as zs:
        zs.push(_as_i8(e, rng), "i8")
        for column in columns:
            info, out = _check_view(zs, e, "rise", 0.0, length, points or 0, column, exact_mean=True, tag=(length, points, column))
            assert info.start == start and info.n_rise + info.n_fall == length - 1
        # the free-run window at the end of the history too (another start, another residue)
        _check_view(zs, e, "free_run", 0.0, length, points or 0, "mean", exact_mean=True, tag=(length, points, "free run"))
        # NaNs at the seams: the same train as float32, a few samples replaced
        nans = zc.nan_positions(length, points)
        if nans:
            f = e.copy()
            f[start + np.array(nans)] = np.nan
            assert zc.view(f, cap, length, "rise", 0.0)[0] == start                     # the trigger pair is untouched
            zs.reset()
            zs.push(f, "f32r")
            for column in columns:
                info, out = _check_view(zs, f, "rise", 0.0, length, points or 0, column, tag=(length, points, column, "NaN"))
                assert info.start == start and np.isnan(info.min) and np.isnan(info.mean)
                assert info.n_rise + info.n_fall < length - 1
    print(f"L={length} points={points}: window at {start % cap} of {cap}, n_rise + n_fall = {length - 1}, exact sums, "
          f"{len(nans)} NaN positions")


def test_out_dev_out_host_and_both_give_the_same_bits():
    nat = _nat()
    length = 1024 * 3 + 1
    rng = np.random.default_rng(5)
    e, cap, start = zc.train_case(length, 99)
    with _Zs(cap) as zs, _aligned(4 * (length + 64)) as dev:
        zs.push(_as_i8(e, rng), "i8")
        for points, column, n_out in ((0, "minmax", length), (3, "minmax", 6), (300, "minmax", 600), (300, "mean", 300)):
            chunk = zc.view(e, cap, length, "rise", 0.0)[2]
            want = chunk if points == 0 else zc.columns(chunk, points, column).astype(F32).reshape(-1)
            _, host_only = _check_view(zs, e, "rise", 0.0, length, points, column, exact_mean=True)
            got = {}
            for name, host in (("dev only", False), ("both", True)):
                dev.put(np.full(length + 64, SENTINEL, dtype=F32))
                info, out = zs.view("rise", 0.0, length, points, column, host=host, dev_ptr=dev.at(16))
                back = dev.get(length + 64, F32)
                assert np.all(back[:4] == SENTINEL) and np.all(back[4 + n_out:] == SENTINEL), (points, column, name)
                got[name] = back[4:4 + n_out]
                assert (info.start, info.triggered, info.length) == (start, 1, length)
                _check_info(info, chunk, 0.0, True)
                if host:
                    assert _same_bits(out, got[name])
            assert _same_bits(host_only, want) and _same_bits(got["dev only"], want) and _same_bits(got["both"], want)
        info = nat.ZspanInfo()
        host = np.zeros(length, dtype=F32)
        for off in (1, 2, 3):
            rc = nat.lib.tdsa_zspan_view(zs.h, nat.ZS_RISE, 0.0, length, 0, 0, C.byref(info),
                                         host.ctypes.data_as(C.c_void_p), dev.at(off))
            assert rc == ERR_ARG and "aligned" in nat.lib.tdsa_last_error_string().decode()
    print("out_dev only / out_host only / both: the same bits, sentinels kept, odd pointers refused")


def test_read_back_on_both_sides_of_the_bounce_threshold():
    edge = 1 << 21                                                # 8 MiB of floats: the last size that bounces
    cap = edge + 1 + PAD
    rng = np.random.default_rng(21)
    e = zc.crossing_train(cap + 1000, rng)
    e[::3] *= F32(0.5)
    assert np.all(e[1:] != e[:-1]) and zc.sum_is_exact(e, 2.0 ** -8)
    with _Zs(cap, max_host=1 << 20) as zs:
        zs.push(e, "f32r")
        for nd in (edge, edge + 1):
            info, out = _check_view(zs, e, "free_run", 0.0, nd, exact_mean=True, tag=nd)
            assert out.size == nd
            info, out = _check_view(zs, e, "fall", 0.0, nd, exact_mean=True, tag=nd)
            assert info.triggered == 1
    print(f"chunks of {edge} (bounce) and {edge + 1} floats (direct copy) match the contract")


# ---------------------------------------------------------------------------------------------------- 5. totals past 2^32
def _i8_block(rng, n):
    """Interleaved int8 with a slow square wave in I (crossings of 0.1 every 37 samples) and noise."""
    i = np.where((np.arange(n) // 37) % 2 == 0, -40, 60) + rng.integers(-9, 10, n)
    raw = np.stack([i, rng.integers(-128, 128, n)], axis=1).astype(np.int8)
    return raw.reshape(-1)


def test_totals_past_2_to_the_31_and_2_to_the_32():
    from topdogspectrumanalyser_amd import ZeroSpan
    nat = _nat()
    rate, cap, big = 500.0, 1000, 1 << 30
    rng = np.random.default_rng(2 ** 31 - 1)
    level = 0.1

    def real(raw):
        return zc.detect(*zc.unpack(raw, "i8"), "real")

    class Stream:
        """The last `cap` detected samples of a stream and where they begin."""

        def __init__(self, zs):
            self.zs, self.tail, self.total = zs, np.empty(0, dtype=F32), 0

        def add(self, raw_tail, n):
            self.tail = np.concatenate([self.tail, real(raw_tail)])[-cap:]
            self.total += n

        def check(self, mode, nd, points=None, column="minmax"):
            origin = self.total - self.tail.size
            start, trig, chunk = zc.view(self.tail, cap, nd, mode, level, origin=origin)
            v = self.zs.view(mode=mode, level=level, n_display=nd, points=points, column=column)
            print(f"total={self.total} ({self.total / 2 ** 31:.3f} x 2^31) {mode} n_display={nd} points={points}: start "
                  f"{v.start} / {start}, triggered {int(v.triggered)} / {trig}")
            assert (v.total, v.start, int(v.triggered), v.length) == (self.total, start, trig, chunk.size)
            if points is None:
                assert _same_bits(v.samples, chunk)
                assert v.time_s.dtype == np.float32 and _same_bits(v.time_s, np.arange(chunk.size, dtype=F32) / rate)
            else:
                P, b = zc.cells(chunk.size, points)
                want = zc.columns(chunk, points, column)
                assert _same_values(v.columns, want) if column == "minmax" else _same_bits(v.columns, want)
                assert np.array_equal(v.time_s, np.array(b[:-1], dtype=np.float64) / rate)
            st = zc.statistics(chunk, level)
            assert (v.n_at_or_above, v.n_rise, v.n_fall) == (st["n_at_or_above"], st["n_rise"], st["n_fall"])
            assert _same_values(v.min, st["min"]) and _same_values(v.max, st["max"]) and v.mean == st["mean"]
            return v

    with ZeroSpan(rate) as za, ZeroSpan(rate) as zb, _aligned(2 * big) as dev:
        assert za.capacity == cap and cap & (cap - 1) != 0
        a, b = Stream(za), Stream(zb)

        def push_big():
            """2^30 samples from device memory: only the last `cap` of them are read, and only those were written."""
            raw = _i8_block(rng, cap)
            dev.put(raw, 2 * (big - cap))
            za.push_device(None, nat.IN_I8, dev.ptr, big)
            a.add(raw, big)
            # the second handle starts again at 0 after every step, with a stream of its own through the same buffer
            zb.reset()
            b.tail, b.total = np.empty(0, dtype=F32), 0
            zb.push_device(None, nat.IN_I8, dev.at(2 * (big - cap - 7), 2 * (cap + 7)), cap + 7)
            b.add(raw, cap + 7)
            small = _i8_block(rng, 123)
            zb.push(small)
            b.add(small, 123)
            for mode in ("free_run", "rise", "fall"):
                b.check(mode, 100)
            b.check("free_run", cap)

        def push_small(sizes):
            for n in sizes:
                raw = _i8_block(rng, n)
                za.push(raw)
                a.add(raw, n)

        push_big()
        push_big()
        assert a.total == 1 << 31                                 # 1. exactly 2^31
        for mode, nd in (("free_run", cap), ("rise", 100), ("fall", 7), ("free_run", 3)):
            a.check(mode, nd)
        push_big()                                                # 2. past 2^31, then pushes of 1 .. 7 samples
        push_small(range(1, 8))
        assert a.total == 3 * big + 28
        for mode in ("rise", "fall"):
            v = a.check(mode, 100)
            assert v.triggered
            for column in ("minmax", "sample"):
                a.check(mode, 100, points=7, column=column)
        a.check("free_run", cap)
        push_big()                                                # 3. past 2^32
        push_big()
        assert a.total == 5 * big + 28 > 1 << 32
        a.check("free_run", cap)
        a.check("rise", 100)
        # 4. a crossing carried over the physical wrap by small pushes: low up to position cap - 1, high from 0 on
        to_wrap = (-a.total) % cap
        assert to_wrap > 60
        low = np.stack([np.full(to_wrap, -40), np.zeros(to_wrap)], axis=1).astype(np.int8).reshape(-1)
        high = np.stack([np.full(60, 60), np.zeros(60)], axis=1).astype(np.int8).reshape(-1)
        za.push(low[:2 * (to_wrap - 1)])
        a.add(low[:2 * (to_wrap - 1)], to_wrap - 1)
        za.push(np.concatenate([low[-2:], high[:2]]))             # the pair (cap - 1, 0) in one push ...
        a.add(np.concatenate([low[-2:], high[:2]]), 2)
        za.push(high[2:])
        a.add(high[2:], 59)
        v = a.check("rise", 50)
        assert v.triggered and v.start % cap == 0 and v.start > 1 << 32
        a.check("fall", 50)
        a.check("free_run", cap)
        v = a.check("rise", 50, points=16, column="minmax")
        assert v.start % cap == 0


# ---------------------------------------------------------------------------------------------------- 6. Python layer
def _small_ring_history(rng, n):
    """Two levels around LEVEL with a different multiple of 2^-8 on every sample: all values distinct, all sums exact."""
    e = np.where(rng.integers(0, 2, n) == 1, 0.5, -0.25) + rng.permutation(n) / 256.0
    assert n <= 45 and zc.sum_is_exact(e, 2.0 ** -8)
    return e.astype(F32)


@pytest.mark.parametrize("cap", [4, 5])
def test_the_smallest_rings_through_the_python_layer(cap):
    from topdogspectrumanalyser_amd import ZeroSpan
    rng = np.random.default_rng(cap)
    sizes = [int(v) for v in rng.permutation(np.arange(1, 10))]
    e = _small_ring_history(rng, sum(sizes))
    assert sum(zc.crossings(e, LEVEL)) >= 8 and np.all(e[1:] != e[:-1])
    triggered = 0
    with ZeroSpan(1.0, buffer_s=float(cap)) as zs:
        assert zs.capacity == cap and zs.view().length == 0
        done = 0
        for n in sizes:
            assert zs.push(e[done:done + n]) == n
            done += n
            for nd in range(1, 7):
                for mode in ("free_run", "rise", "fall"):
                    start, trig, chunk = zc.view(e[:done], cap, nd, mode, LEVEL)
                    v = zs.view(mode=mode, level=LEVEL, n_display=nd)
                    assert (v.total, v.start, int(v.triggered), v.length) == (done, start, trig, chunk.size), (n, nd, mode)
                    assert _same_bits(v.samples, chunk)
                    st = zc.statistics(chunk, LEVEL)
                    assert (v.n_at_or_above, v.n_rise, v.n_fall) == (st["n_at_or_above"], st["n_rise"], st["n_fall"])
                    assert v.min == st["min"] and v.max == st["max"] and v.mean == st["mean"]   # multiples of 2^-6: exact
                    triggered += trig
                    c = zs.view(mode=mode, level=LEVEL, n_display=nd, points=3)
                    assert _same_values(c.columns, zc.columns(chunk, 3, "minmax")) and c.start == start
    assert triggered >= 10
    print(f"capacity {cap}: pushes of {sizes}, n_display 1 .. 6, all modes; {triggered} triggered views")


def test_stereo_blocks_column_times_and_the_empty_view():
    from topdogspectrumanalyser_amd import ZeroSpan
    rng = np.random.default_rng(6)
    rate = 48.0
    with ZeroSpan(rate) as zs:                                    # capacity 96
        v = zs.view(n_display=10)
        assert v.length == 0 and v.samples.size == 0 and np.isnan(v.duty_cycle) and np.isnan(v.pulse_rate_hz)
        assert np.isnan(v.min) and np.isnan(v.max) and np.isnan(v.mean) and v.time_s.size == 0
        c = zs.view(n_display=10, points=4)
        assert c.length == 0 and c.columns.size == 0 and c.time_s.size == 0 and np.isnan(c.duty_cycle)
        history = np.empty(0, dtype=F32)
        for n, dtype in ((1, np.float32), (7, np.float64), (50, np.float32), (61, np.int16)):
            raw = (rng.standard_normal((n, 2)) * 100).astype(dtype)
            want = raw.mean(axis=1).astype(F32)
            assert np.any(want != raw[:, 0].astype(F32))
            assert zs.push(raw) == n
            history = np.concatenate([history, want])
            v = zs.view(n_display=96)
            assert _same_bits(v.samples, history[-96:]), (n, dtype)
        for length, points in ((96, 7), (50, 50), (37, 5), (96, 96), (10, 16)):
            start, trig, chunk = zc.view(history, 96, length, "rise", 0.0)
            for column in ("minmax", "sample", "mean"):
                v = zs.view(mode="rise", level=0.0, n_display=length, points=points, column=column)
                P, b = zc.cells(length, points)
                assert v.start == start and np.array_equal(v.time_s, np.array(b[:-1], dtype=np.int64) / rate)
                want = zc.columns(chunk, points, column)
                assert _same_values(v.columns, want) if column == "minmax" else (
                    _same_bits(v.columns, want) if column == "sample" else
                    np.all(np.abs(v.columns - want) <= 2.0 ** -23 * np.max(np.abs(chunk))))
                assert v.duty_cycle == v.n_at_or_above / length and v.pulse_rate_hz == v.n_rise * rate / length


@pytest.mark.parametrize("D,max_host,tpp", [(2, 1, 34), (4096, 1000, 2)])
def test_tuned_channel_with_blocks_around_one_decimation(D, max_host, tpp):
    from topdogspectrumanalyser_amd import ZeroSpan
    from topdogspectrumanalyser_amd.zoom import DownConverter, design_decimator
    rng = np.random.default_rng(D)
    fs, f = 1e6, 1.25e5
    blocks = [1, D - 1, D, D + 1, 1, D + 1, D, D - 1, 1, 3 * D + 1]
    n = sum(blocks)
    x = (0.7 * np.exp(2j * np.pi * f / fs * np.arange(n)) * (1 + 0.5 * np.sin(np.arange(n) / (3.0 * D)))
         + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    taps = design_decimator(D, tpp)
    with DownConverter(D, fs, f, taps, max_host_samples=1 << 16) as ddc:
        y = ddc.process(x)
    assert y.size == -(-n // D) and y.size >= 9 and np.all(np.abs(np.diff(np.abs(y))) > 0)
    for det in ("real", "mag"):
        want = zc.detect(y.real, y.imag, det)
        with ZeroSpan(fs, detector=det, decimation=D, offset_hz=f, taps=taps, max_host_samples=max_host,
                      buffer_s=64.5 * D / fs) as zs:
            assert zs.capacity == 64 and max_host < D
            got, done = 0, 0
            for b in blocks:
                got += zs.push(x[done:done + b])
                done += b
                v = zs.view(n_display=64)
                assert v.total == got == -(-done // D) and _same_bits(v.samples, want[:got]), (det, b, done)
        print(f"D={D} max_host_samples={max_host} {det}: {len(blocks)} blocks, {got} outputs, bit for bit")
