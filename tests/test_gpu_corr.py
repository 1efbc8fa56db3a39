"""The correlation search on the device (tdsa_corr_*) against tests/corr_contract.py.

Arithmetic: m and c of every window (the metric trace) and c1, c2, e of every match within the bounds of the header.
Matches: every input is first classified on the CPU in float64 - each window a sure match, surely none, or undecided
within twice the bound of m - and no input here leaves a window undecided; then indices, counts, stored ordinals and
n_lost are np.array_equal.  Split invariance: records, summaries and trace bit for bit, with no reference to the
contract."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import corr_contract as cc
from kernel_build import CSRC
from topdogspectrumanalyser_amd import Channelizer, DeviceBuffer, DownConverter, SpectrumEngine
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd.correlate import Correlator, barker, zadoff_chu

pytestmark = pytest.mark.gpu


def _const(name):
    src = open(os.path.join(CSRC, "tdsa_corr.hpp")).read()
    expr = re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)
    return int(eval(re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), expr)))


T = _const("kCorrTile")
R = _const("kCorrWindowsPerThread")
MAX_TILES = _const("kCorrMaxLaunchTiles")
LS = (2, 3, 16, 17, 64, 255, 1024)
DTYPE = {cc.I8: np.int8, cc.U8: np.uint8, cc.C64: np.complex64}
THR = 0.6
DISTINCT = 4                                     # the streams of a 256-stream case repeat after this many


def sizes(L):
    return (L - 1, L, L + 1, T - 1, T, T + 1, T + L - 1, T + L, 3 * T + 1)


def distances(L):
    return (1, 2, L, T - 1, T, T + 1, 65536)


@functools.lru_cache(maxsize=None)
def reference(L):
    """Zadoff-Chu of the next prime cut to L (L = 2, 3: a Barker code): unit amplitude, low sidelobes."""
    if L <= 3:
        return barker(L) * np.complex64(np.exp(0.3j))
    p = L
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return zadoff_chu(p, 1 if p < 5 else 2)[:L].copy()


def _per(fmt):
    return 1 if fmt == cc.C64 else 2


def quantize(x, fmt):
    """The complex signal x as raw samples of the format (interleaved bytes, or complex64)."""
    if fmt == cc.C64:
        return x.astype(np.complex64)
    iq = np.stack([x.real, x.imag], axis=-1).reshape(-1)
    if fmt == cc.I8:
        return np.clip(np.rint(iq * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(iq * 127.5 + 127.5), 0, 255).astype(np.uint8)


def spots(L, n):
    """Where the shape cases plant the reference in n samples: the first and the last window, the middle, and around
    the first tile seam; no two closer than L + 2."""
    nw = n - L + 1
    kept = []
    for p in (0, nw - 1, T - 1, T + L + 3, nw // 2, 7 * R + 1, 2 * T - 2):
        if 0 <= p < nw and all(abs(p - q) >= L + 2 for q in kept):
            kept.append(p)
    return sorted(kept)


@functools.lru_cache(maxsize=None)
def signal(L, n, fmt, seed, at=None, amp=0.5, noise=0.02):
    """Raw samples of one stream: noise with the reference planted at `at` (default: spots), the k-th under k times more
    interference of its own, so that two of them within W of each other never tie.  With L of 2 or 3 any noise correlates: there the background is a
    constant, to which these references answer with m = 0 and 1 / 9."""
    rng = np.random.default_rng([L, n, seed])
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if L <= 3:
        x = 0.1 * x + complex(0.1, 0.05)
    r = reference(L).astype(np.complex128)
    for k, p in enumerate(spots(L, n) if at is None else at):
        x[p:p + L] += amp * np.exp(1j * rng.uniform(0, 2 * np.pi)) * r + 0.05 * k * amp * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    out = quantize(x, fmt)
    out.setflags(write=False)
    return out


class Want:
    """The contract's view of one stream's raw samples: the windows, and per min_distance the sure decisions."""

    def __init__(self, L, raw, fmt):
        self.L = L
        self.w = cc.Windows(cc.samples(raw, fmt), reference(L))
        self._dec = {}

    def sure(self, thr, W):
        """The indices of the sure matches; asserts that no window is undecided within twice the bound of m."""
        key = (float(thr), int(W))
        if key not in self._dec:
            d = cc.decide(self.w.m, 2.0 * self.w.b_m, thr, W)
            assert not (d == cc.OPEN).any(), (self.L, self.w.n, key, np.flatnonzero(d == cc.OPEN)[:5])
            self._dec[key] = np.flatnonzero(d == cc.YES)
        return self._dec[key]


@functools.lru_cache(maxsize=64)
def want_of(L, n, fmt, seed, at=None):
    return Want(L, signal(L, n, fmt, seed, at), fmt)


def same(p, wants, n_total, flushed, tag="", thr=THR):
    """The handle's state against the contract's view of its streams (wants[c % len(wants)])."""
    sums = p.read_summaries()
    W = p.min_distance
    for c in range(p.streams):
        wt = wants[c % len(wants)]
        nd = wt.w.n if flushed else max(0, wt.w.n - W)
        idx = wt.sure(thr, W)
        idx = idx[idx < nd]
        s = sums[c]
        got = (int(s["n_total"]), int(s["n_windows"]), int(s["n_decided"]), int(s["n_matches"]), int(s["n_lost"]), int(s["n_bad"]),
               int(s["flushed"]))
        assert got == (n_total, wt.w.n, nd, idx.size, max(0, idx.size - p.capacity), int(wt.w.bad.sum()), int(flushed)), (tag, c, got)
    for c in sorted({0, 1, p.streams // 2, p.streams - 1} & set(range(p.streams))):
        wt = wants[c % len(wants)]
        nd = wt.w.n if flushed else max(0, wt.w.n - W)
        idx = wt.sure(thr, W)
        idx = idx[idx < nd][:p.capacity]
        t = p.read(c)
        assert np.array_equal(t.index, idx), (tag, c, t.index[:8], idx[:8])
        within(t.records, wt.w, (tag, c))


def within(rec, w, tag=""):
    """The float fields of match records within the bounds of the header."""
    i = rec["index"]
    for name, val, bound in (("metric", w.m, w.b_m), ("energy", w.e, w.b_e), ("c1_re", w.c1.real, w.b_c1.real),
                             ("c1_im", w.c1.imag, w.b_c1.imag), ("c2_re", w.c2.real, w.b_c2.real), ("c2_im", w.c2.imag, w.b_c2.imag)):
        err = np.abs(rec[name].astype(np.float64) - val[i])
        ok = err <= bound[i]
        assert ok.all(), (tag, name, i[~ok][:4], err[~ok][:4], bound[i][~ok][:4])


def gap_of(fmt, L, count):
    """`count` samples that would match if they were read: the reference, strong."""
    return quantize(np.resize(0.9 * reference(L).astype(np.complex128), count), fmt)


def feed_device(p, x2d, fmt, extra=0, offset=0, engine=None):
    """The streams through the device entry point: `offset` samples into a 16-byte aligned buffer, in_stride = n + extra,
    the gaps and the lead filled with the reference.  Waits, so the buffer may go."""
    x2d = np.ascontiguousarray(x2d)
    per, unit = _per(fmt), 8 if fmt == cc.C64 else 2
    n = x2d.shape[1] // per
    stride = n + extra
    full = np.empty((x2d.shape[0], stride * per), dtype=DTYPE[fmt])
    full[:, :n * per] = x2d
    if extra:
        full[:, n * per:] = gap_of(fmt, p.L, extra)
    with DeviceBuffer(full.nbytes + offset * unit + 16) as buf:
        assert buf.ptr % 16 == 0
        if offset:
            buf.put(gap_of(fmt, p.L, offset))
        buf.put(full, offset * unit)
        p.process_device(engine, buf.at(offset * unit, full.nbytes), n, stride, fmt)
        p.read_summaries()


def feed(p, x2d, fmt, how):
    """how: 0 = the host entry point; k > 0: the device entry point with stride n + (0, 1, 7)[k - 1]."""
    if how == 0:
        p.process(x2d)
    else:
        feed_device(p, x2d, fmt, (0, 1, 7)[how - 1])


def stack(L, n, fmt, C_, seed=0):
    return np.stack([signal(L, n, fmt, seed + (c % DISTINCT)) for c in range(C_)]), [want_of(L, n, fmt, seed + c)
                                                                                   for c in range(min(C_, DISTINCT))]


# ---- shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_one_stream_every_reference_length_stream_length_and_min_distance(L):
    """The full cross-product of L, n and W for one stream; the format, the entry point and the stride rotate over it, so
    that every one of them meets every L, every n and every W.  Each case is checked undecided tail and all, then
    flushed and checked again."""
    with Correlator(reference(L), 1, 64, max_host_samples=3 * T + 1) as p:
        for (i, n), (j, W) in itertools.product(enumerate(sizes(L)), enumerate(distances(L))):
            fmt, how = (i + j) % 3, (i + 2 * j + LS.index(L)) % 4
            x, wants = stack(L, n, fmt, 1)
            p.configure(THR, W)
            feed(p, x, fmt, how)
            same(p, wants, n, False, (L, n, W, fmt, how))
            p.flush()
            same(p, wants, n, True, (L, n, W, fmt, how, "flushed"))


@pytest.mark.parametrize("C_", (2, 3, 256))
@pytest.mark.parametrize("fmt", (cc.I8, cc.U8, cc.C64))
def test_more_streams_every_format_entry_point_and_stride(fmt, C_):
    """A covering subset for more than one stream: every L with a short, a seam and a long n, every W once per format."""
    cases = [(2, 2, 1), (3, T + 1, T + 1), (16, T + 15, 2), (17, 3 * T + 1, T - 1), (64, T, 64), (255, T + 255, T), (1024, 3 * T + 1, 1024),
             (16, 15, 16), (64, 3 * T + 1, 65536 if C_ < 256 else 1)]
    for k, (L, n, W) in enumerate(cases):
        with Correlator(reference(L), C_, 64, max_host_samples=C_ * n) as p:
            p.configure(THR, W)
            x, wants = stack(L, n, fmt, C_, seed=10)
            for how in ((0, 1 + k % 3) if C_ < 256 else (k % 4,)):
                p.reset()
                feed(p, x, fmt, how)
                same(p, wants, n, False, (L, n, W, how))
            p.flush()
            same(p, wants, n, True, (L, n, W, "flushed"))


@pytest.mark.parametrize("fmt", (cc.I8, cc.U8, cc.C64))
def test_a_base_pointer_one_and_three_samples_off_16_bytes(fmt):
    for C_, L in ((1, 17), (3, 64)):
        with Correlator(reference(L), C_, 64) as p:
            p.configure(THR, L)
            for n in (L + 1, T + 1, 3 * T + 1):
                x, wants = stack(L, n, fmt, C_, seed=20)
                for offset, extra in ((1, 0), (1, 1), (3, 4)):
                    p.reset()
                    feed_device(p, x, fmt, extra, offset)
                    same(p, wants, n, False, (C_, n, offset, extra))


# ---- arithmetic --------------------------------------------------------------------------------------------------
def _octaves(n, fmt, seed):
    """Noise whose amplitude steps through eight octaves in runs of 37 samples, so that windows of every L see several
    scales at once: a bound that is absolute where it should be relative fails on the quiet runs."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** -rng.integers(0, 9, n // 37 + 1).repeat(37)[:n]
    if fmt == cc.C64:
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)
    return np.clip(np.rint(rng.standard_normal(2 * n) * scale.repeat(2) * 60.0), -128, 127).astype(np.int8)


@pytest.mark.parametrize("fmt", (cc.C64, cc.I8))
@pytest.mark.parametrize("L", LS)
def test_every_window_of_random_input_within_the_bounds_of_the_header(L, fmt):
    """m and c of every window, through the trace, which is what the interface shows of a window that is no match; c1,
    c2 and e of every match, a third of the windows here (threshold 1e-6, min_distance 1).  The trace's c is formed by the
    library on the host from the ring's c1 and c2, so comparing it with their float32 sum says nothing about the
    kernel.  What does: the kernel's m, recomputed here in float32 from that c and the record's e, operation by operation
    - it comes out bit for bit only if the c the kernel squared is fl(c1 + c2)."""
    n = T + L + 300
    x = _octaves(n, fmt, L)
    w = cc.Windows(cc.samples(x, fmt), reference(L))
    assert w.n == T + 301                                 # int8 at the quiet end is mostly (0, 0): windows with e = 0, m = 0
    with Correlator(reference(L), 1, 4096, trace=w.n) as p:
        p.configure(1e-6, 1)                               # every local maximum is a match: a third of the windows
        p.process(x)
        p.flush()
        m, c = p.read_trace(0, 0, w.n)
        t = p.read(0)
    err_m = np.abs(m.astype(np.float64) - w.m)
    err_c = np.abs(c.real.astype(np.float64) - w.c.real), np.abs(c.imag.astype(np.float64) - w.c.imag)
    assert (err_m <= w.b_m).all(), np.flatnonzero(err_m > w.b_m)[:5]
    assert (m[w.bad] == 0).all() and t.n_bad == w.bad.sum()
    assert (err_c[0] <= w.b_c.real).all() and (err_c[1] <= w.b_c.imag).all()      # b_c: of the two bounds and the sum's own rounding
    assert len(t) > w.n // 5 and t.n_lost == 0
    within(t.records, w, L)
    i = t.index
    assert np.array_equal(c[i].real, t.c1_re + t.c2_re) and np.array_equal(c[i].imag, t.c1_im + t.c2_im)
    assert np.array_equal(m[i].view(np.uint32), t.metric.view(np.uint32))                 # the record's metric is the trace's
    f32 = np.float32
    with np.errstate(all="ignore"):
        again = (c[i].real * c[i].real + c[i].imag * c[i].imag) / (f32(cc.reference_energy(reference(L))) * t.energy)
    assert again.dtype == f32 and np.array_equal(again.view(np.uint32), t.metric.view(np.uint32)), np.flatnonzero(again != t.metric)[:5]
    assert np.array_equal(t.index, cc.matches(m, 1e-6, 1))      # the match rule on the device's own metric


# ---- matches against the contract ---------------------------------------------------------------------------------
def _run(L, x, fmt, W, at, thr=THR, capacity=256, limits=None, pieces=None, tag=""):
    """One stream through the device entry point (in `pieces`, if given) against the contract; flushes."""
    wt = Want(L, x, fmt)
    with Correlator(reference(L), 1, capacity) as p:
        p.configure(thr, W)
        if limits:
            p._debug_limits(*limits)
        per, k = _per(fmt), 0
        for m in pieces or (x.size // per,):
            feed_device(p, x[None, k * per:(k + m) * per], fmt, k % 3, k % 2)
            k += m
        assert k == x.size // per
        same(p, [wt], k, False, tag, thr)
        p.flush()
        same(p, [wt], k, True, tag, thr)
        got = p.read(0)
    if at is not None:
        assert got.index.tolist() == sorted(at)[:capacity], (tag, got.index, at)
    return got, wt


@pytest.mark.parametrize("d", range(-2, 3))
def test_peaks_at_every_offset_around_a_thread_a_wave_a_tile_a_launch_and_a_call_seam(d):
    """L = 16, W = 4, launches of one tile (2048 samples), calls of 5000, 700 and the rest.  The first new window of a
    launch or a call lies L - 1 before its first sample, so a window seam and a sample seam of each kind get a peak."""
    L, n, calls = 16, 3 * T + 100, (5000, 700)
    seams = (5 * R, 64 * R, T - (L - 1), 2 * T, calls[0] - (L - 1), sum(calls))
    at = tuple(s + d for s in seams)
    for fmt in (cc.C64, cc.I8):
        x = signal(L, n, fmt, 30 + d, at)
        _run(L, x, fmt, 4, at, limits=(1,), pieces=calls + (n - sum(calls),), tag=(d, fmt))


def test_two_peaks_w_and_w_plus_1_apart_across_a_tile_seam():
    """The weaker of two peaks W apart loses, whichever comes first; W + 1 apart both win.  The second is planted with
    less amplitude over the same noise, so the margins are far above the bound."""
    L, n = 16, 2 * T
    r = reference(L).astype(np.complex128)
    for W, first_stronger in itertools.product((L + 4, T - 1, T), (True, False)):
        for apart in (W, W + 1):
            rng = np.random.default_rng([W, apart])
            x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
            a = T - 3 if W < T - 1 else 5
            x[a:a + L] += (0.5 if first_stronger else 0.1) * r
            x[a + apart:a + apart + L] += (0.1 if first_stronger else 0.5) * r
            want = [a, a + apart] if apart > W else [a] if first_stronger else [a + apart]
            _run(L, x.astype(np.complex64), cc.C64, W, want, tag=(W, apart, first_stronger))


def test_identical_peaks_tie_bit_for_bit_and_the_first_wins():
    """One fixed order per window: the same samples give the same bits wherever the window lies.  Two copies of one
    burst W apart tie exactly, and the first wins; W + 1 apart both win.  The copies lie at different places in their
    threads, waves and tiles."""
    L, W, n = 64, 300, 2 * T + 1000
    rng = np.random.default_rng(5)
    burst = (0.01 * (rng.standard_normal(3 * L) + 1j * rng.standard_normal(3 * L))).astype(np.complex64)
    burst[L:2 * L] += reference(L) * np.complex64(0.5)
    for a, apart in ((T - 3 - L, W), (T - 70 - L, W + 1), (3, W), (T + 5, W + 1)):
        x = np.zeros(n, dtype=np.complex64)
        x[a:a + 3 * L] = burst
        x[a + apart:a + apart + 3 * L] += burst          # apart >= 3 L: they do not overlap
        with Correlator(reference(L), 1, 16, trace=n) as p:
            p.configure(0.9, W)
            p.process(x)
            p.flush()
            got = p.read(0)
            m, c = p.read_trace(0, 0, n - L + 1)
        assert np.array_equal(m[a:a + 2 * L + 1].view(np.uint32), m[a + apart:a + apart + 2 * L + 1].view(np.uint32))
        assert np.array_equal(c[a:a + 2 * L + 1], c[a + apart:a + apart + 2 * L + 1])
        assert got.index.tolist() == ([a + L] if apart == W else [a + L, a + L + apart]), (a, apart, got.index)
        assert got.n_bad == np.count_nonzero(m == 0) > 0     # the zeros between the bursts: e = 0


def test_a_peak_whose_window_straddles_two_calls_and_two_formats():
    """int8 samples, then the same values as complex64 (I / 128 is exact): the window at 2995 takes 5 samples of the first
    call from the history and 11 of the second.  Against the contract, and bit for bit against one int8 call."""
    L, n, cut = 16, 4000, 3000
    raw = signal(L, n, cc.I8, 40, (100, cut - 5, cut + 200))
    wt = Want(L, raw, cc.I8)
    as_c64 = (raw.astype(np.float32) * np.float32(1 / 128)).view(np.complex64)
    with Correlator(reference(L), 1, 16, trace=n) as p:
        p.configure(THR, 8)
        p.process(raw)
        p.flush()
        one = p.read(0), p.read_trace(0, 0, n - L + 1)
        p.reset()
        p.process(raw[:2 * cut])
        feed_device(p, as_c64[None, cut:], cc.C64, 1, 1)
        same(p, [wt], n, False, "two formats")
        p.flush()
        two = p.read(0), p.read_trace(0, 0, n - L + 1)
    assert one[0].index.tolist() == [100, cut - 5, cut + 200]
    assert np.array_equal(one[0].records, two[0].records) and one[0].summary == two[0].summary
    assert np.array_equal(one[1][0].view(np.uint32), two[1][0].view(np.uint32)) and np.array_equal(one[1][1], two[1][1])


# ---- split invariance: bits only ----------------------------------------------------------------------------------
def _noise(C_, n, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == cc.C64:
        return (0.3 * (rng.standard_normal((C_, n)) + 1j * rng.standard_normal((C_, n)))).astype(np.complex64)
    return rng.integers(-128, 128, (C_, 2 * n)).astype(np.int8)


def _state(p, n_windows):
    recs = [p.read(c) for c in range(p.streams)]
    k = min(p.trace, n_windows)
    trace = [p.read_trace(c, n_windows - k, k) for c in range(p.streams)] if k else []
    return p.read_summaries(), [t.records for t in recs], trace


def _same_bits(a, b, tag):
    assert np.array_equal(a[0], b[0]), (tag, a[0], b[0])
    for c, (ra, rb) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(ra, rb) and ra.tobytes() == rb.tobytes(), (tag, c)
    for c, (ta, tb) in enumerate(zip(a[2], b[2])):
        assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes(), (tag, c)


@pytest.mark.parametrize("fmt, L, W", [(cc.C64, 17, 5), (cc.I8, 64, T + 1), (cc.C64, 255, 300)])
def test_one_call_against_six_pieces_through_both_entry_points(fmt, L, W):
    """Noise and a low threshold: hundreds of marginal matches, every one of which a wrong bit would move."""
    pieces = (1, L - 1, T + 1, 500, 3 * T + 1, 64)
    n, per = sum(pieces), _per(fmt)
    x = _noise(2, n, fmt, L)
    nw = n - L + 1
    with Correlator(reference(L), 2, 4096, trace=nw) as p:
        p.configure(2.0 / L, W)
        p.process(x)
        one = _state(p, nw)
        assert one[0]["n_matches"].min() > (20 if W < 100 else 0) and (one[0]["n_decided"] == nw - W).all()
        p.reset()
        k = 0
        for i, m in enumerate(pieces):
            part = x[:, k * per:(k + m) * per]
            if i % 2:
                p.process(part)
            else:
                feed_device(p, part, fmt, i, i % 3)
            p.process_device(None, 4096, 0)              # n_in = 0: nothing happens, the pointer is not read
            p.process(x[:, :0])
            k += m
        _same_bits(one, _state(p, nw), "six pieces")
        p.flush()
        six = _state(p, nw)
        p.reset()
        feed_device(p, x, fmt, 7, 1)
        p.flush()
        _same_bits(six, _state(p, nw), "flushed")
        assert (six[0]["n_decided"] == nw).all() and (six[0]["flushed"] == 1).all()


@pytest.mark.parametrize("C_", (1, 3))
def test_launches_of_one_two_and_three_tiles_cut_a_call_of_seven_and_every_variant_gives_the_same_bits(C_):
    L, W, n = 64, 100, 6 * T + 11 + 63
    x = _noise(C_, n, cc.C64, 7 + C_)
    nw = n - L + 1
    with Correlator(reference(L), C_, 4096, trace=nw) as p:
        p.configure(2.0 / L, W)
        feed_device(p, x, cc.C64, 1)
        plain = _state(p, nw)
        assert plain[0]["n_matches"].min() > 20
        for tiles in (3, 2, 1):
            p.reset()
            p._debug_limits(tiles * C_)
            feed_device(p, x, cc.C64, tiles)
            _same_bits(plain, _state(p, nw), tiles)
        for variant in range(1, 8):                        # 4, 8, 16 windows per thread, packed or not, the reference from LDS or not
            p.reset()
            p._debug_limits(MAX_TILES, 15, variant)
            feed_device(p, x, cc.C64, 0, variant % 2)
            _same_bits(plain, _state(p, nw), ("variant", variant))


# ---- also ---------------------------------------------------------------------------------------------------------
def test_capacity_1_and_3_flush_and_the_minus_1_after_it():
    L, n = 16, 3 * T + 1
    at = tuple(range(50, n - 100, 617))
    x = signal(L, n, cc.C64, 50, at)
    for capacity in (1, 3):
        got, _ = _run(L, x, cc.C64, L, at, capacity=capacity, tag=capacity)
        assert len(got) == capacity and got.n_matches == len(at) and got.n_lost == len(at) - capacity
    with Correlator(reference(L), 1, 64) as p, DeviceBuffer.of(x) as d:
        p.configure(THR, 600)
        p.process(x)
        before = p.read(0)
        assert before.index.tolist() == [a for a in at if a < n - L + 1 - 600] and len(before) < len(at) and not before.flushed
        p.flush()
        p.flush()                                          # a second flush changes nothing
        after = p.read(0)
        assert after.index.tolist() == list(at) and after.flushed and after.n_decided == after.n_windows == n - L + 1
        err = lambda: nat.lib.tdsa_last_error_string().decode()
        text = "the correlator was flushed: it takes no samples until tdsa_corr_reset"
        assert nat.lib.tdsa_corr_process(p._h, cc.C64, x.ctypes.data_as(C.c_void_p), 10, 10) == -1 and err() == text
        assert nat.lib.tdsa_corr_process_dev(p._h, None, cc.C64, C.c_void_p(d.ptr), 10, 10) == -1 and err() == text
        with pytest.raises(nat.TdsaError):
            p.process(x[:10])
        assert p.read(0).n_total == n
        p.reset()
        p.process(x[:100])
        assert p.read(0).n_total == 100 and not p.read(0).flushed


def test_reset_set_reference_and_reconfiguration():
    L, n = 64, T + 500
    x, wants = stack(L, n, cc.C64, 2, seed=60)
    with Correlator(reference(L), 2, 64) as p:
        p.configure(THR, 10)
        p.process(x)
        p.process(x)                                       # the state accumulates ...
        twice = [Want(L, np.concatenate([s, s]), cc.C64) for s in x]
        same(p, twice, 2 * n, False, "twice")
        p.reset()                                          # ... until a reset
        assert not p.read_summaries()["n_total"].any() and len(p.read(1)) == 0
        for thr, W in ((THR, 1), (0.9, T + 1), (0.3, 64)):
            p.process(x[:, :100])                          # what a reconfiguration must forget
            p.configure(thr, W)
            assert (p.threshold, p.min_distance) == (float(np.float32(thr)), W)
            p.process(x)
            same(p, wants, n, False, (thr, W), thr)
        p.configure(THR)                                   # min_distance defaults to L
        assert p.min_distance == L
        # another reference, of another length: the streams start again, threshold and min_distance stay
        L2 = 17
        x2, wants2 = stack(L2, n, cc.C64, 2, seed=61)
        p.process(x[:, :300])
        p.set_reference(reference(L2))
        assert p.L == L2 and p.min_distance == L
        p.process(x2)
        same(p, wants2, n, False, "new reference")


def test_trace_ranges_that_are_gone_or_not_yet_there_return_minus_1():
    L, K = 16, 1000
    x = signal(L, 3000, cc.C64, 70)
    with Correlator(reference(L), 1, 16, trace=K) as p:
        p.configure(THR)
        m0 = np.zeros(8, dtype=np.float32)
        call = lambda first, count: nat.lib.tdsa_corr_read_trace(p._h, 0, first, count, m0.ctypes.data_as(C.c_void_p), None)
        assert call(0, 0) == 0 and call(0, 1) == -1        # nothing yet
        p.process(x[:L - 1])
        assert call(0, 1) == -1                            # no complete window
        p.process(x[L - 1:500])
        nw = 500 - L + 1
        m, c = p.read_trace(0, 0, nw)
        assert call(nw - 1, 1) == 0 and call(nw, 1) == -1 and call(nw - 1, 2) == -1 and call(nw, 0) == 0
        p.process(x[500:])
        nw = 3000 - L + 1
        assert call(nw - K, 8) == 0 and call(nw - K - 1, 1) == -1 and call(0, 1) == -1 and call(nw - 8, 8) == 0 and call(nw - 7, 8) == -1
        assert "the trace holds" in nat.lib.tdsa_last_error_string().decode()
        assert nat.lib.tdsa_corr_read_trace(p._h, 1, nw - 8, 8, m0.ctypes.data_as(C.c_void_p), None) == -1
        with pytest.raises(nat.TdsaError):
            p.read_trace(0, 0, 10)
        late_m, late_c = p.read_trace(0, nw - K, K)
        w = cc.Windows(x.astype(np.complex128), reference(L))
        assert (np.abs(late_m - w.m[nw - K:]) <= w.b_m[nw - K:]).all() and (np.abs(m - w.m[:m.size]) <= w.b_m[:m.size]).all()
    with Correlator(reference(L), 256, 1, trace=1 << 30) as p:      # the trace of all streams stays within 256 MiB
        assert p.trace == (1 << 28) // (24 * 256)


def test_nan_and_inf_samples_squares_that_overflow_and_streams_of_zeros():
    L = 16
    x = signal(L, T + 400, cc.C64, 80, (30, 700, T + 100)).copy()
    x[300] = complex(np.nan, 0)
    x[T - 1] = complex(0, np.inf)                           # windows on either side of the tile seam
    x[1200] = complex(-np.inf, np.nan)
    x[1500] = complex(2e19, 0)                             # the square overflows float32: e = +inf
    x[1800:1800 + 2 * L] = 0                                # L + 1 windows of nothing: e = 0
    wt = Want(L, x, cc.C64)
    assert wt.w.bad.sum() == 4 * L + L + 1
    with Correlator(reference(L), 1, 64, trace=wt.w.n) as p:
        p.configure(THR, L)
        p.process(x)
        p.flush()
        same(p, [wt], x.size, True, "non-finite, host")
        m, c = p.read_trace(0, 0, wt.w.n)
        assert (m[wt.w.bad] == 0).all() and np.isfinite(m).all() and p.read(0).index.tolist() == [30, 700, T + 100]
        p.reset()
        feed_device(p, x[None, :], cc.C64, 0, 1)
        p.flush()
        same(p, [wt], x.size, True, "non-finite, device")
        p.reset()
        p.process(np.zeros(3 * L, dtype=np.int8))          # (0, 0) samples: every window bad
        p.flush()
        t = p.read(0)
        assert len(t) == 0 and t.n_bad == t.n_windows == 3 * L // 2 - L + 1


def test_behind_a_channelizer_and_a_down_converter_on_an_engine_stream():
    """The reference as the streams carry it: cut from the filters' own output of a first pass, then searched for in a
    second pass that nobody waits for between the filter and the search."""
    rng = np.random.default_rng(4)
    n_in, M, D, L = 1 << 16, 8, 4, 64
    burst = rng.integers(-100, 100, 2 * 8 * L)
    iq = rng.integers(-6, 6, 2 * n_in)
    starts = (5000, 21000, 40000)
    for s in starts:
        iq[2 * s:2 * s + burst.size] += burst
    iq = iq.astype(np.int8)
    with SpectrumEngine(64) as eng, Channelizer(M, 1e6) as ch, DownConverter(D, 1e6, 1e5) as ddc, DeviceBuffer.of(iq) as d_in:
        n_ch, n_dd = ch.outputs_completed_by(n_in), n_in // D + 1
        stride = n_ch + 3
        with DeviceBuffer(8 * M * stride) as d_ch, DeviceBuffer(8 * n_dd) as d_dd:
            got_ch = ch.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_ch.ptr, stride)
            got_dd = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_dd.ptr)
            eng.synchronize()
            y_ch = d_ch.get((M, stride), np.complex64)[:, :got_ch]
            y_dd = d_dd.get((got_dd,), np.complex64)
            # the first burst as each filter delivers it: L outputs from a little behind its start
            r_ch = y_ch[1, starts[0] // M + 4:starts[0] // M + 4 + L].copy()
            r_dd = y_dd[starts[0] // D + 8:starts[0] // D + 8 + L].copy()
            with Correlator(r_ch, M, 64) as pm, Correlator(r_dd, 1, 64) as p1:
                pm.configure(0.5, L)
                p1.configure(0.5, L)
                d_ch.put(np.full(M * stride, np.nan, dtype=np.complex64))
                ch.reset()
                ddc.reset()
                got_ch = ch.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_ch.ptr, stride)
                pm.process_device(eng, d_ch.ptr, got_ch, stride)          # no wait in between: the stream orders them
                got_dd = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n_in, d_dd.ptr)
                p1.process_device(eng, d_dd.ptr, got_dd)
                pm.flush()
                p1.flush()
                t_ch, t_dd = pm.read(1), p1.read(0)
                eng.synchronize()
            for t, y, r, first, tag in ((t_ch, y_ch[1], r_ch, starts[0] // M + 4, "channelizer"), (t_dd, y_dd, r_dd, starts[0] // D + 8, "ddc")):
                w = cc.Windows(y.astype(np.complex128), r)
                d = cc.decide(w.m, 2.0 * w.b_m, 0.5, L)
                assert not (d == cc.OPEN).any(), tag
                assert np.array_equal(t.index, np.flatnonzero(d == cc.YES)) and first in t.index and len(t) >= 1, (tag, t.index)
                assert t.metric[t.index.tolist().index(first)] > 0.999
                within(t.records, w, tag)


def test_error_returns_with_a_live_handle():
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()
    buf = (C.c_byte * 4096)()
    sums = (nat.CorrSummary * 4)()
    rec = (nat.CorrRecord * 16)()
    r = reference(16)
    ref = r.ctypes.data_as(C.c_void_p)
    with Correlator(r, 3, 4, trace=50, max_host_samples=300) as p, DeviceBuffer(4096) as d:
        h = p._h
        for bad in ((0.0, 4), (-1.0, 4), (1.5, 4), (float("nan"), 4), (0.5, 0), (0.5, 65537)):
            assert lib.tdsa_corr_configure(h, *bad) == -1, bad
        for n in (1, 1025):
            assert lib.tdsa_corr_set_reference(h, ref, n) == -1 and "ref_len" in err()
        assert lib.tdsa_corr_set_reference(h, None, 16) == -1 and err() == "null reference"
        assert lib.tdsa_corr_process(h, 5, buf, 4, 4) == -1 and "in_format" in err()
        assert lib.tdsa_corr_process(h, cc.I8, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_corr_process(h, cc.I8, buf, 4, 3) == -1 and "in_stride" in err()
        assert lib.tdsa_corr_process(h, cc.I8, buf, 101, 101) == -1 and "max_host_samples" in err()
        assert lib.tdsa_corr_process_dev(h, None, cc.C64, C.c_void_p(d.ptr + 4), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_corr_process_dev(h, None, cc.I8, C.c_void_p(d.ptr + 1), 4, 4) == -1 and "aligned" in err()
        assert lib.tdsa_corr_process_dev(h, None, cc.C64, None, 4, 4) == -1 and "null samples" in err()
        assert lib.tdsa_corr_process_dev(h, None, cc.C64, C.c_void_p(d.ptr), 4, 3) == -1 and "in_stride" in err()
        for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
            assert lib.tdsa_corr_read(h, first, count, rec, sums) == -1 and "streams" in err()
        assert lib.tdsa_corr_read(h, 0, 3, rec, None) == -1 and "null summaries" in err()
        for stream in (-1, 3):
            assert lib.tdsa_corr_read_trace(h, stream, 0, 0, buf, buf) == -1 and "stream" in err()
        for bad in ((2, 15, 0), (MAX_TILES + 1, 15, 0), (16, 16, 0), (16, -1, 0), (16, 15, 8), (16, 15, -1)):
            assert lib.tdsa_corr_debug_limits(h, *bad) == -1, bad
        assert lib.tdsa_corr_timer_end(h, None) == -1
        assert lib.tdsa_corr_process(h, cc.I8, None, 0, 0) == 0 and lib.tdsa_corr_process_dev(h, None, cc.I8, None, 0, 0) == 0
        assert lib.tdsa_corr_read(h, 0, 3, rec, sums) == 0 and [s.n_total for s in sums[:3]] == [0, 0, 0]
        assert lib.tdsa_corr_read(h, 1, 2, None, sums) == 0     # the records are optional
        p.timer_begin()
        p.process_device(None, d.ptr, 16, 16, cc.I8)
        assert p.timer_end() >= 0.0
    with Correlator(barker(2), 1, 2, max_host_samples=8) as p:                          # C = 1: the stride is ignored
        p.configure(0.99, 1)
        x = np.tile(np.array([60, 0, -60, 0, 5, 9, -7, 3, 2, -8], dtype=np.int8), 6)   # + - then three samples of anything
        assert lib.tdsa_corr_process(p._h, cc.I8, x.ctypes.data_as(C.c_void_p), 5, 0) == 0 and p.read(0).n_total == 5
        p.process(x[10:])                                                              # above the staging: in pieces
        p.flush()
        got = p.read(0)
        assert got.n_total == 30 and got.n_matches == 6 and got.n_lost == 4 and got.index.tolist() == [0, 5]
