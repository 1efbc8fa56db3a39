"""The eye diagrams on the device (tdsa_eye_*) against tests/eye_contract.py: bit for bit where
the contract is exact - integer positions, the rows, the counts, the centre column against the analysers that produced
the clock -, within the two producers' derived bounds in every other column, and the same integers for any split of the
segments over calls and entry points."""
import ctypes as C

import numpy as np
import pytest

import eye_contract as ec
import fsk_contract as fc
import symsync_contract as sc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, _native as nat
from topdogspectrumanalyser_amd import eye as ey
from topdogspectrumanalyser_amd import fsk as fk
from topdogspectrumanalyser_amd import symbols as sy

pytestmark = pytest.mark.gpu

ONE = ec.ONE
SPS_ALL = (4, 4.37, 5, 8 - 2.0 ** -20, 8, 16, 33.3, 64)
BOXCARS = (1, 2, 3, 32, 64)
TILE = 1024                                  # samples of the series a work item holds (tdsa_eye.hpp: kEyeTile)
KIND = {"iq": ec.IQ, "fm": ec.FM, "real": ec.REAL}
SMALL = dict(max_host_samples=1 << 17, max_segments=512)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def seg_len_for(step, K, kind, B):
    """The shortest segment that gives K symbols."""
    n = 4 + -(-(K + 1) * step // ONE) + (B if kind == ec.FM else B - 1 if kind == ec.REAL else 0)
    assert ec.symbols_per_segment(step, n, kind, B) == K and ec.symbols_per_segment(step, n - 1, kind, B) == K - 1
    return n


def symbols_per_item(step):
    return ((TILE - 5) << 32) // step


def _same_image(img, tr, K, skipped=0, what=None):
    """The device's image against the contract's binning of (the device's) traces [n_seg][K - 2][P], skipped segments
    left out of `tr`; the invariant."""
    P = img.points
    counts, totals = ec.bin_traces(tr, np.float32(img.lo), np.float32(img.hi), img.rows)
    assert np.array_equal(img.counts, counts), what
    got = np.stack([img.n_points, img.n_under, img.n_over, img.n_nan], axis=1)
    assert np.array_equal(got, totals), (what, got, totals)
    assert img.skipped == skipped and ec.invariant(img.counts, got, img.segments, img.skipped, K, P), what


def _image_bits(a, b):
    return (_bits(a.counts, b.counts) and all(_bits(getattr(a, f), getattr(b, f)) for f in ("n_points", "n_under", "n_over", "n_nan"))
            and (a.segments, a.skipped) == (b.segments, b.skipped))


def _run(e, x, L, hop, ck, traces=True):
    """The traces of one call, [n_seg][K - 2][P] with the sentinel where nothing is written: through the host entry point
    where its staging takes the block, else through the device entry point."""
    K, n_seg = e.symbols_per_segment(L), len(ck)
    if x.size <= e.max_host_samples:
        return e.process(x, L, ck, hop, traces=traces)
    shape = (n_seg, K - 2, e.points)
    unit = 8 if e.kind == nat.EYE_IQ else 4
    with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(unit * int(np.prod(shape))) as d_t:
        d_x.put(x)
        d_t.put(np.full(shape, ey.SENTINEL, dtype=e._trace_dtype))
        e.process_device(None, d_x.ptr, L, hop, n_seg, ck, d_t.ptr if traces else None)
        e.read()
        return d_t.get(shape, e._trace_dtype) if traces else None


# ---- 1: exact traces and counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("real", "iq"))
@pytest.mark.parametrize("sps, P", [(4, 4), (8, 8), (16, 8), (64, 64), (64, 4)])
def test_integer_clocks_pick_input_samples_bit_for_bit(sps, P, kind):
    """Integer sps with P | sps and an integer delta_fx: every mu is 0 and a point is an input sample (REAL with B = 1; IQ
    with a zero carrier), so traces and counts are numpy indexing plus the contract's binning.  The launcher cuts a
    segment into work items of up to `spi` symbols - the fewer the call brings, the shorter - so the symbol counts go one
    past one and two full items, and one call of 520 segments is long enough to fill them."""
    step, H, lo, hi = sps * ONE, 37, -0.8, 0.9
    rng = np.random.default_rng(sps * 100 + P)
    spi = symbols_per_item(step)
    Ks = {3} | {2 - (-n // P) for n in (255, 256, 257)} | {k for k in (spi + 3, 2 * spi + 3) if k <= 4096} | ({4096} if sps == 4 else set())
    n_base = 3 * seg_len_for(step, max(Ks - {4096}), KIND[kind], 1) + 17000      # three of the longest, or one of K = 4096
    base = rng.uniform(-1.0, 1.0, n_base).astype(np.float32)
    if kind == "iq":
        base = (base + 1j * rng.uniform(-1.0, 1.0, n_base)).astype(np.complex64)
    n_run = 0
    with ey.EyeDiagram(sps, kind, points=P, rows=H, v_range=(lo, hi), boxcar=1, max_host_samples=1 << 15, max_segments=520) as e:
        for K in sorted(Ks):
            L = seg_len_for(step, K, KIND[kind], 1)
            lays = [(1, L), (2, 5)] if K == 4096 else [(1, L), (2, L + 3), (3, L), (3, max(1, L - 7))] + ([(257, 5)] if L <= 600 else [])
            if K == 2 * spi + 3:                    # a call long enough for the launcher to fill the items' tiles
                lays.append((520, 5))
            for n_seg, hop in lays:
                for delta in sorted({1, sps}):
                    x = base[:(n_seg - 1) * hop + L]
                    ck = e.clocks(delta=float(delta), n_seg=n_seg)
                    if n_seg >= 3:
                        ck["delta_fx"][n_seg // 2] = 0                      # a skip clock in the middle
                    e.reset()
                    tr = _run(e, x, L, hop, ck)
                    n_run += 1
                    idx = delta + np.arange(1, K - 1)[:, None] * sps + (np.arange(P)[None, :] - P // 2) * (sps // P)
                    live = [g for g in range(n_seg) if ck["delta_fx"][g]]
                    want = np.stack([x[g * hop:g * hop + L][idx] for g in live])
                    what = (K, L, n_seg, hop, delta)
                    assert _bits(tr[live], want), what
                    for g in set(range(n_seg)) - set(live):
                        assert np.all(tr[g] == ey.SENTINEL), what
                    img = e.read()
                    assert img.segments == n_seg
                    _same_image(img, want, K, n_seg - len(live), what)
    print(f"sps {sps} P {P} {kind}: {n_run} calls")


# ---- 2: row edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo, hi", [(-1.0, 1.0), (0.0, 0.37), (-0.3, 1.1), (-3e38, 3e38)])
@pytest.mark.parametrize("H", (8, 17, 128, 255, 256))
def test_row_edges(H, lo, hi):
    """REAL at P = sps = 4, B = 1, delta = 1: the points of a segment are its samples 3, 4, ... in order, column j mod 4.
    Values on every row edge and on both float32 neighbours, at and around lo and hi, zeros, infinities, NaN, a denormal,
    the largest magnitudes: counts and all three overflow totals are the contract's."""
    lo, hi = np.float32(lo), np.float32(hi)
    scale = float(ec.scale_of(H, lo, hi))
    edges = np.array([float(lo) + r / scale for r in range(H + 1)]).astype(np.float32)
    pad = [lo, lo, lo]
    with np.errstate(over="ignore"):
        vals = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                               np.array([lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf)),
                                         np.nextafter(hi, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)),
                                         0.0, -0.0, 1e-45, -1e-45, 3.4e38, -3.4e38]
                                        + pad + [np.inf] + pad + [-np.inf] + pad + [np.nan] + pad, dtype=np.float32)])
    vals = np.concatenate([vals, np.full(-vals.size % 4, lo, dtype=np.float32)]).astype(np.float32)
    K = vals.size // 4 + 2
    L = seg_len_for(4 * ONE, K, ec.REAL, 1)
    x = np.full(L, lo, dtype=np.float32)
    x[3:3 + vals.size] = vals
    # mu = 0: the coefficients are (0, 1, 0, 0), and 0 x (an infinity or a NaN) under a neighbouring tap is a NaN
    idx = 3 + np.arange(vals.size)
    want = np.where(np.isfinite(x[idx - 1]) & np.isfinite(x[idx + 1]) & np.isfinite(x[idx + 2]), vals, np.float32(np.nan))
    assert np.count_nonzero(np.isnan(want)) == 10 and np.isposinf(want).any() and np.isneginf(want).any()
    with ey.EyeDiagram(4, "real", points=4, rows=H, v_range=(lo, hi), boxcar=1, **SMALL) as e:
        tr = e.process(x, L, e.clocks(delta=1.0), traces=True)
        assert np.array_equal(tr.reshape(-1), want, equal_nan=True)
        img = e.read()
    _same_image(img, want.reshape(1, -1, 4), K, 0, (H, lo, hi))
    rows = ec.rows_of(want, lo, hi, H)
    assert img.n_nan[0] == 10 and img.n_under[0] == np.count_nonzero(rows == ec.UNDER) >= 3
    assert img.n_over[0] == np.count_nonzero(rows == ec.OVER) >= 4            # hi, its upper neighbour, +inf, 3.4e38


# ---- 3, 4, 5: the centre column, the other columns, the counts -----------------------------------------------------------
def _real_columns(e, x, L, ck, tr, kind, B, what):
    """Every column of FM or REAL traces within fsk_contract's bounds of the float64 contract at the device's clocks."""
    step, P, K = e.step, e.points, e.symbols_per_segment(L)
    worst = 0.0
    for g in range(len(ck)):
        seg = x[g * L:g * L + L]
        d = fc.discriminate(seg.astype(np.complex128)) if kind == ec.FM else seg.astype(np.float64)
        y, mag, sumc = ec.interpolate(fc.boxcar(d, B), int(ck["delta_fx"][g]), step, K, P, True)
        bound = ec.real_bound(mag, sumc, float(np.abs(d).max()), kind, B)
        err = np.abs(tr[g].astype(np.float64) - y) / np.maximum(bound, 1e-300)
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (what, g, float(err.max()))
    return worst


@pytest.mark.parametrize("sps", SPS_ALL)
def test_fm_and_real_eyes_behind_the_fsk_analyser(sps):
    """FM behind FskAnalyzer(input="iq") and REAL behind input="freq" on the analyser's own records' clocks: the centre
    column is its levels [1 .. K - 2] bit for bit, every column lies within the derived bounds, and the image is the
    contract's binning of the device's traces."""
    step = fc.step_of(sps)
    worst = 0.0
    for nb, B in enumerate(BOXCARS):
        P = ey.POINTS[(nb + int(sps)) % 5]
        L = int(40 * sps) + B + 9
        x, _, _ = fc.make_fsk(2, sps, 3 * L, 0.5, 0.5, seed=nb + 1)
        x = x.astype(np.complex64)
        f = fc.discriminate(x.astype(np.complex128)).astype(np.float32)
        for kind, inp, data in (("fm", "iq", x), ("real", "freq", f[:3 * (L - 1)])):
            Ls = L if kind == "fm" else L - 1
            with fk.FskAnalyzer(sps, 2, input=inp, boxcar=B, max_host_samples=1 << 15) as a, \
                    ey.EyeDiagram(sps, kind, points=P, rows=64, v_range=(-0.3, 0.35), boxcar=B, **SMALL) as e:
                r = a.process(data, Ls)
                K = e.symbols_per_segment(Ls)
                assert K == a.symbols_per_segment(Ls) and not (r.flags & nat.FSK_NONFINITE).any()
                ck = e.clocks(r)
                assert np.array_equal(ck["delta_fx"], r.records["delta_fx"])
                tr = e.process(data, Ls, ck, traces=True)
                what = (sps, B, P, kind)
                assert _bits(tr[:, :, P // 2], r.levels[:, 1:K - 1]), what
                worst = max(worst, _real_columns(e, data, Ls, ck, tr, KIND[kind], B, what))
                _same_image(e.read(), tr, K, 0, what)
    print(f"sps {sps}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("sps", SPS_ALL)
def test_iq_eyes_behind_the_symbol_recovery(sps):
    """IQ behind SymbolSync for qpsk and 16qam with a carrier offset either way and with carrier=False: the centre column
    is its symbols [1 .. K - 2] bit for bit (by value where the recovery does not rotate at all), every column within
    symsync_contract's bounds, the image the contract's binning of the device's traces."""
    step = sc.step_of(sps)
    L = int(48 * sps) + 9
    worst, negative = 0.0, False
    for n_case, (mod, w, carrier) in enumerate((("qpsk", 0.01, True), ("16qam", -0.013, True), ("qpsk", -0.004, True), ("qpsk", 0.0, False))):
        P = ey.POINTS[(n_case + int(sps)) % 5]
        x, _, _ = sc.make_signal(mod, sps, 3 * L, seed=n_case + 2, w=w / sps * 4)
        x = x.astype(np.complex64)
        with sy.SymbolSync(sps, mod, carrier=carrier, max_host_samples=1 << 15) as s, \
                ey.EyeDiagram(sps, "iq", points=P, rows=48, v_range=(-1.6, 1.7), **SMALL) as e:
            r = s.process(x, L)
            K = e.symbols_per_segment(L)
            assert K == s.symbols_per_segment(L) and not (r.flags & nat.SYMSYNC_NONFINITE).any()
            ck = e.clocks(r)
            negative |= bool(np.any(ck["step_f"].astype(np.int32) < 0))
            tr = e.process(x, L, ck, traces=True)
            what = (sps, mod, w, carrier, P)
            if carrier:
                assert _bits(tr[:, :, P // 2], r.symbols[:, 1:K - 1]), what
            else:                                   # step_f = theta_fx = 0: the identity, up to the sign of a zero
                assert not ck["step_f"].any() and not ck["theta_fx"].any()
                assert np.array_equal(tr[:, :, P // 2], r.symbols[:, 1:K - 1]), what
            for g in range(3):
                seg = x[g * L:g * L + L].astype(np.complex128)
                y, mag, _ = ec.interpolate(seg, int(ck["delta_fx"][g]), step, K, P, True)
                v = ec.derotate(y, int(ck["theta_fx"][g]), int(ck["step_f"][g]))
                err = np.abs(tr[g].astype(np.complex128) - v) / np.maximum(ec.iq_bound(y, mag), 1e-300)
                worst = max(worst, float(err.max()))
                assert err.max() <= 1.0, (what, g, float(err.max()))
            _same_image(e.read(), tr, K, 0, what)
    assert negative                                  # a record whose step_f is negative as int32 was among them
    print(f"sps {sps}: worst error / bound {worst:.3f}")


# ---- 6: hot bins -------------------------------------------------------------------------------------------------------------
def test_a_constant_stream_fills_one_bin_per_column_past_2_to_the_20():
    """K = 4096 at P = sps = 4, 257 segments: 4094 x 257 > 2^20 into one bin per column - 16-bit packing and lost LDS adds
    would show."""
    L = seg_len_for(4 * ONE, 4096, ec.REAL, 1)
    x = np.full(L + 256, 0.3, dtype=np.float32)                 # row 2.4 of 8: no rounding of the cubic moves it
    with ey.EyeDiagram(4, "real", points=4, rows=8, v_range=(0.0, 1.0), boxcar=1, **SMALL) as e:
        e.process(x, L, e.clocks(delta=2.5, n_seg=257), hop=1)
        img = e.read()
    want = np.zeros((1, 8, 4), dtype=np.uint64)
    want[0, 2, :] = 4094 * 257
    assert np.array_equal(img.counts, want) and img.n_points[0] == 4 * 4094 * 257 and img.segments == 257


def test_a_bin_carries_past_2_to_the_32():
    """The same stream, one sample apart, ceil(2^32 / 4094) + 1 segments in one call: every column's bin passes 2^32."""
    L = seg_len_for(4 * ONE, 4096, ec.REAL, 1)
    n_seg = -(-(1 << 32) // 4094) + 1
    x = np.full(L + n_seg - 1, 0.3, dtype=np.float32)
    with ey.EyeDiagram(4, "real", points=4, rows=8, v_range=(0.0, 1.0), boxcar=1, max_host_samples=1 << 12, max_segments=n_seg) as e, \
            DeviceBuffer(x.nbytes) as d_x:
        d_x.put(x)
        e.timer_begin()
        e.process_device(None, d_x.ptr, L, 1, n_seg, e.clocks(delta=1.0, n_seg=n_seg))
        ms = e.timer_end()
        img = e.read()
    print(f"{n_seg} segments of {L}: {ms:.1f} ms")
    want = np.zeros((1, 8, 4), dtype=np.uint64)
    want[0, 2, :] = 4094 * n_seg
    assert 4094 * n_seg > 1 << 32 and np.array_equal(img.counts, want)
    assert img.n_points[0] == 4 * 4094 * n_seg and (img.segments, img.skipped) == (n_seg, 0)


# ---- 7: split invariance -------------------------------------------------------------------------------------------------------
def test_the_image_does_not_depend_on_how_the_segments_are_split():
    """One call; the same segments over five calls of uneven sizes; the host entry point; the device entry point: the same
    bits of counts and totals.  reset() and set_range() zero everything."""
    sps, L, hop, n_seg, P = 4.37, 300, 211, 41, 16
    x, _, _ = sc.make_signal("qpsk", sps, (n_seg - 1) * hop + L, seed=7)
    x = x.astype(np.complex64)
    with sy.SymbolSync(sps, "qpsk", max_host_samples=1 << 15) as s, ey.EyeDiagram(sps, "iq", points=P, rows=33, **SMALL) as e, \
            DeviceBuffer(x.nbytes) as d_x:
        ck = e.clocks(s.process(x, L, hop))
        ck["delta_fx"][[3, 17]] = 0
        e.process(x, L, ck, hop)
        one = e.read()
        assert (one.segments, one.skipped) == (n_seg, 2) and one.counts.sum() > 0
        e.reset()
        zero = e.read()
        assert not zero.counts.any() and (zero.segments, zero.skipped) == (0, 0) and not zero.n_points.any()
        at = 0
        for n in (1, 17, 2, 20, 1):
            e.process(x[at * hop:], L, ck[at:at + n], hop)
            at += n
        assert at == n_seg and _image_bits(e.read(), one)
        d_x.put(x)
        e.reset()
        e.process_device(None, d_x.ptr, L, hop, 20, ck[:20])
        e.process_device(None, d_x.ptr + 8 * 20 * hop, L, hop, 1, ck[20:21])       # back to back: the clocks' staging
        e.process_device(None, d_x.ptr + 8 * 21 * hop, L, hop, 20, ck[21:])
        assert _image_bits(e.read(), one)
        e.set_range(-1.5, 1.5)
        assert not e.read().counts.any() and e.read().segments == 0
        e.process(x, L, ck, hop)
        assert _image_bits(e.read(), one)                                           # the same range again
        e.set_range(-1.0, 2.0)
        e.process(x, L, ck, hop)
        other = e.read()
        assert not _bits(other.counts, one.counts) and np.array_equal(other.n_points, one.n_points)


def test_behind_the_down_converter_and_the_symbol_recovery_on_an_engine_stream():
    """capture -> DownConverter(D = 2) -> SymbolSync -> EyeDiagram, all on the engine's stream with no wait but the
    recovery's own for its records, against the same chain staged through the host."""
    from topdogspectrumanalyser_amd import DownConverter, SpectrumEngine, design_decimator
    sps, L, D, P = 8, 1023, 2, 32
    x, _, _ = sc.make_signal("qpsk", sps * D, D * (3 * L + 64), seed=9)
    x = x.astype(np.complex64)
    taps = design_decimator(D)
    with SpectrumEngine(64) as eng, DownConverter(D, 1.0, taps=taps) as ddc, DownConverter(D, 1.0, taps=taps) as ddc_h, \
            sy.SymbolSync(sps, "qpsk") as s, ey.EyeDiagram(sps, "iq", points=P, rows=64, **SMALL) as e, \
            ey.EyeDiagram(sps, "iq", points=P, rows=64, **SMALL) as e_h:
        y = ddc_h.process(x)
        K = s.symbols_per_segment(L)
        n_seg = (y.size - L) // L + 1
        with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * (y.size + 8)) as d_y, DeviceBuffer(8 * n_seg * K) as d_s, \
                DeviceBuffer(8 * n_seg * (K - 2) * P) as d_t:
            d_x.put(x)
            ny = ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            r = s.process_device(eng, d_y.ptr, L, L, n_seg, d_s.ptr, K)
            e.process_device(eng, d_y.ptr, L, L, n_seg, e.clocks(r), d_t.ptr)
            img = e.read()
            tr = d_t.get((n_seg, K - 2, P), np.complex64)
            sym = d_s.get((n_seg, K), np.complex64)
        assert ny == y.size and n_seg == 3
        r_h = s.process(y, L)
        assert r.records.tobytes() == r_h.records.tobytes()
        tr_h = e_h.process(y, L, e_h.clocks(r_h), traces=True)
        assert _bits(tr, tr_h) and _image_bits(img, e_h.read()) and _bits(tr[:, :, P // 2], sym[:, 1:K - 1])


# ---- 8: non-finite input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("real", "iq"))
def test_a_nan_and_an_infinity_touch_only_the_points_whose_taps_read_them(kind):
    sps, L, P, H = 4.37, 200, 8, 32
    step = sc.step_of(sps)
    rng = np.random.default_rng(8)
    clean = rng.uniform(-0.9, 0.9, 3 * L).astype(np.float32)
    if kind == "iq":
        clean = (clean + 1j * rng.uniform(-0.9, 0.9, 3 * L)).astype(np.complex64)
    bad = clean.copy()
    at = (L + 57, L + 131)
    bad[at[0]] = np.nan
    bad[at[1]] = np.inf if kind == "real" else complex(0.1, -np.inf)
    with ey.EyeDiagram(sps, kind, points=P, rows=H, v_range=(-1.0, 1.0), boxcar=1, **SMALL) as e:
        K = e.symbols_per_segment(L)
        ck = e.clocks(delta=2.25, n_seg=3)
        ck["step_f"], ck["theta_fx"] = 12345678, 999                 # read for iq only
        tr_clean = e.process(clean, L, ck, traces=True)
        e.reset()
        tr = e.process(bad, L, ck, traces=True)
        img = e.read()
    i, _ = ec.positions(int(ck["delta_fx"][1]), step, K, P)
    hit = np.zeros(i.shape, dtype=bool)
    for a in at:
        hit |= (i - 1 <= a - L) & (a - L <= i + 2)
    assert 8 <= np.count_nonzero(hit) < hit.size // 4
    for g in (0, 2):
        assert _bits(tr[g], tr_clean[g])
    assert _bits(tr[1][~hit], tr_clean[1][~hit]) and np.all(np.isfinite(tr[1][~hit]))
    parts = (tr[1].real, tr[1].imag) if kind == "iq" else (tr[1],)
    assert np.all(~np.isfinite(parts[0][hit]) | ~np.isfinite(parts[-1][hit]))
    _same_image(img, tr, K, 0, kind)
    assert sum(int(img.n_nan[q]) + int(img.n_over[q]) + int(img.n_under[q]) for q in range(img.counts.shape[0])) >= np.count_nonzero(hit)
    assert img.n_nan.sum() >= 4


# ---- 9: the -1s that need a live handle ---------------------------------------------------------------------------------------------
def test_error_returns_with_a_live_handle():
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()                                   # noqa: E731
    Pt = lambda addr: C.c_void_p(int(addr))                                              # noqa: E731
    x = np.zeros(8192, dtype=np.complex64)
    ck = np.zeros(8, dtype=ey.CLOCK)
    ck["delta_fx"] = 2 * ONE
    tr = np.zeros(1 << 16, dtype=np.complex64)
    px, pc, pt = x.ctypes.data, ck.ctypes.data, tr.ctypes.data
    raw = C.c_void_p()
    assert lib.tdsa_eye_create(0, 4096, 4, C.byref(raw)) == 0
    try:
        assert lib.tdsa_eye_process(raw, Pt(px), 100, 100, 100, 1, Pt(pc), None) == -3 and err() == "not configured: call tdsa_eye_configure first"
        assert lib.tdsa_eye_process_dev(raw, None, Pt(px), 100, 100, 1, Pt(pc), None) == -3 and "not configured" in err()
        assert lib.tdsa_eye_process(raw, None, 100, 100, 100, 1, None, None) == -3      # asked before the arguments
        assert lib.tdsa_eye_read(raw, Pt(pt), Pt(pt)) == -3 and "not configured" in err()
    finally:
        assert lib.tdsa_eye_destroy(raw) == 0
    with ey.EyeDiagram(4, "iq", points=8, rows=16, max_host_samples=4096, max_segments=4) as a, \
            ey.EyeDiagram(4, "real", points=8, rows=16, boxcar=2, max_host_samples=4096, max_segments=4) as f, \
            DeviceBuffer(8 * 4096) as d_x, DeviceBuffer(8 * 4096) as d_t:
        host = lambda h, **kw: lib.tdsa_eye_process(h, *[kw.get(k, v) for k, v in (                        # noqa: E731
            ("inp", Pt(px)), ("n", 1000), ("seg", 100), ("hop", 100), ("n_seg", 2), ("ck", Pt(pc)), ("tr", Pt(pt)))])
        dev = lambda h, **kw: lib.tdsa_eye_process_dev(h, None, *[kw.get(k, v) for k, v in (               # noqa: E731
            ("inp", Pt(d_x.ptr)), ("seg", 100), ("hop", 100), ("n_seg", 2), ("ck", Pt(pc)), ("tr", Pt(d_t.ptr)))])
        for call in (host, dev):
            for h in (a._h, f._h):
                assert call(h) == 0, err()
                assert call(h, tr=None) == 0, err()                                        # the traces are optional
                assert call(h, inp=None) == -1 and err() == "null samples"
                assert call(h, ck=None) == -1 and err() == "null clocks"
                assert call(h, ck=Pt(pc + 4)) == -1 and err() == "clocks must be aligned to 8 bytes"
                assert call(h, n_seg=0) == -1 and err() == "n_seg=0: 1 .. 4 (the handle's max_segments)"
                assert call(h, n_seg=5) == -1 and err() == "n_seg=5: 1 .. 4 (the handle's max_segments)"
                assert call(h, hop=0) == -1 and err() == "hop=0: at least one sample"
            # K outside 3 .. 4096: iq has n = seg_len, real n = seg_len - 1 at B = 2
            for h, two, three, most in ((a._h, 19, 20, 16392), (f._h, 20, 21, 16393)):
                assert call(h, seg=two, hop=two, n_seg=1) == -1 and err() == f"seg_len={two} gives 2 symbols per segment: 3 .. 4096"
                assert call(h, seg=3, hop=3, n_seg=1) == -1 and "gives -1 symbols" in err()
                assert call(h, seg=most + 4, hop=1, n_seg=1) == -1 and "gives 4097 symbols" in err()
                if call is host:
                    assert call(h, seg=three, hop=three, n_seg=1) == 0, err()
            # a clock outside its range names its segment; 0 is the skip
            for d, ok in ((ONE - 1, False), (5 * ONE, False), (5 * ONE - 1, True), (0, True), (ONE, True)):
                ck["delta_fx"][1] = d
                assert (call(a._h) == 0) == ok, (d, err())
                if not ok:
                    assert err() == f"clock of segment 1: delta_fx={d}: 0 (skip) or 2^32 <= delta_fx < step + 2^32"
            ck["delta_fx"] = 2 * ONE
        # the device entry point alone: the alignment of what is read and written in place
        assert dev(a._h, inp=Pt(d_x.ptr + 4)) == -1 and err() == "input pointer must be aligned to one complex64 sample (8 bytes)"
        assert dev(f._h, inp=Pt(d_x.ptr + 2)) == -1 and err() == "input pointer must be aligned to one float32 (4 bytes)"
        assert dev(f._h, inp=Pt(d_x.ptr + 4)) == 0, err()
        assert dev(a._h, tr=Pt(d_t.ptr + 4)) == -1 and err() == "traces pointer must be aligned to one complex64 point (8 bytes)"
        assert dev(f._h, tr=Pt(d_t.ptr + 2)) == -1 and err() == "traces pointer must be aligned to one float32 (4 bytes)"
        # the host entry point alone: the block and the staging
        for h in (a._h, f._h):
            assert host(h, n=199) == -1 and err() == "2 segments of 100 samples every 100 need 200 samples, the block has 199"
            assert host(h, n=99, n_seg=1) == -1 and "the block has 99" in err()
            assert host(h, n=1000, n_seg=3, hop=1 << 63) == -1 and "the block has 1000" in err()      # a product that would wrap
            assert host(h, n=200) == 0, err()
            assert host(h, n=4097, n_seg=1) == -1 and err() == "block of 4097 samples, the handle stages at most 4096 (max_host_samples)"
        n_dev = C.c_int()
        assert lib.tdsa_device_count(C.byref(n_dev)) == 0
        if n_dev.value > 1:                                                                # a plan on another device
            from topdogspectrumanalyser_amd import SpectrumEngine
            with SpectrumEngine(64, device=1) as eng:
                assert lib.tdsa_eye_process_dev(a._h, eng._h, Pt(d_x.ptr), 100, 100, 2, Pt(pc), None) == -1
                assert err() == "plan and eye diagram handle live on different devices"
        assert lib.tdsa_eye_read(a._h, None, Pt(pt)) == -1 and err() == "null counts"
        assert lib.tdsa_eye_read(a._h, Pt(pt), None) == -1 and err() == "null totals"
        assert lib.tdsa_eye_timer_end(a._h, None) == -1 and err() == "null elapsed_ms"
        with pytest.raises(ValueError, match="3 clocks for n_seg=2"):
            a.process_device(None, d_x.ptr, 100, 100, 2, a.clocks(delta=1.0, n_seg=3))
        with pytest.raises(ValueError, match="5 clocks: 1 .. 4 segments"):
            a.process(x, 100, a.clocks(delta=1.0, n_seg=5))
        a.timer_begin()
        assert dev(a._h) == 0 and a.timer_end() >= 0.0


# ---- 10: past 2^32 bytes ------------------------------------------------------------------------------------------------------------
def test_a_segment_past_4_gib():
    """Two segments, the second 2^29 + 1 complex samples on: the input offset is past 2^32 bytes.  Only the two segments
    are uploaded."""
    sps, L, hop, P = 4.37, 1500, (1 << 29) + 1, 16
    segs = [sc.make_signal("qpsk", sps, L, seed=20 + g)[0].astype(np.complex64) for g in range(2)]
    with ey.EyeDiagram(sps, "iq", points=P, rows=40, **SMALL) as e, ey.EyeDiagram(sps, "iq", points=P, rows=40, **SMALL) as e_h:
        K = e.symbols_per_segment(L)
        ck = e.clocks(delta=3.3, n_seg=2)
        ck["step_f"], ck["theta_fx"] = (77777, 4000000000), (5, 6)
        with room_or_skip((hop + L) * 8) as d_x, DeviceBuffer(8 * 2 * (K - 2) * P) as d_t:
            d_x.put(segs[0])
            d_x.put(segs[1], hop * 8)
            e.process_device(None, d_x.ptr, L, hop, 2, ck, d_t.ptr)
            img = e.read()
            tr = d_t.get((2, K - 2, P), np.complex64)
        tr_h = e_h.process(np.concatenate(segs), L, ck, traces=True)
        assert _bits(tr, tr_h) and _image_bits(img, e_h.read())
        _same_image(img, tr, K, 0)


# ---- 11: end to end ------------------------------------------------------------------------------------------------------------------
def test_bursts_through_the_down_converter_open_their_eyes():
    """A GFSK burst -> DownConverter -> FskAnalyzer -> EyeDiagram("fm"), and a QPSK burst -> DownConverter -> SymbolSync ->
    EyeDiagram("iq"): the opening of the device's image is the opening of the contract's image of the device's traces,
    and both eyes are open."""
    from topdogspectrumanalyser_amd import DownConverter, design_decimator
    sps, L, D, P, H = 8, 1023, 2, 32, 64
    taps = design_decimator(D)
    n = D * (3 * L + 64)
    x, _, _ = fc.make_fsk(2, sps * D, n, 0.5, 0.5, seed=11)
    with DownConverter(D, 1.0, taps=taps) as ddc, fk.FskAnalyzer(sps, 2) as a, \
            ey.EyeDiagram(sps, "fm", points=P, rows=H, v_range=(-0.15, 0.25), **SMALL) as e:
        y = ddc.process(x.astype(np.complex64))
        r = a.process(y, L)
        tr = e.process(y, L, e.clocks(r), traces=True)
        img = e.read()
        th = float(ey.EyeImage.thresholds_from(r)[0])
    counts, _ = ec.bin_traces(tr, np.float32(-0.15), np.float32(0.25), H)
    got, want = img.opening(th), ec.opening(counts[0], img.lo, img.hi, th)
    print("gfsk opening (height, width):", got)
    assert got == want and got[0] > 0 and got[1] > 0
    x, _, _ = sc.make_signal("qpsk", sps * D, n, seed=12)
    with DownConverter(D, 1.0, taps=taps) as ddc, sy.SymbolSync(sps, "qpsk") as s, \
            ey.EyeDiagram(sps, "iq", points=P, rows=H, v_range=(-1.5, 1.5), **SMALL) as e:
        y = ddc.process(x.astype(np.complex64))
        r = s.process(y, L)
        tr = e.process(y, L, e.clocks(r), traces=True)
        img = e.read()
    counts, _ = ec.bin_traces(tr, np.float32(-1.5), np.float32(1.5), H)
    for q in (0, 1):
        got, want = img.opening(0.0, eye=q), ec.opening(counts[q], img.lo, img.hi, 0.0)
        print("qpsk opening (height, width) of eye", q, got)
        assert got == want and got[0] > 0 and got[1] > 0
