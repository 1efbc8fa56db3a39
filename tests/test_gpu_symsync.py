"""The symbol recovery on the device (tdsa_symsync_*) against tests/symsync_contract.py: exact
where the contract's arithmetic is exact (integer positions, powers of two, quarter turns), within derived bounds stage
by stage elsewhere - each stage is handed the device's own result of the stage before, so a bound never has to absorb a
decision taken on the other side of a seam - and bit-equal across n_seg, the segment's place and the entry point."""
import math

import numpy as np
import pytest

import symsync_contract as sc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, _native as nat
from topdogspectrumanalyser_amd import symbols as sy

pytestmark = pytest.mark.gpu

SPS_ALL = (4, 4.37, 5, 8 - 2.0 ** -20, 8, 16, 33.3, 64)
SPS_INT = (4, 5, 8, 16, 64)
ONE = sc.ONE
J = np.array([1, 1j, -1, -1j])              # j^q, exactly


def seg_lens(sps):
    """The smallest segment with K = 2, 255 .. 16384, and the largest with K = 4096, where K is within 2 .. 4096."""
    step = sc.step_of(sps)
    lo = -(-3 * step // ONE) + 4
    hi = -(-4098 * step // ONE) - 1 + 4
    assert sc.symbols_per_segment(step, lo) == 2 and sc.symbols_per_segment(step, lo - 1) == 1
    assert sc.symbols_per_segment(step, hi) == 4096 and sc.symbols_per_segment(step, hi + 1) == 4097
    return sorted({L for L in (lo, 255, 256, 257, 1023, 4097, 16384, hi) if 2 <= sc.symbols_per_segment(step, L) <= 4096})


def layouts(seg_len):
    """(n_seg, hop) of every segment length: one segment; two with the hop above and at the segment's length; 257 that
    overlap, five samples apart."""
    return [(1, seg_len), (2, seg_len + 3), (2, seg_len), (257, 5)]


@pytest.fixture(scope="module")
def syncs():
    """SymbolSync handles by configuration, made once."""
    made = {}

    def get(sps, **kw):
        key = (sps, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = sy.SymbolSync(sps, **kw)
        return made[key]
    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(11)
    n = 2 * (64 * 4098 + 8) + 16
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _run(s, x, L, hop, n_seg, stride):
    """(symbols, raw, records) of n_seg segments of x, rows `stride` wide with the sentinel where nothing is written:
    through the host entry point where its staging takes the call, else through the device entry point."""
    if n_seg * L <= s.max_host_samples:
        r = s.process(x, L, hop, raw=True, out_stride=stride)
        return r.symbols, r.raw, r.records
    with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * n_seg * stride) as d_s, DeviceBuffer(8 * n_seg * stride) as d_r:
        d_x.put(x)
        d_s.put(np.full(n_seg * stride, sy.SENTINEL))
        d_r.put(np.full(n_seg * stride, sy.SENTINEL))
        r = s.process_device(None, d_x.ptr, L, hop, n_seg, d_s.ptr, stride, d_r.ptr)
        return d_s.get((n_seg, stride), np.complex64), d_r.get((n_seg, stride), np.complex64), r.records


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _c128(x):
    return np.asarray(x).astype(np.complex128)


# ---- exact: integer positions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", SPS_INT)
def test_fixed_integer_timing_picks_the_samples_exactly(syncs, noise, sps):
    """mu = 0: the symbols are x[delta + k sps] bit for bit - every index, seam and stride, no tolerance; the gaps of a
    wider out_stride keep the sentinel."""
    for delta in sorted({1, 2, sps - 1, sps}):
        s = syncs(sps, timing=float(delta), carrier=False)
        for L in seg_lens(sps):
            K = s.symbols_per_segment(L)
            for n_seg, hop in layouts(L):
                x = noise[:(n_seg - 1) * hop + L]
                sym, raw, rec = _run(s, x, L, hop, n_seg, K + 3)
                idx = (np.arange(n_seg) * hop)[:, None] + delta + np.arange(K)[None, :] * sps
                assert np.array_equal(sym[:, :K], x[idx]), (delta, L, n_seg, hop)
                assert np.array_equal(raw[:, :K], x[idx]), (delta, L, n_seg, hop)
                assert np.all(sym[:, K:] == sy.SENTINEL) and np.all(raw[:, K:] == sy.SENTINEL)
                assert np.all(rec["delta_fx"] == delta * ONE) and not rec["flags"].any()
                assert np.all(rec["step_f"] == 0) and np.all(rec["theta_fx"] == 0)


def _turn(y, m):
    """y (-j)^m for integer m, exactly."""
    y = np.asarray(y, dtype=np.complex64)
    out = y.copy()
    m = np.asarray(m) % 4
    out[m == 1] = (y.imag - 1j * y.real)[m == 1]
    out[m == 2] = -y[m == 2]
    out[m == 3] = (-y.imag + 1j * y.real)[m == 3]
    return out


@pytest.mark.parametrize("sps", SPS_INT)
@pytest.mark.parametrize("M,ref", [(2, 0.0), (2, math.pi), (4, 0.0), (8, 0.0)])
def test_powers_of_two_on_quarter_turns_come_back_exactly(syncs, M, ref, sps):
    """x = 2^e j^q with a carrier of whole quarter turns: z = y^M is exact and real, so g*, step_f, theta_fx and the
    derotated symbols are exact, at every shape of the test above.  Segments apart carry c = 0 .. 3 quarter turns per
    symbol on their symbol instants; segments that overlap share their samples, so there every sample carries `a`
    quarter turns per sample, which is c = a sps mod 4 per symbol and a whole number of quarter turns of phase per
    segment.  With M = 2 a segment's z may be negative real: its argument is pi from either side in float64, so
    theta_fx is compared modulo 2^32 / M, and the symbols against the device's own theta_fx."""
    rng = np.random.default_rng(16 * M + sps)
    s = syncs(sps, timing=2.0, order=M, ref_arg=ref)
    for L in seg_lens(sps):
        K = s.symbols_per_segment(L)
        for n_seg, hop in layouts(L):
            apart = hop >= L
            for c in range(4) if (n_seg, hop) != (1, L) else (1,):
                n = (n_seg - 1) * hop + L
                e = rng.integers(-1, 2, n)
                d = rng.integers(0, 2, n) * 2 if M == 2 else rng.integers(0, 4, n)
                if apart:
                    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
                    for g in range(n_seg):
                        at = g * hop + 2 + np.arange(K) * sps
                        x[at] = (np.ldexp(1.0, e[at]) * J[(d[at] + c * np.arange(K)) % 4]).astype(np.complex64)
                    c_sym = c
                else:
                    x = (np.ldexp(1.0, e) * J[(d + c * np.arange(n)) % 4]).astype(np.complex64)
                    c_sym = c * sps % 4
                sym, raw, rec = _run(s, x, L, hop, n_seg, K)
                idx = (np.arange(n_seg) * hop)[:, None] + 2 + np.arange(K)[None, :] * sps
                assert np.array_equal(raw, x[idx]), (L, n_seg, c)
                want_step = (c_sym % 2) * 0xC0000000 if M == 2 else 0        # M = 4, 8: whole quarter turns are invisible
                assert np.all(rec["step_f"] == want_step), (L, n_seg, c, np.unique(rec["step_f"]))
                assert np.all(rec["g"] == (c_sym % 2) * sc.grid(K) // 2 if M == 2 else rec["g"] == 0), (L, n_seg, c)
                assert np.all(rec["theta_fx"] % (1 << 30) == 0) and not rec["flags"].any()
                assert np.all(rec["peak"] > 0) and np.all(rec["mean"] > 0)
                m = (rec["theta_fx"].astype(np.int64)[:, None] + np.arange(K)[None, :] * want_step) % ONE // (1 << 30)
                for g in range(n_seg):
                    assert np.array_equal(sym[g], _turn(raw[g], m[g])), (L, n_seg, c, g)
                if M == 2 and ref == 0.0:
                    assert np.all(sym.imag == 0)                             # bpsk back on the real axis
                for g in sorted({0, n_seg // 2, n_seg - 1}):
                    want = sc.recover(_c128(x[g * hop:g * hop + L]), sps, M, ref, delta_fx=2 * ONE)
                    assert (rec["g"][g], rec["step_f"][g]) == (want["g"], want["step_f"]), (L, n_seg, c, g)
                    assert (int(rec["theta_fx"][g]) - want["theta_fx"]) % (ONE // M) == 0, (L, n_seg, c, g)


# ---- stage by stage ---------------------------------------------------------------------------------------------------------
def _check_stages(r, x, sps, M, ref, L, hop, what):
    """Every segment of result r (made with raw=True) against the contract, each stage from the device's own input.
    Returns the number of segments whose theta_fx was held absolutely."""
    step, nu = sc.step_of(sps), sc.nu_of(sps)
    worst = dict(c=0.0, delta=0.0, raw=0.0, peak=0.0, step_f=0.0, theta=0.0, sym=0.0)
    absolute = 0                     # segments whose theta_fx was compared modulo 2^32, not modulo 2^32 / M
    for g in range(r.records.size):
        seg = _c128(x[g * hop:g * hop + L])
        rec = r.records[g]
        K = sc.symbols_per_segment(step, L)
        # 1 timing
        Cw, Pw, dw = sc.timing(seg, nu, step)
        assert abs(Cw) >= 0.05 * Pw, (what, g, abs(Cw) / Pw)           # the bound says something
        eb = sc.timing_bound(Pw, L)
        ec = max(abs(rec["c_re"] - Cw.real), abs(rec["c_im"] - Cw.imag), abs(rec["p"] - Pw))
        worst["c"] = max(worst["c"], ec / eb)
        assert ec <= eb, (what, g, ec, eb)
        db = sc.delta_bound(Cw, Pw, L, step)
        dd = (int(rec["delta_fx"]) - dw) % step
        dd = min(dd, step - dd)
        worst["delta"] = max(worst["delta"], dd / db)
        assert dd <= db, (what, g, dd, db)
        d = int(rec["delta_fx"])
        assert ONE <= d < step + ONE
        # 2 resample, from the device's delta_fx
        yr, mr = sc.resample(seg.real, d, step, K, True)
        yi, mi = sc.resample(seg.imag, d, step, K, True)
        raw = _c128(r.raw[g])
        er = np.maximum(np.abs(raw.real - yr.real) / np.maximum(sc.resample_bound(mr), 1e-300),
                        np.abs(raw.imag - yi.real) / np.maximum(sc.resample_bound(mi), 1e-300))
        worst["raw"] = max(worst["raw"], float(er.max()))
        assert er.max() <= 1.0, (what, g, float(er.max()))
        if not M:
            assert _bits(r.symbols[g], r.raw[g])
            continue
        # 3 carrier, from the device's raw symbols
        own = sc.carrier(raw, M, ref)
        pb = sc.power_bound(own["z"], M)
        gd = int(rec["g"])
        assert 0 <= gd < own["G"]
        assert own["power"][gd] >= own["peak"] - 2 * pb, (what, g, gd, own["g"])     # a neighbour may win a near tie
        assert abs(rec["peak"] - own["power"][gd]) <= pb and rec["peak"] >= own["peak"] - pb, (what, g)
        worst["peak"] = max(worst["peak"], abs(rec["peak"] - own["power"][gd]) / pb)
        assert abs(rec["mean"] - own["mean"]) <= pb + 16 * sc.U * own["mean"], (what, g)
        at_g = sc.carrier(raw, M, ref, g=gd)
        half = float(np.sum(np.abs(at_g["z"][:at_g["H"]])))
        assert abs(at_g["S1"]) >= 0.02 * half and abs(at_g["S2"]) >= 0.02 * half, (what, g)   # the bound says something
        sb = sc.step_f_bound(at_g, M)
        ds = (int(rec["step_f"]) - at_g["step_own"]) % ONE
        ds = min(ds, ONE - ds)
        worst["step_f"] = max(worst["step_f"], ds / sb)
        assert ds <= sb, (what, g, ds, sb)
        at_f = sc.carrier(raw, M, ref, g=gd, step_f=int(rec["step_f"]))
        tb = sc.theta_bound(at_f, M)
        # arg of the phase sum wraps at +-pi, where theta_fx jumps by 2^32 / M: away from there the comparison is absolute
        far = 1.0 - abs(at_f["a"]) > 0.05
        span = ONE if far else ONE // M
        absolute += far
        dt = (int(rec["theta_fx"]) - at_f["theta_fx"]) % span
        dt = min(dt, span - dt)
        worst["theta"] = max(worst["theta"], dt / tb)
        assert dt <= tb, (what, g, dt, tb)
        # 4 derotation, from the device's step_f and theta_fx
        want = sc.derotate(raw, int(rec["step_f"]), int(rec["theta_fx"]))
        es = np.abs(_c128(r.symbols[g]) - want) / np.maximum(sc.derotate_bound(raw), 1e-300)
        worst["sym"] = max(worst["sym"], float(es.max()))
        assert es.max() <= 1.0, (what, g, float(es.max()))
    print(what, "worst error / bound:", {k: round(float(v), 3) for k, v in worst.items()})
    return absolute


@pytest.mark.parametrize("sps,L", [(sps, L) for sps in SPS_INT for L in seg_lens(sps)])
def test_impulse_trains_at_every_residue(syncs, sps, L):
    """|x|^2 an impulse train at t0 mod sps, every t0 < sps at every segment length: |C| = P, delta_fx = t0 2^32 up to the
    bound, whichever side of a sample."""
    s = syncs(sps, carrier=False)
    for t0 in range(sps):
        x = np.full(L, 1e-3 + 1e-3j, dtype=np.complex64)
        x[t0::sps] = 1.0 + 0.5j
        r = s.process(x, L, raw=True)
        _check_stages(r, x, sps, 0, 0.0, L, L, f"impulses sps {sps} L {L} t0 {t0}")
        near = (int(r.records["delta_fx"][0]) - t0 * ONE) % (sps * ONE)
        assert min(near, sps * ONE - near) <= sc.delta_bound(complex(1.0, 0.0), 1.0, L, sps * ONE) + ONE // 500


@pytest.mark.parametrize("sps", SPS_ALL)
@pytest.mark.parametrize("mod", ["bpsk", "qpsk", "8psk", "16qam"])
def test_every_stage_stays_within_its_bound_on_raised_cosine_data(syncs, mod, sps):
    """Raised-cosine data (excess bandwidth 0.9, so that the symbol-rate line is strong: |C| >= 0.05 P is asserted),
    carrier and noise as in the CPU test; every shape, segments that overlap and segments apart."""
    M = sc.ORDER[mod]
    ref = sc.reference_phase(sc.points(mod), M)
    s = syncs(sps, modulation=mod)
    assert s.order == M and abs(abs(s.ref_arg) - abs(ref)) < 1e-6
    for L in seg_lens(sps):
        if s.symbols_per_segment(L) < 24:
            continue                                   # too few symbols for a symbol-rate line: the exact tests cover them
        for n_seg, hop in ((2, L + 3), (3, max(1, L // 3))):
            n = (n_seg - 1) * hop + L
            x, _, _ = sc.make_signal(mod, sps, n, seed=int(sps * 8) + L, alpha=0.9, w=0.01 * 4 / sps)
            x = x.astype(np.complex64)
            r = s.process(x, L, hop, raw=True)
            assert not r.flags.any()
            _check_stages(r, x, sps, M, s.ref_arg, L, hop, f"{mod} sps {sps:g} L {L} n_seg {n_seg}")


@pytest.mark.parametrize("mod", ["bpsk", "qpsk", "8psk"])
def test_theta_is_absolute_where_the_wrap_is_far(syncs, mod):
    """Carrier phases spread over the M-fold sector: wherever the contract's phase sum points more than 0.05 half turns
    away from +-pi, theta_fx must meet the contract's modulo 2^32, not merely modulo 2^32 / M - a device theta_fx off by
    a whole symmetry step fails here."""
    M = sc.ORDER[mod]
    sps, L = 4.37, 1023
    s = syncs(sps, modulation=mod)
    held = 0
    for i in range(6):
        x, _, _ = sc.make_signal(mod, sps, 2 * L, seed=40 + i, alpha=0.9, phase=0.1 + 2 * math.pi / M * i / 6)
        x = x.astype(np.complex64)
        held += _check_stages(s.process(x, L, raw=True), x, sps, M, s.ref_arg, L, L, f"{mod} phase {i}")
    print(mod, "segments held absolutely:", held, "of 12")
    assert held >= 8


# ---- invariance ---------------------------------------------------------------------------------------------------------------
def test_a_segment_does_not_depend_on_n_seg_its_place_or_the_entry_point(syncs):
    sps, L, hop, n_seg = 4.37, 1023, 7, 257
    x, _, _ = sc.make_signal("qpsk", sps, (n_seg - 1) * hop + L, seed=5, alpha=0.9)
    x = x.astype(np.complex64)
    s = syncs(sps, modulation="qpsk")
    K = s.symbols_per_segment(L)
    many = s.process(x, L, hop, raw=True)
    assert len(set(many.records["delta_fx"].tolist())) > 8            # the segments really differ
    for g in (0, 1, 100, 256):
        one = s.process(x[g * hop:g * hop + L], L, raw=True)
        assert _bits(one.symbols[0], many.symbols[g]) and _bits(one.raw[0], many.raw[g]), g
        assert one.records[0].tobytes() == many.records[g].tobytes(), g
    stride = K + 5
    with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * n_seg * stride) as d_s, DeviceBuffer(8 * n_seg * stride) as d_r:
        d_x.put(x)
        d_s.put(np.full(n_seg * stride, sy.SENTINEL))
        d_r.put(np.full(n_seg * stride, sy.SENTINEL))
        dev = s.process_device(None, d_x.ptr, L, hop, n_seg, d_s.ptr, stride, d_r.ptr)
        sym = d_s.get((n_seg, stride), np.complex64)
        raw = d_r.get((n_seg, stride), np.complex64)
    assert dev.records.tobytes() == many.records.tobytes()
    assert _bits(sym[:, :K], many.symbols) and _bits(raw[:, :K], many.raw)
    assert np.all(sym[:, K:] == sy.SENTINEL) and np.all(raw[:, K:] == sy.SENTINEL)


def test_behind_the_down_converter_on_an_engine_stream(syncs):
    """capture -> DownConverter(D = 2, RRC taps) -> SymbolSync on the engine's stream, against the same decimated data
    staged through the host."""
    from topdogspectrumanalyser_amd import DownConverter, SpectrumEngine
    sps, L, D = 4, 1023, 2
    n = 2 * (3 * L + 40)
    x, _, _ = sc.make_signal("qpsk", sps * D, n, seed=9, alpha=0.35)
    x = x.astype(np.complex64)
    s = syncs(sps, modulation="qpsk")
    K = s.symbols_per_segment(L)
    taps = sy.rrc_taps(sps * D, 0.35, 4)
    with SpectrumEngine(64) as eng, DownConverter(D, 1.0, taps=taps) as ddc, DownConverter(D, 1.0, taps=taps) as ddc_h:
        y = ddc_h.process(x)
        n_seg = (y.size - L) // L + 1
        with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * (y.size + 8)) as d_y, DeviceBuffer(8 * n_seg * K) as d_s:
            d_x.put(x)
            ny = ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            dev = s.process_device(eng, d_y.ptr, L, L, n_seg, d_s.ptr, K)
            sym = d_s.get((n_seg, K), np.complex64)
    assert ny == y.size and n_seg == 3
    host = s.process(y, L)
    assert dev.records.tobytes() == host.records.tobytes() and _bits(sym, host.symbols)
    assert host.timing_quality.min() > 0 and not host.flags.any()


# ---- non-finite input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [complex(np.nan, 0), complex(0, np.nan), complex(np.inf, 0), complex(0, -np.inf), complex(3e19, 3e19)])
def test_a_non_finite_segment_is_flagged_and_its_neighbours_keep_their_bits(syncs, bad):
    sps, L = 5, 257
    x, _, _ = sc.make_signal("qpsk", sps, 3 * L, seed=3, alpha=0.9)
    x = x.astype(np.complex64)
    s = syncs(sps, modulation="qpsk")
    clean = s.process(x, L, raw=True)
    for at in (L, L + 100, 2 * L - 1):
        y = x.copy()
        y[at] = np.complex64(bad)
        r = s.process(y, L, raw=True)
        assert r.flags.tolist() == [0, nat.SYMSYNC_NONFINITE, 0], (at, r.flags)
        assert np.isnan(r.symbols[1].real).all() and np.isnan(r.symbols[1].imag).all() and np.isnan(r.raw[1].real).all()
        zero = np.zeros(1, dtype=sy.RECORD)
        zero["flags"] = nat.SYMSYNC_NONFINITE
        assert r.records[1].tobytes() == zero[0].tobytes()
        for g in (0, 2):
            assert _bits(r.symbols[g], clean.symbols[g]) and _bits(r.raw[g], clean.raw[g])
            assert r.records[g].tobytes() == clean.records[g].tobytes()


def test_an_all_zero_segment_is_not_an_error(syncs):
    s = syncs(4, modulation="qpsk")
    r = s.process(np.zeros(3 * 256, dtype=np.complex64), 256, raw=True)
    assert not r.flags.any() and np.all(r.records["delta_fx"] == 4 * ONE)
    assert np.all(r.records["g"] == 0) and np.all(r.records["step_f"] == 0) and np.all(r.symbols == 0) and np.all(r.raw == 0)
    assert np.all(r.timing_quality == 0) and np.all(r.lock == 0)


# ---- offsets past 2^32 bytes -----------------------------------------------------------------------------------------------------
def test_second_segment_past_4_gib(syncs):
    """Two segments, the second 2^29 + 1 samples on: past 2^32 bytes.  Only the two segments are uploaded."""
    sps, L, hop = 4.37, 4097, (1 << 29) + 1
    s = syncs(sps, modulation="qpsk")
    K = s.symbols_per_segment(L)
    segs = [sc.make_signal("qpsk", sps, L, seed=20 + g, alpha=0.9)[0].astype(np.complex64) for g in range(2)]
    stride = (1 << 29) + 3                                            # the outputs past 2^32 bytes as well
    with room_or_skip((hop + L) * 8) as d_x, room_or_skip((stride + K) * 8) as d_s:
        d_x.put(segs[0])
        d_x.put(segs[1], hop * 8)
        dev = s.process_device(None, d_x.ptr, L, hop, 2, d_s.ptr, stride)
        sym = [d_s.get((K,), np.complex64, g * stride * 8) for g in range(2)]
    for g in range(2):
        one = s.process(segs[g], L)
        assert dev.records[g].tobytes() == one.records[0].tobytes() and _bits(sym[g], one.symbols[0]), g
    assert not _bits(sym[0], sym[1])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", [4, 4.37])
@pytest.mark.parametrize("mod", ["qpsk", "16qam"])
def test_device_evm_matches_the_contracts_evm(syncs, mod, sps):
    """The CPU test's signal through SymbolSync, then Constellation.process_segments on the symbols where they lie; the
    same Constellation handle on the float64 contract's symbols of the same input.  Within 5 %: one seam decision
    (delta_fx on either side of 2^32, or t wrapping) shifts the symbol set by one symbol, which moves an rms over ~1000
    noisy symbols by far less; everything else is continuous."""
    from topdogspectrumanalyser_amd import Constellation
    L, n_seg = 4096, 2
    M = sc.ORDER[mod]
    x, _, _ = sc.make_signal(mod, sps, n_seg * L, seed=1, offset=0.37, w=0.01, phase=0.7, noise_db=-40.0)
    x = x.astype(np.complex64)
    s = syncs(sps, modulation=mod)
    K = s.symbols_per_segment(L)
    with Constellation(modulation=mod) as cst, DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * n_seg * K) as d_s:
        d_x.put(x)
        r = s.process_device(None, d_x.ptr, L, L, n_seg, d_s.ptr, K)
        _, evm_dev = cst.process_segments(None, d_s.ptr, nat.IN_C64, K, K, n_seg)
        for g in range(n_seg):
            want = sc.recover(_c128(x[g * L:(g + 1) * L]), sps, M, s.ref_arg)
            evm_ref = cst.process(want["symbols"].astype(np.complex64), counts=False).evm_rms
            ratio = evm_dev[g] / evm_ref
            print(f"{mod} sps {sps} segment {g}: device EVM {evm_dev[g]:.5f}, contract EVM {evm_ref:.5f}, ratio {ratio:.4f}, "
                  f"freq {r.freq[g]:+.6f} cycles/symbol, lock {r.lock[g]:.1f}")
            assert abs(ratio - 1.0) <= 0.05
    assert not r.flags.any()


# ---- the -1s that need a live handle ---------------------------------------------------------------------------------------------
def test_error_returns_with_a_live_handle():
    import ctypes as C
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()                                   # noqa: E731
    P = lambda addr: C.c_void_p(int(addr))                                               # noqa: E731
    x = np.zeros(8192, dtype=np.complex64)
    sym = np.zeros(8192, dtype=np.complex64)
    rw = np.zeros(8192, dtype=np.complex64)
    rec = np.zeros(64, dtype=sy.RECORD)
    px, ps, pw, pr = (v.ctypes.data for v in (x, sym, rw, rec))
    assert px % 8 == 0 and ps % 8 == 0 and pw % 8 == 0 and pr % 8 == 0
    raw = C.c_void_p()
    assert lib.tdsa_symsync_create(0, 4096, C.byref(raw)) == 0
    try:
        # no argument is wrong: the state is (TDSA_ERR_STATE)
        assert lib.tdsa_symsync_process(raw, P(px), 100, 100, 100, 1, P(ps), 64, None, P(pr)) == -3 and "not configured" in err()
        assert lib.tdsa_symsync_process_dev(raw, None, P(px), 100, 100, 1, P(ps), 64, None, P(pr)) == -3 and "not configured" in err()
        assert lib.tdsa_symsync_process(raw, None, 100, 100, 100, 1, P(ps), 64, None, P(pr)) == -3     # asked before the arguments
        assert lib.tdsa_symsync_process_dev(raw, None, P(px), 100, 100, 1, None, 64, None, P(pr)) == -3
    finally:
        assert lib.tdsa_symsync_destroy(raw) == 0
    with sy.SymbolSync(4, max_host_samples=4096) as s, DeviceBuffer(8 * 4096) as d_x, DeviceBuffer(8 * 4096) as d_s, \
            DeviceBuffer(8 * 4096) as d_w:
        K = s.symbols_per_segment(100)                                                    # 23
        assert K == 23
        host = lambda **kw: lib.tdsa_symsync_process(s._h, *[kw.get(k, v) for k, v in (                    # noqa: E731
            ("inp", P(px)), ("n", 1000), ("seg", 100), ("hop", 100), ("n_seg", 2), ("out", P(ps)), ("stride", 64), ("raw", P(pw)), ("rec", P(pr)))])
        dev = lambda **kw: lib.tdsa_symsync_process_dev(s._h, None, *[kw.get(k, v) for k, v in (           # noqa: E731
            ("inp", P(d_x.ptr)), ("seg", 100), ("hop", 100), ("n_seg", 2), ("out", P(d_s.ptr)), ("stride", 64), ("raw", P(d_w.ptr)), ("rec", P(pr)))])
        for call in (host, dev):
            assert call() == 0, err()
            assert call(raw=None) == 0, err()                                              # the raw symbols are optional
            assert call(inp=None) == -1 and err() == "null samples"
            assert call(out=None) == -1 and err() == "null symbols"
            assert call(rec=None) == -1 and err() == "null records"
            base_in, base_out, base_raw = (px, ps, pw) if call is host else (d_x.ptr, d_s.ptr, d_w.ptr)
            for off in (dict(inp=P(base_in + 4)), dict(out=P(base_out + 4)), dict(raw=P(base_raw + 4)), dict(rec=P(pr + 4))):
                assert call(**off) == -1 and err() == "pointers must be aligned to 8 bytes", off
            assert call(n_seg=0) == -1 and "n_seg=0" in err()
            assert call(n_seg=-1) == -1 and "n_seg=-1" in err()
            assert call(hop=0) == -1 and "hop=0" in err()
            assert call(stride=K - 1) == -1 and f"out_stride={K - 1}: a segment gives {K} symbols" in err()
            assert call(stride=K) == 0, err()
            # K outside 2 .. 4096: K = floor((seg_len - 4) / 4) - 1
            assert call(seg=15, hop=15, n_seg=1) == -1 and "seg_len=15 gives 1 symbols per segment: 2 .. 4096" in err()
            assert call(seg=3, hop=3, n_seg=1) == -1 and "gives -1 symbols" in err()
            assert call(seg=16396, hop=1, n_seg=1) == -1 and "gives 4097 symbols" in err()
            if call is host:
                assert call(seg=16, hop=16, n_seg=1) == 0, err()
        # the host entry point alone: the block and the staging
        assert host(n=199) == -1 and "need 200 samples, the block has 199" in err()
        assert host(n=99, n_seg=1) == -1 and "the block has 99" in err()
        assert host(n=1000, n_seg=3, hop=1 << 63) == -1 and "the block has 1000" in err()             # a product that would wrap
        assert host(n=200) == 0, err()
        assert host(n=4097, n_seg=1) == -1 and "the handle stages at most 4096 (max_host_samples)" in err()
        assert host(n=149, n_seg=50, hop=1) == -1 and "max_host_samples" in err()                     # 50 segments of 100 overlap
        assert host(n=139, n_seg=40, hop=1) == 0, err()
        n_dev = C.c_int()
        assert lib.tdsa_device_count(C.byref(n_dev)) == 0
        if n_dev.value > 1:                                                                # a plan on another device
            from topdogspectrumanalyser_amd import SpectrumEngine
            with SpectrumEngine(64, device=1) as eng:
                assert lib.tdsa_symsync_process_dev(s._h, eng._h, P(d_x.ptr), 100, 100, 2, P(d_s.ptr), 64, None, P(pr)) == -1
                assert "different devices" in err()
        assert lib.tdsa_symsync_timer_end(s._h, None) == -1 and err() == "null elapsed_ms"
        s.timer_begin()
        assert dev() == 0 and s.timer_end() >= 0.0
