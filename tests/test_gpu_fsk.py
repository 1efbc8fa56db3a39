"""The FSK analysis on the device (tdsa_fsk_*) against tests/fsk_contract.py: bit for bit where
the contract's arithmetic is exact or restated operation by operation (the boxcar, integer positions, quarter turns,
everything from the levels v on), within derived bounds stage by stage elsewhere - each stage is handed the device's own
result of the stage before - and bit-equal across n_seg, the segment's place and the entry point."""
import math

import numpy as np
import pytest

import fsk_contract as fc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, _native as nat
from topdogspectrumanalyser_amd import fsk as fk

pytestmark = pytest.mark.gpu

SPS_ALL = (4, 4.37, 5, 8 - 2.0 ** -20, 8, 16, 33.3, 64)
SPS_INT = (4, 5, 8, 16, 64)
BOXCARS = (1, 2, 3, 32, 64)
LAGS = (1, 2, 33, 64)
LEVELS = (2, 4, 8)
ONE = fc.ONE
TILE = 1024                                  # the timing stage's tile of differences (tdsa_fsk.hpp: kFskTile)
KINDS = {fc.IQ: "iq", fc.FREQ: "freq"}
DTYPE = {fc.IQ: np.complex64, fc.FREQ: np.float32}


def seg_len_of(n_b, kind, B):
    return n_b + B - 1 + (1 if kind == fc.IQ else 0)


def seg_lens(sps, kind, B, L, largest=False):
    """The smallest segment with K = 2; those that put n_b - L, the number of differences, at 255, 256, 257 and one past
    each of the timing stage's first two tiles; with `largest` the largest with K = 4096.  Only those with K in 2 .. 4096."""
    step = fc.step_of(sps)
    lo = seg_len_of(-(-3 * step // ONE) + 4, kind, B)
    hi = seg_len_of(-(-4098 * step // ONE) - 1 + 4, kind, B)
    assert fc.symbols_per_segment(step, lo, kind, B) == 2 and fc.symbols_per_segment(step, lo - 1, kind, B) == 1
    assert fc.symbols_per_segment(step, hi, kind, B) == 4096 and fc.symbols_per_segment(step, hi + 1, kind, B) == 4097
    lens = {lo} | {seg_len_of(n_e + L, kind, B) for n_e in (255, 256, 257, TILE + 1, 2 * TILE + 1)} | ({hi} if largest else set())
    return sorted(n for n in lens if 2 <= fc.symbols_per_segment(step, n, kind, B) <= 4096)


def layouts(seg_len):
    """(n_seg, hop): one segment; two with the hop above the segment's length; three with it at the length; three
    that overlap; 257 that overlap, five samples apart, where the segment is short."""
    out = [(1, seg_len), (2, seg_len + 3), (3, seg_len), (3, max(1, seg_len - 7))]
    return out + ([(257, 5)] if seg_len <= 1200 else [])


@pytest.fixture(scope="module")
def analysers():
    """FskAnalyzer handles by configuration, made once."""
    made = {}

    def get(sps, **kw):
        key = (sps, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = fk.FskAnalyzer(sps, **kw)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def _run(a, x, L, hop, n_seg, stride):
    """(levels, indices, records) of n_seg segments of x, rows `stride` wide with the sentinels where nothing is
    written: through the host entry point where its staging takes the call, else through the device entry point."""
    if n_seg * L <= a.max_host_samples and x.size <= a.max_host_samples:
        r = a.process(x, L, hop, out_stride=stride)
        return r.levels, r.indices, r.records
    with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(4 * n_seg * stride) as d_v, DeviceBuffer(n_seg * stride) as d_i:
        d_x.put(x)
        d_v.put(np.full(n_seg * stride, fk.SENTINEL, dtype=np.float32))
        d_i.put(np.full(n_seg * stride, fk.SENTINEL_INDEX, dtype=np.uint8))
        r = a.process_device(None, d_x.ptr, L, hop, n_seg, d_v.ptr, stride, d_i.ptr)
        return d_v.get((n_seg, stride), np.float32), d_i.get((n_seg, stride), np.uint8), r.records


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_record(rec, own, what):
    """The device's record against fsk_contract.levels() of the device's own v: every field of stages 4 and 5."""
    for name, key in (("offset", "offset"), ("dev", "dev"), ("lo", "lo"), ("hi", "hi"), ("err_peak", "err_peak"),
                      ("err_sumsq", "err_sumsq"), ("err_peak_k", "err_peak_k"), ("sum_l", "sum_l"), ("flags", "flags")):
        assert rec[name] == own[key], (what, name, rec[name], own[key])


# ---- exact: the boxcar restated, integer positions, the whole record --------------------------------------------------------
@pytest.mark.parametrize("sps", SPS_INT)
def test_freq_input_with_fixed_integer_timing_is_exact(sps):
    """float32 input, integer sps, fixed integer timing: b is numpy's float32 restated operation by operation, mu = 0
    picks v_k = b[delta + k sps] bit for bit at every index, seam and stride, and from v on the contract restates the
    device exactly, so the whole record and the indices match; the gaps of a wider stride keep the sentinels."""
    rng = np.random.default_rng(sps)
    n_base = max(4400 * sps, 8192)
    base = (np.repeat(2.0 * rng.integers(0, 8, n_base // sps + 1) - 7.0, sps)[:n_base] * 0.03 + 0.1
            + 0.01 * rng.standard_normal(n_base)).astype(np.float32)
    n_run = 0
    for nb, B in enumerate(BOXCARS):
        lag, M = LAGS[nb % 4], LEVELS[nb % 3]
        for delta in sorted({1, sps}):
            with fk.FskAnalyzer(sps, M, input="freq", timing=float(delta), boxcar=B, lag=lag) as a:
                for L in seg_lens(sps, fc.FREQ, B, lag, largest=sps in (4, 64) and B in (1, 64) and delta == 1):
                    K = a.symbols_per_segment(L)
                    for n_seg, hop in layouts(L) if K < 4096 else [(1, L), (2, 5)]:
                        x = base[:(n_seg - 1) * hop + L]
                        lev, idx, rec = _run(a, x, L, hop, n_seg, K + 3)
                        n_run += 1
                        assert np.all(lev[:, K:] == fk.SENTINEL) and np.all(idx[:, K:] == fk.SENTINEL_INDEX)
                        assert np.all(rec["delta_fx"] == delta * ONE)
                        for g in sorted({0, 1, n_seg // 2, n_seg - 1} & set(range(n_seg))):
                            what = (B, lag, M, delta, L, n_seg, hop, g)
                            b = fc.boxcar32(x[g * hop:g * hop + L], B)
                            want = b[delta + np.arange(K) * sps]
                            assert _bits(lev[g, :K], want), what
                            own = fc.levels(want, M)
                            _same_record(rec[g], own, what)
                            assert np.array_equal(idx[g, :K], own["indices"]), what
    print(f"sps {sps}: {n_run} calls")


@pytest.mark.parametrize("M", LEVELS)
def test_levels_on_a_binary_grid_give_an_exact_record(analysers, M):
    """Levels o + l 2^-5 held for a whole symbol, B = 1 and 2, the symbol centres picked: every sum is exact in float64,
    so o, g, the indices, sum_l are the signal's own and err_sumsq = err_peak = 0."""
    sps, L = 8, 1023
    for B in (1, 2):
        f, sent = fc.make_freq(M, sps, 3 * L, 2.0 ** -5, 0.375, seed=M, t0=3)
        a = analysers(sps, levels=M, input="freq", timing=float(3 + 4), boxcar=B, lag=3)
        r = a.process(f.astype(np.float32), L)
        K = a.symbols_per_segment(L)
        for g in range(3):
            m = (g * L + 7 + np.arange(K) * sps + (B - 1) // 2 - 3) // sps          # the symbol each centre lies in
            rec = r.records[g]
            assert np.array_equal(r.indices[g], sent[m + 5]), (B, g)
            assert (rec["offset"], rec["dev"], rec["err_sumsq"], rec["err_peak"], rec["err_peak_k"]) == (0.375, 2.0 ** -5, 0, 0, 0)
            assert rec["sum_l"] == int(np.sum(2 * sent[m + 5].astype(np.int64) - (M - 1))) and rec["flags"] == 0
            assert rec["lo"] == 0.375 - (M - 1) * 2.0 ** -5 and rec["hi"] == 0.375 + (M - 1) * 2.0 ** -5
            assert np.array_equal(r.levels[g], 0.375 + (2.0 * sent[m + 5] - (M - 1)) * 2.0 ** -5)


@pytest.mark.parametrize("sps", SPS_INT)
def test_iq_input_with_quarter_turn_steps_is_exact(analysers, sps):
    """x = j^c with c stepping by +1 or -1 per sample, a symbol at a time: d is +1/2 or -1/2 exactly, so the 2-level
    record and the indices are exact: o = 0, g = 1/2, no error; also d = 0 and 1 (steps of 0 and 2) as the two levels."""
    rng = np.random.default_rng(100 + sps)
    J = np.array([1, 1j, -1, -1j])
    for steps, o, g in (((-1, 1), 0.0, 0.5), ((0, 2), 0.5, 0.5)):
        for B in (1, 2):
            L = 75 * sps + 40 + B
            n_seg, hop = 3, (L // sps + 2) * sps                                     # every segment begins on a symbol's edge
            n = (n_seg - 1) * hop + L
            sent = rng.integers(0, 2, n // sps + 2)
            inc = np.repeat(np.array(steps)[sent], sps)[:n - 1]                     # d_j: the step from x[j] to x[j + 1]
            x = J[np.concatenate([[0], np.cumsum(inc)]) % 4].astype(np.complex64)
            delta = 1 + (B == 1)                                                     # inside the flat part of a symbol
            a = analysers(sps, levels=2, timing=float(delta), boxcar=B, lag=2)
            K = a.symbols_per_segment(L)
            r = a.process(x, L, hop)
            for s in range(n_seg):
                j = s * hop + delta + np.arange(K) * sps                             # b_j = (d_j + d_j+B-1) / B
                want = sent[j // sps]
                assert np.array_equal(sent[(j + B - 1) // sps], want)                # both terms inside one symbol
                rec = r.records[s]
                assert np.array_equal(r.indices[s], want), (steps, B, s)
                assert np.array_equal(r.levels[s], o + g * (2.0 * want - 1)), (steps, B, s)
                assert (rec["offset"], rec["dev"], rec["err_sumsq"], rec["err_peak"], rec["flags"]) == (o, g, 0, 0, 0)
                assert rec["sum_l"] == int(np.sum(2 * want - 1)) and (rec["lo"], rec["hi"]) == (o - g, o + g)
                assert rec["delta_fx"] == delta * ONE


# ---- stage by stage ---------------------------------------------------------------------------------------------------------
def _prepare(seg, sps, M, kind, B, L, lone=True):
    """The CPU's side of one segment before the device runs: the contract's chain, its bounds, and the proof that every
    decision and the place of the largest error are safe from the device's rounding.  lone: the signal was made with one
    error that stands out; without it the place of the largest error is compared only where it happens to be safe."""
    step, nu = fc.step_of(sps), fc.nu_of(sps)
    K = fc.symbols_per_segment(step, seg.size, kind, B)
    d = fc.discriminate(seg.astype(np.complex128)) if kind == fc.IQ else seg.astype(np.float64)
    b = fc.boxcar(d, B)
    eb = fc.boxcar_bound(float(np.abs(d).max()), kind, B)
    C, P, dl = fc.timing(b, nu, step, L)
    assert abs(C) >= 0.05 * P, abs(C) / P                                         # the bound says something
    e_c = fc.timing_bound(b, L, eb)
    db = fc.delta_bound(C, e_c, step)
    v, mag, sumc = fc.resample(b, dl, step, K, True)
    # v under the device's rounding and under a delta_fx up to db counts away: the cubic's slope is below 4 max |b_j+1 - b_j|
    vb = float(np.max(fc.resample_bound(mag, sumc, eb))) + 4.0 * float(np.abs(np.diff(b)).max()) * db / ONE
    own = fc.levels(v.astype(np.float32), M)
    assert own["flags"] == 0
    shift = fc.threshold_shift(own["l"], vb + fc.U * float(np.abs(v).max()), M)
    for o, g in own["deciders"]:
        margin = fc.threshold_margin(v, o, g, M)
        need = vb + shift + fc.A_DEC * fc.U * (M / 2 + 1) * 2 * abs(float(g))
        assert margin.min() > need, (margin.min(), need)                          # no symbol is left undecided
    ae = np.sort(np.abs(own["err"].astype(np.float64)))
    safe_peak = ae[-1] - ae[-2] > 2 * (vb + shift + (M - 1) * shift)
    assert safe_peak or not lone, (ae[-1], ae[-2], vb, shift)                      # no tie decides err_peak_k
    return dict(safe_peak=safe_peak, K=K, b=b, eb=eb, C=C, P=P, delta=dl, e_c=e_c, db=db, own=own, step=step, vb=vb, shift=shift)


def _check_stages(p, lev, idx, rec, M, what, worst):
    """One segment of the device's result against what _prepare made of it."""
    step, K = p["step"], p["K"]
    ec = max(abs(rec["c_re"] - p["C"].real), abs(rec["c_im"] - p["C"].imag), abs(rec["p"] - p["P"]))
    worst["c"] = max(worst["c"], ec / p["e_c"])
    assert ec <= p["e_c"], (what, ec, p["e_c"])
    d = int(rec["delta_fx"])
    assert ONE <= d < step + ONE
    dd = (d - p["delta"]) % step
    dd = min(dd, step - dd)
    worst["delta"] = max(worst["delta"], dd / p["db"])
    assert dd <= p["db"], (what, dd, p["db"])
    # 3 resample, from the device's delta_fx
    v, mag, sumc = fc.resample(p["b"], d, step, K, True)
    ev = np.abs(lev.astype(np.float64) - v) / fc.resample_bound(mag, sumc, p["eb"])
    worst["v"] = max(worst["v"], float(ev.max()))
    assert ev.max() <= 1.0, (what, float(ev.max()))
    # 4, 5 from the device's v: the contract restates them exactly; o and g are held to the fit's bound by name
    own = fc.levels(lev, M)
    assert abs(float(rec["offset"]) - float(own["offset"])) <= fc.fit_bound(own["offset"], own["dev"]), what
    assert abs(float(rec["dev"]) - float(own["dev"])) <= fc.fit_bound(own["offset"], own["dev"]), what
    _same_record(rec, own, what)
    assert np.array_equal(idx, own["indices"]), what
    # ... and the decisions the CPU proved safe, against the contract's own chain (a delta_fx across the seam at 2^32
    # moves the symbols by one)
    sh = int(round((d - p["delta"]) / step))
    mine, theirs = (idx[:K - sh], p["own"]["indices"][sh:]) if sh >= 0 else (idx[-sh:], p["own"]["indices"][:K + sh])
    assert abs(sh) <= 1 and np.array_equal(mine, theirs), (what, sh)
    if sh == 0:
        assert rec["sum_l"] == p["own"]["sum_l"], what
        assert rec["err_peak_k"] == p["own"]["err_peak_k"] or not p["safe_peak"], what
        tol = 2 * (p["vb"] + M * p["shift"])
        assert abs(float(rec["err_peak"]) - float(p["own"]["err_peak"])) <= tol, what
        rms_c, rms_d = math.sqrt(p["own"]["err_sumsq"] / K), math.sqrt(rec["err_sumsq"] / K)
        assert abs(rms_d - rms_c) <= tol, (what, rms_d, rms_c)


@pytest.mark.parametrize("sps", SPS_INT)
@pytest.mark.parametrize("bt", [None, 0.5])
def test_every_stage_stays_within_its_bound_at_every_residue(analysers, sps, bt):
    """Rectangular and Gaussian FSK whose symbol boundaries sit at every residue t0 < sps: complex64 for t0 even, the
    same frequency as float32 for t0 odd; B and L rotate, and M where the pulses are rectangular.  |C| >= 0.05 P, the
    decisions' margins and the lone peak error are asserted on the CPU before the device runs."""
    worst = dict(c=0.0, delta=0.0, v=0.0)
    n_sym = 48
    for t0 in range(sps):
        M = LEVELS[t0 % 3] if bt is None else 2          # Gaussian pulses close a 4-level eye too far for the first guess's margins
        kind = fc.IQ if t0 % 2 == 0 else fc.FREQ
        B, L = max(1, sps // 2 - (t0 % 2)), max(1, sps // 2 + (t0 % 3) - 1)
        seg_len = n_sym * sps + 11 + t0
        n_seg, hop = 2, seg_len - 3 * sps - 1
        n = (n_seg - 1) * hop + seg_len
        h = 0.5 if M == 2 else 0.3 if M == 4 else 0.2
        # one symbol in the middle of each segment stands between two of its own kind, free of intersymbol interference,
        # and a quarter of a level spacing off its level, outwards: the lone largest error by construction
        rng = np.random.default_rng(1000 * sps + t0)
        sent = rng.integers(0, M, n // sps + 16)
        lone = [20 + g * (hop // sps + 2) for g in range(n_seg)]
        for m in lone:
            sent[m + 4:m + 7] = sent[m + 5]                                        # symbol m is stored at [m + 5]
            sent[m + 5 + 4], sent[m + 5 + 6] = 0, M - 1                            # both outer levels are there for the first guess
        f, _ = fc.make_freq(M, sps, n + 1, h / sps, 0.013, t0=t0, bt=bt, symbols=sent)
        f = f + 2e-4 * rng.standard_normal(f.size)
        for m in lone:
            f[t0 + m * sps:t0 + (m + 1) * sps] += (0.5 if 2 * sent[m + 5] > M - 1 else -0.5) * h / sps     # outwards
        if kind == fc.IQ:
            x = np.exp(1j * np.pi * np.concatenate([[0.0], np.cumsum(f[:n - 1])])).astype(np.complex64)
        else:
            x = f[:n].astype(np.float32)
        prep = [_prepare(x[g * hop:g * hop + seg_len], sps, M, kind, B, L) for g in range(n_seg)]
        a = analysers(sps, levels=M, input=KINDS[kind], boxcar=B, lag=L)
        r = a.process(x, seg_len, hop)
        assert not r.flags.any()
        for g in range(n_seg):
            _check_stages(prep[g], r.levels[g], r.indices[g], r.records[g], M, (sps, bt, t0, g), worst)
    print(f"sps {sps} BT {bt}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("sps", SPS_ALL)
def test_every_stage_stays_within_its_bound_at_any_symbol_rate(analysers, sps):
    """The CPU test's signals (GFSK and rectangular 4-FSK with a carrier offset, noise 40 dB down) at every sps, default B
    and L, segments that overlap and segments apart, at lengths around the workgroup's width and the timing stage's tile."""
    worst = dict(c=0.0, delta=0.0, v=0.0)
    B = fc.default_boxcar(sps)
    for M, h, bt in ((2, 0.5, 0.5), (4, 0.5, None)):
        for n_e in (257, TILE + 1) if sps <= 16 else (TILE + 1, 2 * TILE + 1):
            L = seg_len_of(n_e + B, fc.IQ, B)
            if fc.symbols_per_segment(fc.step_of(sps), L, fc.IQ, B) < 24:
                continue
            for n_seg, hop in ((2, L + 3), (3, max(1, L // 3))):
                n = (n_seg - 1) * hop + L
                x, _, _ = fc.make_fsk(M, sps, n, h, bt, seed=int(sps * 8) + L, cfo=0.003)
                x = x.astype(np.complex64)
                prep = [_prepare(x[g * hop:g * hop + L], sps, M, fc.IQ, B, B, lone=False) for g in range(n_seg)]
                a = analysers(sps, levels=M)
                r = a.process(x, L, hop)
                assert not r.flags.any()
                for g in range(n_seg):
                    _check_stages(prep[g], r.levels[g], r.indices[g], r.records[g], M, (sps, M, L, n_seg, g), worst)
    print(f"sps {sps:g}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


# ---- invariance ---------------------------------------------------------------------------------------------------------------
def test_a_segment_does_not_depend_on_n_seg_its_place_or_the_entry_point(analysers):
    from topdogspectrumanalyser_amd import SpectrumEngine
    sps, L, hop, n_seg = 4.37, 1023, 7, 257
    x, _, _ = fc.make_fsk(4, sps, (n_seg - 1) * hop + L, 0.5, 0.5, seed=5)
    x = x.astype(np.complex64)
    a = analysers(sps, levels=4)
    K = a.symbols_per_segment(L)
    many = a.process(x, L, hop)
    assert len(set(many.records["delta_fx"].tolist())) > 8            # the segments really differ
    for g in (0, 1, 100, 256):
        one = a.process(x[g * hop:g * hop + L], L)
        assert _bits(one.levels[0], many.levels[g]) and _bits(one.indices[0], many.indices[g]), g
        assert one.records[0].tobytes() == many.records[g].tobytes(), g
    few = a.process(x[:2 * hop + L], L, hop)
    assert few.records.tobytes() == many.records[:3].tobytes() and _bits(few.levels, many.levels[:3])
    stride = K + 5
    with SpectrumEngine(64) as eng, DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(4 * n_seg * stride) as d_v, \
            DeviceBuffer(n_seg * stride) as d_i:
        d_x.put(x)
        for engine in (None, eng):
            d_v.put(np.full(n_seg * stride, fk.SENTINEL, dtype=np.float32))
            d_i.put(np.full(n_seg * stride, fk.SENTINEL_INDEX, dtype=np.uint8))
            dev = a.process_device(engine, d_x.ptr, L, hop, n_seg, d_v.ptr, stride, d_i.ptr)
            lev, idx = d_v.get((n_seg, stride), np.float32), d_i.get((n_seg, stride), np.uint8)
            assert dev.levels is None and dev.records.tobytes() == many.records.tobytes()
            assert _bits(lev[:, :K], many.levels) and _bits(idx[:, :K], many.indices)
            assert np.all(lev[:, K:] == fk.SENTINEL) and np.all(idx[:, K:] == fk.SENTINEL_INDEX)
        # without the indices: the same levels and records, and nothing written where they would go
        d_v.put(np.full(n_seg * stride, fk.SENTINEL, dtype=np.float32))
        dev = a.process_device(None, d_x.ptr, L, hop, n_seg, d_v.ptr, stride)
        assert dev.records.tobytes() == many.records.tobytes() and _bits(d_v.get((n_seg, stride), np.float32)[:, :K], many.levels)
    no_idx = a.process(x, L, hop, indices=False)
    assert no_idx.indices is None and _bits(no_idx.levels, many.levels)


def test_behind_the_down_converter_and_the_demodulator_on_an_engine_stream(analysers):
    """capture -> DownConverter(D = 2) -> FskAnalyzer(iq) on the engine's stream, and -> Demodulator(FM, R = 1) ->
    FskAnalyzer(freq), each against the same intermediate data staged through the host."""
    from topdogspectrumanalyser_amd import Demodulator, DownConverter, SpectrumEngine, design_decimator
    sps, L, D = 8, 1023, 2
    n = D * (3 * L + 64)
    x, _, _ = fc.make_fsk(2, sps * D, n, 0.5, 0.5, seed=9)
    x = x.astype(np.complex64)
    a = analysers(sps, levels=2)
    af = analysers(sps, levels=2, input="freq")
    K, Kf = a.symbols_per_segment(L), af.symbols_per_segment(L)
    taps = design_decimator(D)
    lp = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    with SpectrumEngine(64) as eng, DownConverter(D, 1.0, taps=taps) as ddc, DownConverter(D, 1.0, taps=taps) as ddc_h, \
            Demodulator("fm", 1.0, 1, taps=lp) as dem, Demodulator("fm", 1.0, 1, taps=lp) as dem_h:
        y = ddc_h.process(x)
        fm = dem_h.process(y)
        fm = np.asarray(fm, dtype=np.float32).reshape(-1)
        n_seg = (y.size - L) // L + 1
        with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * (y.size + 8)) as d_y, DeviceBuffer(4 * (y.size + 8)) as d_f, \
                DeviceBuffer(4 * n_seg * K) as d_v, DeviceBuffer(n_seg * K) as d_i, DeviceBuffer(4 * n_seg * Kf) as d_vf:
            d_x.put(x)
            ny = ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            dev = a.process_device(eng, d_y.ptr, L, L, n_seg, d_v.ptr, K, d_i.ptr)
            nf = dem.process_device(eng, d_y.ptr, ny, ny, d_f.ptr, ny)
            devf = af.process_device(eng, d_f.ptr, L, L, n_seg, d_vf.ptr, Kf)
            lev, idx = d_v.get((n_seg, K), np.float32), d_i.get((n_seg, K), np.uint8)
            levf = d_vf.get((n_seg, Kf), np.float32)
    assert ny == y.size and nf == fm.size == ny and n_seg == 3
    host = a.process(y, L)
    assert dev.records.tobytes() == host.records.tobytes() and _bits(lev, host.levels) and _bits(idx, host.indices)
    hostf = af.process(fm, L)
    assert devf.records.tobytes() == hostf.records.tobytes() and _bits(levf, hostf.levels)
    assert host.timing_quality.min() > 0.05 and hostf.timing_quality.min() > 0.05 and not host.flags.any() and not hostf.flags.any()


# ---- flags ---------------------------------------------------------------------------------------------------------------------
BAD_IQ = [(complex(np.nan, 0),), (complex(0, np.nan),), (complex(np.inf, 0),), (complex(0, -np.inf),), (complex(3e19, 3e19), complex(3e19, -3e19))]


@pytest.mark.parametrize("bad", BAD_IQ)
def test_a_non_finite_iq_segment_is_flagged_and_its_neighbours_keep_their_bits(analysers, bad):
    """A NaN, an infinity, and two samples whose product overflows, in the middle segment of three."""
    sps, L = 5, 257
    x, _, _ = fc.make_fsk(2, sps, 3 * L, 0.5, 0.5, seed=3)
    x = x.astype(np.complex64)
    a = analysers(sps, levels=2)
    clean = a.process(x, L)
    for at in (L, L + 100, 2 * L - len(bad)):
        y = x.copy()
        y[at:at + len(bad)] = np.array(bad, dtype=np.complex64)
        r = a.process(y, L)
        assert r.flags.tolist() == [0, nat.FSK_NONFINITE, 0], (at, r.flags)
        assert np.isnan(r.levels[1]).all() and not r.indices[1].any()
        zero = np.zeros(1, dtype=fk.RECORD)
        zero["flags"] = nat.FSK_NONFINITE
        assert r.records[1].tobytes() == zero[0].tobytes()
        for g in (0, 2):
            assert _bits(r.levels[g], clean.levels[g]) and _bits(r.indices[g], clean.indices[g])
            assert r.records[g].tobytes() == clean.records[g].tobytes()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e20])
def test_a_non_finite_freq_segment_is_flagged_and_its_neighbours_keep_their_bits(analysers, bad):
    """A NaN, an infinity, and a value whose squared difference overflows, in the middle segment of three."""
    sps, L = 4, 256
    f, _ = fc.make_freq(4, sps, 3 * L, 0.05, 0.01, seed=4, t0=1, bt=0.5)
    f = f.astype(np.float32)
    a = analysers(sps, levels=4, input="freq")
    clean = a.process(f, L)
    for at in (L, L + 100, 2 * L - 1):
        y = f.copy()
        y[at] = np.float32(bad)
        r = a.process(y, L)
        assert r.flags.tolist() == [0, nat.FSK_NONFINITE, 0], (at, r.flags)
        assert np.isnan(r.levels[1]).all() and not r.indices[1].any()
        zero = np.zeros(1, dtype=fk.RECORD)
        zero["flags"] = nat.FSK_NONFINITE
        assert r.records[1].tobytes() == zero[0].tobytes()
        for g in (0, 2):
            assert _bits(r.levels[g], clean.levels[g]) and r.records[g].tobytes() == clean.records[g].tobytes()


def test_constant_and_all_zero_segments(analysers):
    """A constant segment is one level (o = the constant, g = 0, indices 0); an all-zero one is no error either."""
    sps, L = 4, 256
    for M in LEVELS:
        a = analysers(sps, levels=M, input="freq")
        f = np.zeros(3 * L, dtype=np.float32)
        f[L:2 * L] = 0.3
        r = a.process(f, L)
        K = a.symbols_per_segment(L)
        assert r.flags.tolist() == [nat.FSK_ONE_LEVEL] * 3
        assert r.records["offset"].tolist() == [0.0, float(np.float32(0.3)), 0.0] and not r.records["dev"].any()
        assert not r.indices.any() and np.all(r.records["sum_l"] == -K * (M - 1))
        assert not r.records["err_sumsq"].any() and not r.records["err_peak"].any() and not r.records["p"].any()
        assert np.all(r.levels[1] == np.float32(0.3)) and not r.levels[0].any()
        assert not r.fsk_error.any() and not r.timing_quality.any() and not r.deviation.any()
        # t = 0: delta_fx = (L / 2 + sps / 2) mod sps, brought into [1, sps + 1)
        assert np.all(r.records["delta_fx"] == fc.delta_of(0j, fc.step_of(sps), a.lag))
    a = analysers(sps, levels=2)
    r = a.process(np.zeros(3 * L, dtype=np.complex64), L)
    assert r.flags.tolist() == [nat.FSK_ONE_LEVEL] * 3 and not r.levels.any() and not r.records["offset"].any()
    x = np.array([1, 1j, -1, -1j] * (3 * L // 4), dtype=np.complex64)            # a carrier at fs / 4: one level at 1/2, exactly
    r = a.process(x, L)
    assert r.flags.tolist() == [nat.FSK_ONE_LEVEL] * 3 and np.all(r.offset == 0.5) and not r.deviation.any()


# ---- offsets past 2^32 bytes -----------------------------------------------------------------------------------------------------
def test_second_segment_past_4_gib(analysers):
    """Two segments, the second 2^29 + 1 complex samples on: past 2^32 bytes, its levels and indices past 2^32 bytes as
    well.  Only the two segments are uploaded."""
    sps, L, hop = 4.37, 4097, (1 << 29) + 1
    a = analysers(sps, levels=4)
    K = a.symbols_per_segment(L)
    segs = [fc.make_fsk(4, sps, L, 0.5, 0.5, seed=20 + g)[0].astype(np.complex64) for g in range(2)]
    stride = (1 << 32) + 3                                            # uint8 indices past 2^32 bytes too
    with room_or_skip((hop + L) * 8) as d_x, room_or_skip((stride + K) * 4) as d_v, room_or_skip(stride + K) as d_i:
        d_x.put(segs[0])
        d_x.put(segs[1], hop * 8)
        dev = a.process_device(None, d_x.ptr, L, hop, 2, d_v.ptr, stride, d_i.ptr)
        lev = [d_v.get((K,), np.float32, g * stride * 4) for g in range(2)]
        idx = [d_i.get((K,), np.uint8, g * stride) for g in range(2)]
    for g in range(2):
        one = a.process(segs[g], L)
        assert dev.records[g].tobytes() == one.records[0].tobytes(), g
        assert _bits(lev[g], one.levels[0]) and _bits(idx[g], one.indices[0]), g
    assert not _bits(lev[0], lev[1])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_gfsk_burst_through_the_down_converter_matches_the_contract(analysers):
    """A GFSK burst (BT 0.5, h 0.5, 16 samples per symbol at the capture's rate) through DownConverter(D = 2) into the
    analyser.  Deviation, offset and FSK error must each lie within 1 % of the outer deviation of the contract's on the
    same decimated samples."""
    from topdogspectrumanalyser_amd import DownConverter, design_decimator
    sps, D, L, n_seg = 8, 2, 2048, 2
    x, _, _ = fc.make_fsk(2, sps * D, D * (n_seg * L + 64), 0.5, 0.5, seed=31, cfo=0.004, noise_db=-30.0)
    x = x.astype(np.complex64)
    a = analysers(sps, levels=2)
    K = a.symbols_per_segment(L)
    with DownConverter(D, 1.0, taps=design_decimator(D)) as ddc, DownConverter(D, 1.0, taps=design_decimator(D)) as ddc_h:
        y = ddc_h.process(x)
        with DeviceBuffer(x.nbytes) as d_x, DeviceBuffer(8 * (y.size + 8)) as d_y, DeviceBuffer(4 * n_seg * K) as d_v:
            d_x.put(x)
            ny = ddc.process_device(None, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            r = a.process_device(None, d_y.ptr, L, L, n_seg, d_v.ptr, K)
    assert ny == y.size and not r.flags.any()
    for g in range(n_seg):
        want = fc.analyse(y[g * L:(g + 1) * L].astype(np.complex128), sps, 2)
        outer = want["deviation"]
        print(f"segment {g}: deviation {r.deviation[g]:.6f} (contract {outer:.6f}, ratio {r.deviation[g] / outer:.6f}, of nominal "
              f"{r.deviation[g] / (0.5 / sps):.4f}), offset {r.offset[g]:.6f} ({float(want['offset']):.6f}), FSK error "
              f"{r.fsk_error[g]:.5f} ({want['fsk_error']:.5f}), mod index {r.mod_index[g]:.4f}, |C|/P {r.timing_quality[g]:.3f}")
        assert abs(r.deviation[g] - outer) <= 0.01 * outer
        assert abs(r.offset[g] - float(want["offset"])) <= 0.01 * outer
        assert abs(r.fsk_error[g] - want["fsk_error"]) <= 0.01


# ---- the smallest and the largest segments, both kinds, every symbol rate ----------------------------------------------------
def _check_from_the_device(x, rec, lev, idx, sps, M, kind, B, L, what):
    """One segment against the contract with no proof beforehand: C and P within their bound (exactly zero where the
    segment has no differences), delta_fx in its range and, where the line is strong, within its bound; v within its
    bound from the device's delta_fx; everything from v on bit for bit from the device's v."""
    step, nu = fc.step_of(sps), fc.nu_of(sps)
    K = fc.symbols_per_segment(step, x.size, kind, B)
    d = fc.discriminate(x.astype(np.complex128)) if kind == fc.IQ else x.astype(np.float64)
    b = fc.boxcar(d, B)
    eb = fc.boxcar_bound(float(np.abs(d).max()), kind, B)
    C, P, dl = fc.timing(b, nu, step, L)
    dev = int(rec["delta_fx"])
    assert ONE <= dev < step + ONE, what
    if b.size <= L:
        assert (rec["c_re"], rec["c_im"], rec["p"]) == (0, 0, 0) and dev == fc.delta_of(0j, step, L), what
    else:
        e_c = fc.timing_bound(b, L, eb)
        assert max(abs(rec["c_re"] - C.real), abs(rec["c_im"] - C.imag), abs(rec["p"] - P)) <= e_c, what
        if abs(C) >= 0.05 * P and P > 0:
            dd = (dev - dl) % step
            assert min(dd, step - dd) <= fc.delta_bound(C, e_c, step), what
    v, mag, sumc = fc.resample(b, dev, step, K, True)
    bound = fc.resample_bound(mag, sumc, eb)
    assert np.all(np.abs(lev.astype(np.float64) - v) <= bound), (what, float(np.max(np.abs(lev - v) / np.maximum(bound, 1e-300))))
    own = fc.levels(lev, M)
    _same_record(rec, own, what)
    assert np.array_equal(idx, own["indices"]), what


@pytest.mark.parametrize("kind", [fc.IQ, fc.FREQ])
@pytest.mark.parametrize("sps", SPS_ALL)
def test_smallest_and_largest_segments_of_both_kinds_at_every_symbol_rate(sps, kind):
    """Every sps, complex64 and float32 input, every B: the smallest segment with K = 2 (where the last tap of the last
    symbol reads the segment's last sample and, at the larger L, there is no difference at all), 255, 256, 257 differences
    and one past the first two tiles, and for B = 1 and 64 the largest with K = 4096; segments apart and overlapping."""
    biggest = -(-4098 * fc.step_of(sps) // ONE) + 4 + 64 + 8
    x, _, _ = fc.make_fsk(4, sps, biggest, 0.5, None, seed=int(sps * 16) + kind, cfo=0.002, noise_db=-35.0)
    x = x.astype(np.complex64) if kind == fc.IQ else fc.discriminate(x).astype(np.float32)
    n_run = 0
    for nb, B in enumerate(BOXCARS):
        lag, M = LAGS[(nb + 1) % 4], LEVELS[(nb + 1) % 3]
        with fk.FskAnalyzer(sps, M, input=KINDS[kind], boxcar=B, lag=lag) as a:
            for L in seg_lens(sps, kind, B, lag, largest=B in (1, 64)):
                K = a.symbols_per_segment(L)
                for n_seg, hop in [(1, L), (2, L + 3), (3, max(1, L - 7))] if K < 4096 else [(1, L), (2, 5)]:
                    n = (n_seg - 1) * hop + L
                    if n > x.size:
                        continue
                    lev, idx, rec = _run(a, x[:n], L, hop, n_seg, K + 2)
                    n_run += 1
                    assert np.all(lev[:, K:] == fk.SENTINEL) and np.all(idx[:, K:] == fk.SENTINEL_INDEX)
                    assert not (rec["flags"] & nat.FSK_NONFINITE).any()
                    for g in range(n_seg):
                        _check_from_the_device(x[g * hop:g * hop + L], rec[g], lev[g, :K], idx[g, :K], sps, M, kind, B, lag,
                                               (sps, kind, B, lag, M, L, n_seg, hop, g))
    assert n_run >= 60, n_run


@pytest.mark.parametrize("kind", [fc.IQ, fc.FREQ])
@pytest.mark.parametrize("sps", [4, 64])
def test_one_past_every_tile_of_the_timing_stage(sps, kind):
    """Segments whose number of differences is one past every tile of 1024 up to K = 4096, one segment each: 16 tiles at
    4 samples per symbol, 256 at 64 (every eighth of them there, and the last)."""
    B, lag, M = 3, 2, 4
    step = fc.step_of(sps)
    hi = seg_len_of(-(-4098 * step // ONE) - 1 + 4, kind, B)
    x, _, _ = fc.make_fsk(M, sps, hi + 8, 0.5, None, seed=7 + kind, cfo=0.002, noise_db=-35.0)
    x = x.astype(np.complex64) if kind == fc.IQ else fc.discriminate(x).astype(np.float32)
    tiles = [t for t in range(1, 257) if seg_len_of(t * TILE + 1 + lag, kind, B) <= hi]
    assert len(tiles) == (16 if sps == 4 else 256)
    with fk.FskAnalyzer(sps, M, input=KINDS[kind], boxcar=B, lag=lag) as a:
        for t in tiles if sps == 4 else tiles[::8] + tiles[-1:]:
            L = seg_len_of(t * TILE + 1 + lag, kind, B)
            K = a.symbols_per_segment(L)
            lev, idx, rec = _run(a, x[:L], L, L, 1, K)
            _check_from_the_device(x[:L], rec[0], lev[0], idx[0], sps, M, kind, B, lag, (sps, kind, t, L))


def test_a_nan_is_flagged_where_the_segment_has_no_differences(analysers):
    """n_b <= L: P = C = 0 say nothing, and a NaN under a symbol's taps is found among the v_k; one that no tap reads
    changes nothing."""
    sps, L = 4, 16                                              # K = 2, 16 boxcar outputs, lag 64: no difference
    a = analysers(sps, levels=2, input="freq", timing=2.0, boxcar=1, lag=64)
    f = (0.1 * np.random.default_rng(3).standard_normal(3 * L)).astype(np.float32)
    clean = a.process(f, L)
    assert not clean.records["p"].any() and not (clean.flags & nat.FSK_NONFINITE).any()
    for at, seen in ((1, True), (3, True), (8, True), (0, False), (9, False), (15, False)):   # the taps read b[1 .. 8]
        for bad in (np.nan, np.inf):
            y = f.copy()
            y[L + at] = bad
            r = a.process(y, L)
            if seen:
                assert r.flags.tolist() == [clean.flags[0], nat.FSK_NONFINITE, clean.flags[2]], (at, bad)
                zero = np.zeros(1, dtype=fk.RECORD)
                zero["flags"] = nat.FSK_NONFINITE
                assert r.records[1].tobytes() == zero[0].tobytes() and np.isnan(r.levels[1]).all() and not r.indices[1].any()
                want = fc.analyse(y[L:2 * L], sps, 2, fc.FREQ, 1, 64, delta_fx=2 * ONE)
                assert want["flags"] == fc.NONFINITE
            else:
                assert r.records[1].tobytes() == clean.records[1].tobytes() and _bits(r.levels[1], clean.levels[1])
            for g in (0, 2):
                assert r.records[g].tobytes() == clean.records[g].tobytes() and _bits(r.levels[g], clean.levels[g])


# ---- the -1s that need a live handle ---------------------------------------------------------------------------------------------
def test_error_returns_with_a_live_handle():
    import ctypes as C
    lib = nat.lib
    err = lambda: lib.tdsa_last_error_string().decode()                                   # noqa: E731
    P = lambda addr: C.c_void_p(int(addr))                                               # noqa: E731
    x = np.zeros(8192, dtype=np.complex64)
    out = np.zeros(8192, dtype=np.float32)
    idx = np.zeros(8192, dtype=np.uint8)
    rec = np.zeros(64, dtype=fk.RECORD)
    px, po, pi, pr = (v.ctypes.data for v in (x, out, idx, rec))
    assert px % 8 == 0 and po % 4 == 0 and pr % 8 == 0
    raw = C.c_void_p()
    assert lib.tdsa_fsk_create(0, 4096, C.byref(raw)) == 0
    try:
        # no argument is wrong: the state is (TDSA_ERR_STATE, as the symbol recovery answers)
        assert lib.tdsa_fsk_process(raw, P(px), 100, 100, 100, 1, P(po), 64, None, P(pr)) == -3 and "not configured" in err()
        assert lib.tdsa_fsk_process_dev(raw, None, P(px), 100, 100, 1, P(po), 64, None, P(pr)) == -3 and "not configured" in err()
        assert lib.tdsa_fsk_process(raw, None, 100, 100, 100, 1, P(po), 64, None, P(pr)) == -3     # asked before the arguments
    finally:
        assert lib.tdsa_fsk_destroy(raw) == 0
    with fk.FskAnalyzer(4, 2, boxcar=2, max_host_samples=4096) as a, fk.FskAnalyzer(4, 2, input="freq", boxcar=2, max_host_samples=4096) as f, \
            DeviceBuffer(8 * 4096) as d_x, DeviceBuffer(4 * 4096) as d_v, DeviceBuffer(4096) as d_i:
        K = a.symbols_per_segment(100)                                                    # 22
        host = lambda h, **kw: lib.tdsa_fsk_process(h, *[kw.get(k, v) for k, v in (                        # noqa: E731
            ("inp", P(px)), ("n", 1000), ("seg", 100), ("hop", 100), ("n_seg", 2), ("out", P(po)), ("stride", 64), ("idx", P(pi)), ("rec", P(pr)))])
        dev = lambda h, **kw: lib.tdsa_fsk_process_dev(h, None, *[kw.get(k, v) for k, v in (               # noqa: E731
            ("inp", P(d_x.ptr)), ("seg", 100), ("hop", 100), ("n_seg", 2), ("out", P(d_v.ptr)), ("stride", 64), ("idx", P(d_i.ptr)), ("rec", P(pr)))])
        for call in (host, dev):
            for h in (a._h, f._h):
                assert call(h) == 0, err()
                assert call(h, idx=None) == 0, err()                                       # the indices are optional
                assert call(h, inp=None) == -1 and err() == "null samples"
                assert call(h, out=None) == -1 and err() == "null levels"
                assert call(h, rec=None) == -1 and err() == "null records"
                assert call(h, rec=P(pr + 4)) == -1 and "records must be aligned to 8 bytes" in err()
                assert call(h, n_seg=0) == -1 and "n_seg=0" in err()
                assert call(h, n_seg=-1) == -1 and "n_seg=-1" in err()
                assert call(h, hop=0) == -1 and "hop=0" in err()
                assert call(h, stride=K - 1) == -1 and f"out_stride={K - 1}: a segment gives {K} symbols" in err()
                assert call(h, stride=K) == 0, err()
            base_in, base_out = (px, po) if call is host else (d_x.ptr, d_v.ptr)
            assert call(a._h, inp=P(base_in + 4)) == -1 and "complex64 sample (8 bytes)" in err()
            assert call(f._h, inp=P(base_in + 2)) == -1 and "float32 (4 bytes)" in err()
            assert call(f._h, inp=P(base_in + 4)) == 0, err()                              # a float32 stream needs 4 bytes only
            for h in (a._h, f._h):
                assert call(h, out=P(base_out + 2)) == -1 and "output pointer must be aligned to one float32 (4 bytes)" in err()
            # K outside 2 .. 4096: iq has n_b = seg_len - 2, freq n_b = seg_len - 1 at B = 2
            for h, one, two, most in ((a._h, 17, 18, 16394), (f._h, 16, 17, 16393)):
                assert call(h, seg=one, hop=one, n_seg=1) == -1 and f"seg_len={one} gives 1 symbols per segment: 2 .. 4096" in err()
                assert call(h, seg=3, hop=3, n_seg=1) == -1 and "gives -1 symbols" in err()
                assert call(h, seg=most + 4, hop=1, n_seg=1) == -1 and "gives 4097 symbols" in err()
                if call is host:
                    assert call(h, seg=two, hop=two, n_seg=1) == 0, err()
        # the host entry point alone: the block and the staging
        for h in (a._h, f._h):
            assert host(h, n=199) == -1 and "need 200 samples, the block has 199" in err()
            assert host(h, n=99, n_seg=1) == -1 and "the block has 99" in err()
            assert host(h, n=1000, n_seg=3, hop=1 << 63) == -1 and "the block has 1000" in err()      # a product that would wrap
            assert host(h, n=200) == 0, err()
            assert host(h, n=4097, n_seg=1) == -1 and "the handle stages at most 4096 (max_host_samples)" in err()
            assert host(h, n=149, n_seg=50, hop=1) == -1 and "max_host_samples" in err()              # 50 segments of 100 overlap
            assert host(h, n=139, n_seg=40, hop=1) == 0, err()
        n_dev = C.c_int()
        assert lib.tdsa_device_count(C.byref(n_dev)) == 0
        if n_dev.value > 1:                                                                # a plan on another device
            from topdogspectrumanalyser_amd import SpectrumEngine
            with SpectrumEngine(64, device=1) as eng:
                assert lib.tdsa_fsk_process_dev(a._h, eng._h, P(d_x.ptr), 100, 100, 2, P(d_v.ptr), 64, None, P(pr)) == -1
                assert "different devices" in err()
        assert lib.tdsa_fsk_timer_end(a._h, None) == -1 and err() == "null elapsed_ms"
        a.timer_begin()
        assert dev(a._h) == 0 and a.timer_end() >= 0.0
