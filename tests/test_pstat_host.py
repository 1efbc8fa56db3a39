"""The power statistics without a device: the contract (tests/pstat_contract.py) on constructed input, the analysis in
powerstats.py on states the contract makes, the record layout, and every argument error that needs no handle."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import pstat_contract as pc
from topdogspectrumanalyser_amd import PowerStatistics, PowerStats, gaussian_ccdf
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import powerstats as ps

f32 = np.float32
N_NOISE = 1 << 20


def _stats(states, exp_lo=-40, gate=0.0):
    return PowerStatistics(*pc.stack(states), exp_lo, gate)


def _partition(st):
    r = st.rec
    return int(r["n_total"]) == sum(int(r[f]) for f in pc.COUNTS[1:]) + int(st.hist.sum())


@pytest.fixture(scope="module")
def noise():
    """Seeded complex Gaussian noise, mean power 0.02, its float32 powers and its state."""
    rng = np.random.default_rng(20)
    x = ((rng.standard_normal(N_NOISE) + 1j * rng.standard_normal(N_NOISE)) * 0.1).astype(np.complex64)
    return x, pc.power(*pc.unpack(x, pc.C64)), pc.State().accumulate(x, pc.C64)


# ---- the contract on constructed input ---------------------------------------------------------------------------
def test_the_classes_partition_the_samples(noise):
    assert _partition(noise[2]) and int(noise[2].rec["n_total"]) == N_NOISE
    x, _ = pc.specials()
    for gate in (0.0, 1.0):
        for exp_lo in (-126, -40, 64):
            assert _partition(pc.State().accumulate(np.concatenate([x, noise[0][:1000]]), pc.C64, exp_lo, gate))


def test_every_special_sample_falls_in_its_class():
    x, cls = pc.specials()
    for v, want in zip(x, cls):
        st = pc.State().accumulate(np.array([v]), pc.C64)
        got = [f for f in pc.COUNTS[1:] if int(st.rec[f])]
        assert got == [want] and int(st.hist.sum()) == 0, (v, got, want)
    st = pc.State().accumulate(x, pc.C64)
    assert {f: int(st.rec[f]) for f in pc.COUNTS} == dict(n_total=12, n_nan=3, n_gated=0, n_inf=3, n_zero=2, n_under=1, n_over=3)
    # the denormal power is kept, not flushed: 2^-140 = 2^9 2^-149 in msum[0]; 2^26 and the two large ones by their octaves
    assert int(st.msum[0]) == 1 << 9 and int(st.msum[127 + 26]) == 1 << 23
    assert int(st.rec["min_bits"]) == 1 << 9 and int(st.rec["max_bits"]) == int(f32(f32(1e19) * f32(1e19) * 2).view(np.uint32))
    assert pc.total_power(st.msum) == Fraction(1, 2 ** 140) + 2 ** 26 + 3 * int(f32(1e19) * f32(1e19))


def test_the_gate_takes_what_is_below_it_and_nothing_else():
    x = np.array([0, 0.5, 1.0, 2.0, np.nan, np.inf], dtype=np.complex64)            # p = 0, 0.25, 1, 4, NaN, inf
    st = pc.State().accumulate(x, pc.C64, gate=1.0)
    assert {f: int(st.rec[f]) for f in pc.COUNTS} == dict(n_total=6, n_nan=1, n_gated=2, n_inf=1, n_zero=0, n_under=0, n_over=0)
    assert int(st.hist.sum()) == 2 and st.rec["min_bits"] == f32(1).view(np.uint32) and st.rec["max_bits"] == f32(4).view(np.uint32)
    assert pc.total_power(st.msum) == 5
    off = pc.State().accumulate(x, pc.C64, gate=0.0)
    assert int(off.rec["n_gated"]) == 0 and int(off.rec["n_zero"]) == 1 and int(off.hist.sum()) == 3


@pytest.mark.parametrize("exp_lo", (-126, -40, -39, 0, 64))
def test_exact_edges_fall_in_their_bins_and_one_float_below_in_the_bin_below(exp_lo):
    x, bins = pc.edge_set(exp_lo)
    assert x.size >= 64
    edges = pc.edges(exp_lo)
    for v, b in zip(x, bins):
        st = pc.State().accumulate(np.array([v]), pc.C64, exp_lo)
        assert int(st.hist[b]) == 1 and int(st.hist.sum()) == 1, (v, b)
    p = pc.power(*pc.unpack(x, pc.C64)).astype(np.float64)
    at_edge = bins % 32 != 31
    assert np.array_equal(p[at_edge], edges[bins[at_edge]])                         # the constructed powers ARE the edges
    assert np.array_equal(p[~at_edge], np.nextafter(edges[bins[~at_edge] + 1].astype(f32), f32(0)).astype(np.float64))
    # every edge of the window, and the float32 below it, from the powers themselves
    e32 = edges[:-1].astype(f32)
    assert np.array_equal(e32.astype(np.float64), edges[:-1])                       # exact float32
    st = pc.State().accumulate_power(e32, exp_lo)
    assert np.array_equal(st.hist, np.ones(pc.BINS, dtype=np.uint64))
    below = pc.State().accumulate_power(np.nextafter(e32, f32(0)), exp_lo)
    want = np.ones(pc.BINS, dtype=np.uint64)
    want[-1] = 0
    assert np.array_equal(below.hist, want) and int(below.rec["n_under"]) + int(below.rec["n_zero"]) == 1


def test_int8_and_uint8_unpack_as_the_streaming_filters_do():
    b = np.array([-128, 127, 0, 1], dtype=np.int8)
    re, im = pc.unpack(b, pc.I8)
    assert re.tolist() == [-1.0, 0.0] and im.tolist() == [127 / 128, 1 / 128]
    u = np.arange(256, dtype=np.uint8).repeat(2)
    re, im = pc.unpack(u, pc.U8)
    assert np.array_equal(re, (np.arange(256) / 127.5 - 1.0).astype(f32)) and np.array_equal(re, im)


# ---- the analysis ------------------------------------------------------------------------------------------------
def test_the_exact_mean_agrees_with_a_float64_sum(noise):
    _, p, st = noise
    s = _stats([st])
    ref = float(p.astype(np.float64).sum()) / N_NOISE
    rel = abs(s.mean_power[0] - ref) / ref
    print(f"mean {s.mean_power[0]!r} float64 sum {ref!r} rel {rel:.2e}")
    assert rel <= 1e-15
    assert s.mean_power[0] == pc.mean_power(st.rec, st.msum) == float(s.total_power(0) / N_NOISE)
    assert s.peak_power[0] == float(p.max()) and s.min_power[0] == float(p.min()) and s.counted[0] == N_NOISE


def test_noise_follows_the_gaussian_reference_curve(noise):
    s = _stats([noise[2]])
    x_db, prob = s.ccdf_curve(0)
    assert np.array_equal(prob, pc.ccdf_at_edges(noise[2].rec, noise[2].hist))
    for db in (0.0, 3.0, 6.0, 9.0):
        k = int(np.argmin(np.abs(x_db - db)))
        q = float(gaussian_ccdf(x_db[k]))
        sigma = math.sqrt(q * (1.0 - q) / N_NOISE)
        print(f"{db} dB: edge {x_db[k]:.4f} dB, ccdf {prob[k]:.6e}, reference {q:.6e}, {(prob[k] - q) / sigma:+.2f} sigma")
        assert abs(prob[k] - q) <= 6.0 * sigma
        assert s.ccdf(x_db[k]) == prob[k]
    assert abs(s.papr_db[0] - 10 * math.log10(math.log(N_NOISE))) < 2.0          # the largest of n exponentials: ~ ln n


def test_ccdf_is_the_exact_tail_count_and_level_db_inverts_it_at_edges(noise):
    _, p, st = noise
    s = _stats([st])
    edges = s.edges()
    x_db, prob = s.ccdf_curve(0)
    x_abs, prob_abs = s.ccdf_curve(0, relative=False)
    assert np.array_equal(prob, prob_abs) and np.array_equal(x_abs, 10 * np.log10(edges))
    live = np.flatnonzero(st.hist > 0)
    for k in live[[0, 1, len(live) // 3, len(live) // 2, -2, -1]]:
        assert prob[k] == np.count_nonzero(p.astype(np.float64) >= edges[k]) / N_NOISE
        if st.hist[k - 1] > 0:                                                     # strictly falling on both sides
            assert s.level_db(prob[k]) == x_db[k] and s.ccdf(s.level_db(prob[k])) == prob[k]
            assert s.level_db(prob[k], relative=False) == x_abs[k]
    mid = 0.5 * (x_db[live[5]] + x_db[live[5] + 1])
    assert prob[live[5] + 1] < s.ccdf(mid) < prob[live[5]]                         # linear between edges
    assert np.isnan(s.ccdf(x_db[0] - 1.0)) and np.isnan(s.ccdf(x_db[-1] + 1.0)) and np.isnan(s.level_db(1.5))
    lv = s.level_db([0.1, 0.01, 0.001])
    assert np.allclose(lv, 10 * np.log10(-np.log([0.1, 0.01, 0.001])), atol=0.3)


def test_papr_of_a_cw_is_0_db():
    n = np.arange(4096)
    cw = (0.5 * np.exp(2j * np.pi * 0.25 * n)).astype(np.complex64)                 # 0.5 (1, j, -1, -j): p = 0.25 exactly
    s = _stats([pc.State().accumulate(cw, pc.C64)])
    assert s.papr_db[0] == 0.0 and s.mean_power[0] == 0.25 and np.count_nonzero(s.hist[0]) == 1
    tone = (0.3 * np.exp(2j * np.pi * 0.01234 * n)).astype(np.complex64)            # rounding spreads it over a few ulps
    assert abs(_stats([pc.State().accumulate(tone, pc.C64)]).papr_db[0]) < 1e-5


def test_infinite_and_empty_streams_have_defined_answers():
    s = _stats([pc.State().accumulate(np.array([1, np.inf], dtype=np.complex64), pc.C64), pc.State(),
                pc.State().accumulate(np.array([0, 0], dtype=np.complex64), pc.C64)])
    assert s.mean_power[0] == np.inf and s.peak_power[0] == np.inf and s.min_power[0] == 1.0
    assert np.isnan(s.mean_power[1]) and np.isnan(s.peak_power[1]) and np.isnan(s.ccdf_at_edges(1)).all()
    assert s.mean_power[2] == 0.0 and s.peak_power[2] == 0.0 and s.min_power[2] == 0.0
    assert len(s) == 3 and s.n_total.tolist() == [2, 0, 2]


def test_a_shift_by_the_exponent_needs_python_integers():
    m = np.zeros(pc.EXPONENTS, dtype=np.uint64)
    m[200] = 1 << 23                                                               # one sample of power 2^73
    assert pc.total_power(m) == 2 ** 73
    st = pc.State()
    st.msum, st.rec["n_total"] = m, 1
    assert _stats([st]).mean_power[0] == 2.0 ** 73


# ---- layout and argument errors ----------------------------------------------------------------------------------
def test_record_layout():
    assert ps.RECORD.itemsize == pc.RECORD.itemsize == C.sizeof(nat.PstatRecord) == 72
    for f in pc.COUNTS + ("max_bits", "min_bits", "reserved"):
        assert ps.RECORD.fields[f][1] == pc.RECORD.fields[f][1] == getattr(nat.PstatRecord, f).offset, f
    assert ps.RECORD.names[:7] == pc.COUNTS and ps.RECORD.fields["max_bits"][1] == 56 and ps.RECORD.fields["min_bits"][1] == 60
    assert (ps.BINS, ps.BINS_PER_OCTAVE, ps.EXPONENTS) == (pc.BINS, pc.BINS_PER_OCTAVE, pc.EXPONENTS)
    assert np.array_equal(ps.bin_edges(-40), pc.edges(-40))
    w = 10 * np.log10(pc.edges(0)[1:33] / pc.edges(0)[:32])
    assert 0.068 < w.min() < 0.069 and 0.133 < w.max() < 0.134


@pytest.mark.parametrize("kw", [dict(streams=0), dict(streams=257), dict(exp_lo=-127), dict(exp_lo=65), dict(exp_lo=1.5),
                                dict(exp_lo="x"), dict(gate=-1.0), dict(gate=float("nan")), dict(gate=float("inf")),
                                dict(gate=1e39), dict(streams=4, max_host_samples=3)])
def test_the_constructor_refuses_before_the_library_is_called(kw, monkeypatch):
    monkeypatch.setattr(nat.lib, "tdsa_pstat_create", lambda *a: pytest.fail("the library was called"))
    with pytest.raises(ValueError):
        PowerStats(**kw)


def _bare(streams=1):
    """A PowerStats that never reached the library, for the checks that come before it."""
    p = PowerStats.__new__(PowerStats)
    p.streams, p.device, p.max_host_samples, p.exp_lo, p.gate, p._h = streams, 0, 1 << 20, -40, 0.0, None
    return p


def test_calls_refuse_before_the_library_is_called(monkeypatch):
    for name in ("tdsa_pstat_process", "tdsa_pstat_process_dev", "tdsa_pstat_read", "tdsa_pstat_configure"):
        monkeypatch.setattr(nat.lib, name, lambda *a: pytest.fail("the library was called"))
    one, three = _bare(1), _bare(3)
    for bad in (np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.int16), np.zeros(7, dtype=np.int8),
                np.zeros((2, 8), dtype=np.complex64), np.zeros((1, 2, 8), dtype=np.complex64)):
        with pytest.raises(ValueError):
            one.process(bad)
    with pytest.raises(ValueError):
        three.process(np.zeros(8, dtype=np.complex64))
    for args in ((0, 8), (4096, -1), (4097, 8), (4100, 8, None, nat.IN_C64), (4096, 8, None, 3), (4096, 8, None, -1)):
        with pytest.raises(ValueError):
            one.process_device(None, *args)
    with pytest.raises(ValueError):
        three.process_device(None, 4096, 8, 7)
    for bad in (-1, 3, range(2, 4), range(0, 3, 2), range(0)):
        with pytest.raises(ValueError):
            three.read(bad)
    for kw in (dict(exp_lo=-127), dict(gate=-0.5), dict(gate=float("inf"))):
        with pytest.raises(ValueError):
            one.configure(**kw)


def test_argument_errors_that_need_no_handle_return_minus_1():
    lib, h = nat.lib, C.c_void_p()
    err = lambda: lib.tdsa_last_error_string().decode()
    for streams in (0, -1, 257):
        assert lib.tdsa_pstat_create(0, streams, 1024, C.byref(h)) == -1 and "streams" in err() and not h
    assert lib.tdsa_pstat_create(0, 1, 1024, None) == -1 and "null" in err()
    assert lib.tdsa_pstat_create(0, 4, 3, C.byref(h)) == -1 and "max_host_samples" in err()
    for e in (-127, 65):
        assert lib.tdsa_pstat_configure(None, e, 0.0) == -1 and "exp_lo" in err()
    for g in (-1.0, float("nan"), float("inf")):
        assert lib.tdsa_pstat_configure(None, -40, g) == -1 and "gate" in err()
    assert lib.tdsa_pstat_configure(None, -40, 0.0) == -1 and "null" in err()
    buf = (C.c_byte * 64)()
    for fmt in (-1, 3, 7):
        assert lib.tdsa_pstat_process(None, fmt, buf, 4, 4) == -1 and "in_format" in err()
        assert lib.tdsa_pstat_process_dev(None, None, fmt, buf, 4, 4) == -1 and "in_format" in err()
    assert lib.tdsa_pstat_process_dev(None, None, nat.IN_C64, C.c_void_p(4100), 4, 4) == -1 and "aligned" in err()
    assert lib.tdsa_pstat_process_dev(None, None, nat.IN_I8, C.c_void_p(4097), 4, 4) == -1 and "aligned" in err()
    assert lib.tdsa_pstat_process(None, nat.IN_I8, buf, 4, 4) == -1 and "null" in err()
    assert lib.tdsa_pstat_process_dev(None, None, nat.IN_U8, C.c_void_p(4096), 4, 4) == -1 and "null" in err()
    assert lib.tdsa_pstat_read(None, 0, 1, None, None, None) == -1 and "null records" in err()
    assert lib.tdsa_pstat_read(None, 0, 1, buf, None, None) == -1 and "null" in err()
    assert lib.tdsa_pstat_reset(None) == -1 and lib.tdsa_pstat_timer_begin(None) == -1 and lib.tdsa_pstat_timer_end(None, None) == -1
    assert lib.tdsa_pstat_destroy(None) == 0
