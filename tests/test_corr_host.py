"""The correlation search without a device: the contract (tests/corr_contract.py) on constructed input, Matches and the
reference makers of correlate.py, the record and summary layouts, and every argument error that needs no handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corr_contract as cc
from topdogspectrumanalyser_amd import Correlator, Matches, barker, from_symbols, rrc_taps, zadoff_chu
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import correlate as co

f32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdsa_hip.h")


def _matches_of(stream):
    rec, s = stream.result()
    return Matches(rec, s, stream.L, float(cc.reference_energy(stream.r)))


def _planted(r, at, n, amp=1.0, noise=0.0, seed=0, freq=0.0, phase=0.0):
    """n complex64 samples: noise of the given standard deviation per component, r planted at every index of `at`."""
    rng = np.random.default_rng(seed)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    k = np.arange(len(r))
    for a in at:
        x[a:a + len(r)] += amp * np.asarray(r, dtype=np.complex128) * np.exp(1j * (2 * np.pi * freq * k + phase))
    return x.astype(np.complex64)


# ---- the match rule ----------------------------------------------------------------------------------------------
def test_a_metric_exactly_at_the_threshold_matches_and_the_float32_below_it_does_not():
    thr = f32(0.3)
    below = np.nextafter(thr, f32(0))
    m = np.array([0, thr, 0, 0, 0, below, 0, 0], dtype=f32)
    assert cc.matches(m, thr, 2).tolist() == [1]
    assert cc.matches(m, below, 2).tolist() == [1, 5]
    assert cc.decide(m.astype(np.float64), np.zeros(8), thr, 2).tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


def test_of_equal_maxima_inside_w_the_first_wins_and_w_plus_1_apart_both_win():
    for W in (1, 2, 5):
        m = np.zeros(40, dtype=f32)
        m[10] = m[10 + W] = 0.5                      # inside W of each other
        m[25] = m[25 + W + 1] = 0.5                  # W + 1 apart
        assert cc.matches(m, 0.25, W).tolist() == [10, 25, 25 + W + 1], W
        m[10 + W] = np.nextafter(f32(0.5), f32(1))  # the later one larger: it wins alone
        assert cc.matches(m, 0.25, W).tolist() == [10 + W, 25, 25 + W + 1], W


def test_a_window_below_w_has_its_left_range_clipped_at_the_first_window():
    m = np.array([0.2, 0.6, 0.1, 0.1, 0.1, 0.1, 0.7, 0.1], dtype=f32)
    assert cc.matches(m, 0.5, 4).tolist() == [1, 6]  # window 1 has one window to its left, and 0.7 lies W + 1 behind it
    assert cc.matches(m, 0.5, 5).tolist() == [6]     # 0.7 within W of 0.6 beats it; its own left range starts at window 1
    assert cc.matches(m, 0.5, 100).tolist() == [6]
    assert cc.matches(m[:6], 0.5, 100).tolist() == [1]
    assert cc.matches(np.array([0.9], dtype=f32), 0.5, 7).tolist() == [0]


def test_the_last_w_windows_stay_undecided_until_a_second_block_brings_their_neighbours():
    r = zadoff_chu(16)
    x = _planted(r, [20, 70], 120)
    W = 30
    s = cc.Stream(r, 0.5, W).feed(x[:95])            # windows 0 .. 79, decided 0 .. 49: the peak at 70 waits
    t = _matches_of(s)
    assert t.index.tolist() == [20] and t.n_windows == 80 and t.n_decided == 50 and t.n_matches == 1 and not t.flushed
    s.feed(x[95:])
    t = _matches_of(s)
    assert t.index.tolist() == [20, 70] and t.n_windows == 105 and t.n_decided == 75 and t.n_total == 120
    whole = cc.Stream(r, 0.5, W).feed(x).result()
    assert np.array_equal(whole[0], s.result()[0]) and whole[1] == s.result()[1]


def test_flush_decides_the_tail_with_the_right_range_clipped_and_ends_the_stream():
    r = zadoff_chu(16)
    x = _planted(r, [20, 70], 95)
    s = cc.Stream(r, 0.5, 30).feed(x)
    assert _matches_of(s).index.tolist() == [20]
    s.flush()
    t = _matches_of(s)
    assert t.index.tolist() == [20, 70] and t.n_decided == t.n_windows == 80 and t.flushed
    with pytest.raises(RuntimeError):
        s.feed(x)
    # no window at all: a flush of L - 1 samples decides nothing
    t = _matches_of(cc.Stream(r, 0.5).feed(x[:15]).flush())
    assert len(t) == 0 and t.n_windows == 0 and t.n_decided == 0 and t.n_total == 15 and t.flushed


def test_windows_of_zeros_nan_and_inf_have_metric_0_count_as_bad_and_never_match():
    r = barker(5)
    x = _planted(r, [30], 60, noise=0.01)
    x[:10] = 0                                        # windows 0 .. 5: e = 0
    x[45] = complex(np.nan, 0)
    x[55] = complex(0, -np.inf)
    w = cc.Windows(x.astype(np.complex128), r)
    bad = np.zeros(56, dtype=bool)
    bad[0:6] = bad[41:46] = bad[51:56] = True
    assert np.array_equal(w.bad, bad) and not w.m[bad].any() and not w.b_m[bad].any()
    rec, s = cc.Stream(r, 0.01, 3).feed(x).flush().result()
    assert s["n_bad"] == 16 and 30 in rec["index"] and not set(rec["index"]) & set(np.flatnonzero(bad))
    # a square that float32 cannot hold: the energy is not finite
    x[50] = complex(3e38, 0)
    assert cc.Windows(x.astype(np.complex128), r).bad[46:51].all()


def test_matches_beyond_the_capacity_are_counted_and_nothing_is_overwritten():
    r = barker(7)
    at = list(range(5, 200, 20))
    x = _planted(r, at, 220)
    for capacity in (1, 3, 10, 11):
        t = _matches_of(cc.Stream(r, 0.9, 7, capacity).feed(x).flush())
        assert t.index.tolist() == at[:capacity] and t.n_matches == 10 and t.n_lost == max(0, 10 - capacity)


# ---- Matches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (16, 63, 64, 255, 1024))
def test_freq_of_a_reference_planted_with_a_carrier_offset(L):
    r = zadoff_chu(L)
    f = 1.0 / (8 * L)
    for sign in (1, -1):
        x = _planted(r, [40], 3 * L + 100, amp=0.5, freq=sign * f, phase=0.7)
        t = _matches_of(cc.Stream(r, 0.5).feed(x).flush())
        assert t.index.tolist() == [40]
        assert abs(t.freq[0] - sign * f) <= 1e-4 / L


def test_gain_phase_and_snr_of_a_reference_at_a_known_amplitude_in_noise():
    L, amp, phase, sigma = 1024, 0.5, -1.1, 0.1      # noise power 2 sigma^2 = 0.02, signal power 0.25: 10.97 dB
    r = zadoff_chu(1021)
    r = np.concatenate([r, r[:3]])
    x = _planted(r, [333], 3000, amp=amp, noise=sigma, seed=5, phase=phase)
    t = _matches_of(cc.Stream(r, 0.5).feed(x).flush())
    assert t.index.tolist() == [333] and t.to_seconds(1e3).tolist() == [0.333]
    want = amp * np.exp(1j * phase)
    # c / E_r = the amplitude + noise of standard deviation sigma / sqrt(L) per component: five of them
    assert abs(t.gain[0] - want) <= 5 * np.sqrt(2) * sigma / np.sqrt(L)
    assert abs(t.phase[0] - phase) <= 5 * sigma / np.sqrt(L) / amp
    assert np.allclose(t.c, t.c1 + t.c2) and np.array_equal(t.gain, t.c / t.e_ref)
    # m / (1 - m) estimates amp^2 / (2 sigma^2) from L samples: its relative error is of the order sqrt(2 / L) = 4.4 %, 0.2 dB
    assert abs(t.snr_db[0] - 10 * np.log10(amp ** 2 / (2 * sigma ** 2))) <= 1.0


@pytest.mark.parametrize("L, root", [(13, 1), (61, 7), (251, 25), (1021, 3), (64, 1), (63, 2)])
def test_zadoff_chu_has_constant_amplitude_and_no_periodic_autocorrelation_off_the_peak(L, root):
    z = zadoff_chu(L, root)
    assert z.dtype == np.complex64 and z.shape == (L,)
    assert np.abs(np.abs(z.astype(np.complex128)) - 1.0).max() <= 2 * cc.U
    acf = np.fft.ifft(np.fft.fft(z.astype(np.complex128)) * np.conj(np.fft.fft(z.astype(np.complex128))))
    assert abs(acf[0] - L) <= 1e-4 and np.abs(acf[1:]).max() <= 1e-4 * np.sqrt(L)       # float32 samples: 6e-8 each


def test_barker_13_and_the_other_lengths():
    b = barker(13)
    assert b.dtype == np.complex64 and b.real.tolist() == [1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1] and not b.imag.any()
    for n in (2, 3, 4, 5, 7, 11, 13):
        acf = np.correlate(barker(n).real, barker(n).real, mode="full")
        assert acf[n - 1] == n and np.abs(np.delete(acf, n - 1)).max() <= 1
    for bad in (1, 6, 14):
        with pytest.raises(ValueError):
            barker(bad)


def test_from_symbols_holds_or_shapes_and_has_unit_mean_power():
    sym = np.array([1, -1, 1j, -1j], dtype=np.complex64)
    held = from_symbols(sym, 4)
    assert held.dtype == np.complex64 and held.shape == (16,) and np.array_equal(held[4:8], np.full(4, -1, dtype=np.complex64))
    taps = rrc_taps(4)
    shaped = from_symbols(sym, 4, taps)
    assert shaped.shape == (16 + taps.size - 1,) and abs(np.mean(np.abs(shaped.astype(np.complex128)) ** 2) - 1) <= 1e-6
    want = np.convolve(np.kron(sym.astype(np.complex128), [1, 0, 0, 0]), taps.astype(np.float64))
    assert np.allclose(shaped, want / np.sqrt(np.mean(np.abs(want) ** 2)), atol=1e-6)
    for args in ((sym, 0), (np.zeros(0), 4)):
        with pytest.raises(ValueError):
            from_symbols(*args)
    for args in ((1, 1), (13, 0), (13, 13), (12, 4), (12, -1)):
        with pytest.raises(ValueError):
            zadoff_chu(*args)


# ---- layout and argument errors ----------------------------------------------------------------------------------
def _header_fields(struct):
    txt = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, names in re.findall(r"(\w+)\s+([^;]+);", body):
        out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_record_and_summary_layouts():
    ctypes_of = {"int64_t": np.int64, "uint64_t": np.uint64, "int32_t": np.int32, "float": np.float32}
    for struct, dtype, cdef, size in (("tdsa_corr_record", co.RECORD, nat.CorrRecord, 32),
                                      ("tdsa_corr_summary", co.SUMMARY, nat.CorrSummary, 56)):
        fields = _header_fields(struct)
        assert [n for n, _ in fields] == list(dtype.names)
        off = 0
        for name, ctype in fields:                       # the header's order, naturally aligned, no padding
            assert dtype.fields[name][0] == np.dtype(ctypes_of[ctype]) and dtype.fields[name][1] == off == getattr(cdef, name).offset, name
            off += np.dtype(ctypes_of[ctype]).itemsize
        assert off == size == dtype.itemsize == C.sizeof(cdef)
    assert co.RECORD == cc.RECORD and co.SUMMARY == cc.SUMMARY and co.COUNTS == cc.COUNTS
    hpp = open(os.path.join(os.path.dirname(co.__file__), "csrc", "tdsa_corr.hpp")).read()
    assert "static_assert(sizeof(CorrRecord) == 32" in hpp and "static_assert(sizeof(CorrSummary) == 56" in hpp


REF = zadoff_chu(16)
BAD_REFS = (np.zeros(1, dtype=np.complex64), np.zeros(1025, dtype=np.complex64), np.zeros(16, dtype=np.complex64),
            np.zeros((2, 8), dtype=np.complex64), np.array([1, np.nan], dtype=np.complex64), np.array([1, complex(0, np.inf)]),
            np.array([1e30, 1e30], dtype=np.complex64), np.array(["a", "b"]), np.array([1e300, 1.0]))


@pytest.mark.parametrize("kw", [dict(streams=0), dict(streams=257), dict(capacity=0), dict(capacity=-1), dict(streams=2, capacity=(1 << 21) + 1),
                                dict(capacity=(1 << 22) + 1), dict(streams=4, max_host_samples=3), dict(trace=-1), dict(trace=1.5)]
                         + [dict(reference=r) for r in BAD_REFS])
def test_the_constructor_refuses_before_the_library_is_called(kw, monkeypatch):
    monkeypatch.setattr(nat.lib, "tdsa_corr_create", lambda *a: pytest.fail("the library was called"))
    kw.setdefault("reference", REF)
    with pytest.raises(ValueError):
        Correlator(**kw)


def _bare(streams=1):
    """A Correlator that never reached the library, for the checks that come before it."""
    p = Correlator.__new__(Correlator)
    p.streams, p.capacity, p.device, p.max_host_samples, p._h, p.reference, p.trace = streams, 16, 0, 1 << 20, None, REF, 0
    return p


def test_calls_refuse_before_the_library_is_called(monkeypatch):
    for name in ("tdsa_corr_process", "tdsa_corr_process_dev", "tdsa_corr_read", "tdsa_corr_read_trace", "tdsa_corr_configure",
                 "tdsa_corr_set_reference"):
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
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            three.read(bad)
        with pytest.raises(ValueError):
            three.read_trace(bad, 0, 1)
    for args in ((0, -1, 1), (0, 0, -1)):
        with pytest.raises(ValueError):
            one.read_trace(*args)
    for args in ((0.0,), (-0.5,), (1.5,), (float("nan"),), (float("inf"),), (1e-50,), (0.5, 0), (0.5, -1), (0.5, 65537), (0.5, 1.5),
                 (0.5, "x")):
        with pytest.raises(ValueError):
            one.configure(*args)
    for bad in BAD_REFS:
        with pytest.raises(ValueError):
            one.set_reference(bad)


def test_argument_errors_that_need_no_handle_return_minus_1():
    lib, h = nat.lib, C.c_void_p()
    err = lambda: lib.tdsa_last_error_string().decode()
    ref = REF.ctypes.data_as(C.c_void_p)
    create = lambda *a: lib.tdsa_corr_create(*a, C.byref(h))
    for streams in (0, -1, 257):
        assert create(0, streams, 16, 0, 1024, ref, 16) == -1 and "streams" in err() and not h
    for streams, capacity in ((1, 0), (1, -5), (1, (1 << 22) + 1), (256, (1 << 14) + 1)):
        assert create(0, streams, capacity, 0, 1024, ref, 16) == -1 and "capacity" in err() and not h
    assert create(0, 1, 16, -1, 1024, ref, 16) == -1 and err() == "trace=-1: not negative"
    assert create(0, 4, 16, 0, 3, ref, 16) == -1 and "max_host_samples" in err()
    for n in (1, 0, -3, 1025):
        assert create(0, 1, 16, 0, 1024, ref, n) == -1 and err() == f"ref_len={n}: 2 .. 1024"
        assert lib.tdsa_corr_set_reference(None, ref, n) == -1 and err() == f"ref_len={n}: 2 .. 1024"
    assert create(0, 1, 16, 0, 1024, None, 16) == -1 and err() == "null reference"
    nan = np.array([1, 2, complex(0, np.nan), 3], dtype=np.complex64)
    assert create(0, 1, 16, 0, 1024, nan.ctypes.data_as(C.c_void_p), 4) == -1 and err() == "reference sample 2 is not finite"
    zero = np.zeros(4, dtype=np.complex64)
    assert create(0, 1, 16, 0, 1024, zero.ctypes.data_as(C.c_void_p), 4) == -1 and "reference energy" in err() and not h
    huge = np.full(4, 1e30, dtype=np.complex64)
    assert lib.tdsa_corr_set_reference(None, huge.ctypes.data_as(C.c_void_p), 4) == -1 and "reference energy" in err()
    assert lib.tdsa_corr_create(0, 1, 16, 0, 1024, ref, 16, None) == -1 and err() == "null out"
    assert lib.tdsa_corr_set_reference(None, ref, 16) == -1 and err() == "null correlator"
    for thr in (0.0, -1.0, 1.5, float("nan")):
        assert lib.tdsa_corr_configure(None, thr, 16) == -1 and "threshold" in err()
    for w in (0, -1, 65537):
        assert lib.tdsa_corr_configure(None, 0.5, w) == -1 and err() == f"min_distance={w}: 1 .. 65536"
    assert lib.tdsa_corr_configure(None, 0.5, 16) == -1 and err() == "null correlator"
    buf = (C.c_byte * 64)()
    for fmt in (-1, 3, 7):
        text = f"in_format={fmt}: the correlation search takes complex IQ (TDSA_IN_I8 / _U8 / _C64)"
        assert lib.tdsa_corr_process(None, fmt, buf, 4, 4) == -1 and err() == text
        assert lib.tdsa_corr_process_dev(None, None, fmt, buf, 4, 4) == -1 and err() == text
    assert lib.tdsa_corr_process_dev(None, None, nat.IN_C64, C.c_void_p(4100), 4, 4) == -1 and err() == "input pointer must be aligned to one sample (8 bytes)"
    assert lib.tdsa_corr_process_dev(None, None, nat.IN_I8, C.c_void_p(4097), 4, 4) == -1 and err() == "input pointer must be aligned to one sample (2 bytes)"
    assert lib.tdsa_corr_process(None, nat.IN_I8, C.c_void_p(4097), 4, 4) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_process_dev(None, None, nat.IN_U8, C.c_void_p(4096), 4, 4) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_read(None, 0, 1, buf, None) == -1 and err() == "null summaries"
    assert lib.tdsa_corr_read(None, 0, 1, None, buf) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_read_trace(None, 0, -1, 1, buf, buf) == -1 and err() == "first=-1, count=1: not negative"
    assert lib.tdsa_corr_read_trace(None, 0, 0, 1, None, buf) == -1 and err() == "null m_out"
    assert lib.tdsa_corr_read_trace(None, 0, 0, 1, buf, None) == -1 and err() == "null correlator"
    for call in (lib.tdsa_corr_flush, lib.tdsa_corr_reset, lib.tdsa_corr_timer_begin):
        assert call(None) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_timer_end(None, None) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_debug_limits(None, 16, 15, 0) == -1 and err() == "null correlator"
    assert lib.tdsa_corr_destroy(None) == 0
