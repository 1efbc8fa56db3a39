"""The pulse analysis without a device: the contract (tests/pulse_contract.py) on constructed input, PulseTrain in
pulses.py on records the contract makes, the record and summary layouts, and every argument error that needs no handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pulse_contract as pc
from topdogspectrumanalyser_amd import PulseAnalyzer, PulseTrain, levels_from_db
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import pulses as pu

f32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdsa_hip.h")


def _amp(*powers):
    """complex64 samples (re, 0) whose float32 power is exactly the given one: the powers are squares of float32."""
    re = np.sqrt(np.array(powers, dtype=np.float64)).astype(f32)
    assert np.array_equal((re * re).astype(f32), np.array(powers, dtype=f32)), powers
    return re.astype(np.complex64)


def _stream(x, on=0.25, off=0.0625, **kw):
    return pc.Stream(on, off, **kw).feed(np.asarray(x, dtype=np.complex64), pc.C64)


def _train(s, stream=0):
    return PulseTrain(s.records(), s.summary(), stream)


HI, MID, LO = 1.0, 0.140625, 0.015625            # p of the classes A, C, B with on = 0.25, off = 0.0625: 1, (3/8)^2, (1/8)^2


# ---- the state machine -------------------------------------------------------------------------------------------
def test_c_samples_keep_the_state_after_a_and_after_b():
    s = _stream(_amp(MID, MID, HI, MID, MID, LO, MID, MID, HI, HI, LO, MID))
    t = _train(s)
    assert t.toa.tolist() == [2, 8] and t.width.tolist() == [3, 2]           # C after A stays on, C after B (and at the start) off
    assert t.n_on == 5 and t.n_total == 12 and t.open_pulse is None and t.duty_cycle == 5 / 12
    assert pc.states(pc.classes(np.array([MID, MID], dtype=f32), 0.25, 0.0625), True).tolist() == [True, True]


def test_nan_ends_a_pulse_and_never_starts_one():
    x = _amp(HI, HI, HI, LO, HI, MID).copy()
    x[2] = complex(np.nan, 0)
    x[3] = complex(0, np.nan)
    t = _train(_stream(x))
    assert t.toa.tolist() == [0] and t.width.tolist() == [2] and t.n_nan == 2 and t.open_pulse == (4, 2)
    t = _train(_stream(np.array([complex(np.nan, np.nan)] * 3 + [complex(np.inf, 0), 0], dtype=np.complex64)))
    assert t.toa.tolist() == [3] and t.flags.tolist() == [pc.FLAG_INF] and np.isinf(t.energy[0]) and t.n_nan == 3


def test_equal_levels_are_one_threshold():
    p = np.array([HI, MID, HI, LO, MID, HI], dtype=f32)
    s = pc.Stream(MID, MID).feed_iq(np.sqrt(p), np.zeros(6, dtype=f32))
    assert not (pc.classes(p, MID, MID) == pc.C).any()
    assert s.records()["toa"].tolist() == [0] and s.records()["width"].tolist() == [3] and s.summary()["open_toa"] == 4
    assert s.summary()["open_width"] == 2 and s.summary()["n_on"] == 5


def test_a_power_exactly_at_each_level_and_the_float32_below_it():
    on, off = f32(0.25), f32(0.0625)
    below = lambda v: np.nextafter(f32(v), f32(0))
    p = np.array([on, below(on), off, below(off)], dtype=f32)
    assert pc.classes(p, on, off).tolist() == [pc.A, pc.C, pc.C, pc.B]
    # the same through samples: (0.5, 0)^2 = on exactly; re = nextafter(0.5, 0) squares to below on
    x = np.array([0.5, below(0.5), 0.25, below(0.25), below(0.5), 0.25, 0.5, 0.0], dtype=np.complex64)
    t = _train(_stream(x))
    assert t.toa.tolist() == [0, 6] and t.width.tolist() == [3, 1]            # below(0.5) alone does not switch on
    assert np.isnan(t.freq[1]) and not np.isnan(t.freq[0])


def test_peak_ties_take_the_first_index_and_the_pair_sum_skips_the_first_sample():
    x = np.array([0, 0.5, 0.75, 0.5j, 0.75j, -0.75, 0], dtype=np.complex64)
    t = _train(_stream(x))
    assert t.toa.tolist() == [1] and t.width.tolist() == [5] and t.peak_index.tolist() == [2]
    assert t.peak_bits[0] == f32(0.5625).view(np.uint32) and t.peak_power[0] == 0.5625
    assert t.energy[0] == 0.25 + 0.5625 + 0.25 + 0.5625 + 0.5625 and t.mean_power[0] == t.energy[0] / 5
    # x[2] conj(x[1]) + x[3] conj(x[2]) + x[4] conj(x[3]) + x[5] conj(x[4]); x[1] conj(x[0]) is not part of the pulse
    want = 0.75 * 0.5 + 0.5j * 0.75 + 0.75j * -0.5j + -0.75 * -0.75j
    assert (t.acc_re[0], t.acc_im[0]) == (want.real, want.imag)


def test_min_width_drops_the_pulse_one_sample_short():
    for w in (1, 2, 5):
        parts = []
        for width in (w - 1, w, w + 1):
            parts += [HI] * width + [LO] * 2
        t = _train(_stream(_amp(*parts), min_width=w))
        kept = [width for width in (w - 1, w, w + 1) if width >= max(w, 1)]
        assert t.width.tolist() == kept and t.n_short == (1 if w > 1 else 0) and t.n_on == 3 * w


def test_overflow_counts_n_lost_and_keeps_the_first_pulses():
    x = _amp(*([HI, LO] * 7))
    for capacity in (1, 3, 7, 8):
        t = _train(_stream(x, capacity=capacity))
        assert len(t) == min(capacity, 7) and t.toa.tolist() == list(range(0, 14, 2))[:capacity]
        assert t.n_pulses == 7 and t.n_lost == max(0, 7 - capacity)


def test_an_open_pulse_is_reported_then_completed_by_a_second_block():
    a, b = _amp(LO, HI, MID, HI), _amp(MID, 4.0, LO, HI)
    s = pc.Stream(0.25, 0.0625).feed(a, pc.C64)
    t = _train(s)
    assert len(t) == 0 and t.open_pulse == (1, 3) and t.n_pulses == 0
    s.feed(b, pc.C64)
    t = _train(s)
    assert t.toa.tolist() == [1] and t.width.tolist() == [5] and t.peak_index.tolist() == [5] and t.open_pulse == (7, 1)
    whole = _stream(np.concatenate([a, b]))
    assert pc.within_bounds(s.records(), whole.records()) is None and s.summary() == whole.summary()
    # the pair that crosses the blocks is part of the sum: 3/8 * 1 from x[4] conj(x[3])
    assert t.acc_re[0] == 1 * 0.375 + 0.375 * 1 + 1 * 0.375 + 0.375 * 2.0
    # any split of a noisy stream gives the same integers
    rng = np.random.default_rng(1)
    x = ((rng.standard_normal(5000) + 1j * rng.standard_normal(5000)) * 0.3).astype(np.complex64)
    one = _stream(x, min_width=2, capacity=50)
    cut = pc.Stream(0.25, 0.0625, 2, 50)
    for part in np.split(x, [1, 2, 700, 701, 3333]):
        cut.feed(part, pc.C64)
    assert pc.within_bounds(cut.records(), one.records()) is None and cut.summary() == one.summary() and one.sum["n_lost"] > 0


def test_a_tone_burst_gives_its_frequency_and_power():
    n = np.arange(1000)
    burst = (0.5 * np.exp(2j * np.pi * n / 16)).astype(np.complex64)
    x = np.concatenate([np.zeros(10, dtype=np.complex64), burst, np.zeros(10, dtype=np.complex64)])
    t = _train(_stream(x, on=0.125, off=0.0625))
    assert t.toa.tolist() == [10] and t.width.tolist() == [1000]
    print(f"freq {t.freq[0]!r}, error {abs(t.freq[0] - 1 / 16):.3e}; mean power {t.mean_power[0]!r}")
    assert abs(t.freq[0] - 1 / 16) <= 1e-6              # one pair's angle is off by about 4e-8 from the components' float32 rounding
    assert abs(t.mean_power[0] - 0.25) <= 1e-6 * 0.25
    assert abs(t.freq[0]) <= 0.5 and t.prf(1e6).size == 0 and t.pri().size == 0
    toa_s, width_s = t.to_seconds(1e6)
    assert toa_s[0] == 1e-5 and width_s[0] == 1e-3
    two = _train(_stream(np.concatenate([x, x]), on=0.125, off=0.0625))
    assert two.pri().tolist() == [1020] and two.prf(1.02e6).tolist() == [1000.0]


def test_levels_from_db():
    assert levels_from_db(0.0) == (1.0, 1.0)
    on, off = levels_from_db(-10.0, 3.0)
    assert on == float(f32(10.0 ** -1.0)) and off == float(f32(10.0 ** -1.3)) and off < on
    with pytest.raises(ValueError):
        levels_from_db(0.0, -1.0)


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
    ctypes_of = {"int64_t": np.int64, "uint64_t": np.uint64, "uint32_t": np.uint32, "int32_t": np.int32, "double": np.float64}
    for struct, dtype, cdef, size in (("tdsa_pulse_record", pu.RECORD, nat.PulseRecord, 64),
                                      ("tdsa_pulse_summary", pu.SUMMARY, nat.PulseSummary, 72)):
        fields = _header_fields(struct)
        assert [n for n, _ in fields] == list(dtype.names)
        off = 0
        for name, ctype in fields:                       # the header's order, naturally aligned, no padding
            assert dtype.fields[name][0] == np.dtype(ctypes_of[ctype]) and dtype.fields[name][1] == off == getattr(cdef, name).offset, name
            off += np.dtype(ctypes_of[ctype]).itemsize
        assert off == size == dtype.itemsize == C.sizeof(cdef)
    assert pu.RECORD == pc.RECORD and pu.SUMMARY == pc.SUMMARY and pu.COUNTS == pc.COUNTS
    hpp = open(os.path.join(os.path.dirname(pu.__file__), "csrc", "tdsa_pulse.hpp")).read()
    assert "static_assert(sizeof(PulseRecord) == 64" in hpp and "static_assert(sizeof(PulseSummary) == 72" in hpp


@pytest.mark.parametrize("kw", [dict(streams=0), dict(streams=257), dict(capacity=0), dict(capacity=-1), dict(streams=2, capacity=(1 << 21) + 1),
                                dict(capacity=(1 << 22) + 1), dict(streams=4, max_host_samples=3)])
def test_the_constructor_refuses_before_the_library_is_called(kw, monkeypatch):
    monkeypatch.setattr(nat.lib, "tdsa_pulse_create", lambda *a: pytest.fail("the library was called"))
    with pytest.raises(ValueError):
        PulseAnalyzer(**kw)


def _bare(streams=1):
    """A PulseAnalyzer that never reached the library, for the checks that come before it."""
    p = PulseAnalyzer.__new__(PulseAnalyzer)
    p.streams, p.capacity, p.device, p.max_host_samples, p._h = streams, 16, 0, 1 << 20, None
    return p


def test_calls_refuse_before_the_library_is_called(monkeypatch):
    for name in ("tdsa_pulse_process", "tdsa_pulse_process_dev", "tdsa_pulse_read", "tdsa_pulse_read_pulses", "tdsa_pulse_configure"):
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
    for args in ((0.0,), (-1.0,), (float("inf"),), (float("nan"),), (1e39,), (1.0, 2.0), (1.0, 0.0), (1.0, -0.5), (1.0, float("nan")),
                 (1.0, None, 0), (1.0, None, 1 << 31), (1.0, None, 1.5), (1.0, None, "x")):
        with pytest.raises(ValueError):
            one.configure(*args)


def test_argument_errors_that_need_no_handle_return_minus_1():
    lib, h = nat.lib, C.c_void_p()
    err = lambda: lib.tdsa_last_error_string().decode()
    for streams in (0, -1, 257):
        assert lib.tdsa_pulse_create(0, streams, 16, 1024, C.byref(h)) == -1 and "streams" in err() and not h
    for streams, capacity in ((1, 0), (1, -5), (1, (1 << 22) + 1), (256, (1 << 14) + 1)):
        assert lib.tdsa_pulse_create(0, streams, capacity, 1024, C.byref(h)) == -1 and "capacity" in err() and not h
    assert lib.tdsa_pulse_create(0, 1, 16, 1024, None) == -1 and "null" in err()
    assert lib.tdsa_pulse_create(0, 4, 16, 3, C.byref(h)) == -1 and "max_host_samples" in err()
    for on in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.tdsa_pulse_configure(None, on, 0.5, 1) == -1 and "on_level" in err()
    for off in (0.0, -1.0, float("nan"), 1.5):
        assert lib.tdsa_pulse_configure(None, 1.0, off, 1) == -1 and "off_level" in err()
    for w in (0, -1, 1 << 31, 1 << 40):
        assert lib.tdsa_pulse_configure(None, 1.0, 1.0, w) == -1 and "min_width" in err()
    assert lib.tdsa_pulse_configure(None, 1.0, 0.5, 1) == -1 and "null" in err()
    buf = (C.c_byte * 64)()
    for fmt in (-1, 3, 7):
        assert lib.tdsa_pulse_process(None, fmt, buf, 4, 4) == -1 and "in_format" in err()
        assert lib.tdsa_pulse_process_dev(None, None, fmt, buf, 4, 4) == -1 and "in_format" in err()
    assert lib.tdsa_pulse_process_dev(None, None, nat.IN_C64, C.c_void_p(4100), 4, 4) == -1 and "aligned" in err()
    assert lib.tdsa_pulse_process_dev(None, None, nat.IN_I8, C.c_void_p(4097), 4, 4) == -1 and "aligned" in err()
    assert lib.tdsa_pulse_process(None, nat.IN_I8, buf, 4, 4) == -1 and "null" in err()
    assert lib.tdsa_pulse_process_dev(None, None, nat.IN_U8, C.c_void_p(4096), 4, 4) == -1 and "null" in err()
    assert lib.tdsa_pulse_read(None, 0, 1, None) == -1 and "null summaries" in err()
    assert lib.tdsa_pulse_read(None, 0, 1, buf) == -1 and "null" in err()
    n = C.c_int(5)
    assert lib.tdsa_pulse_read_pulses(None, 0, 0, 1, buf, None) == -1 and "null n_out" in err()
    assert lib.tdsa_pulse_read_pulses(None, 0, 0, 1, buf, C.byref(n)) == -1 and "null" in err() and n.value == 0
    assert lib.tdsa_pulse_debug_limits(None, 16, 7) == -1
    assert lib.tdsa_pulse_reset(None) == -1 and lib.tdsa_pulse_timer_begin(None) == -1 and lib.tdsa_pulse_timer_end(None, None) == -1
    assert lib.tdsa_pulse_destroy(None) == 0
