"""The FSK analysis without a GPU: the contract alone recovers clock, symbols and deviation of synthesised FSK and GFSK;
the accuracy of the device's new arithmetic is measured by a host program that compiles the same header; the segment
arithmetic and the argument errors, which the Python layer and the library report before any device call."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fsk_contract as fc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import fsk as fk
from topdogspectrumanalyser_amd import symbols as sy

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SPS = (4, 4.37, 8, 16, 33.3)
# (levels, modulation index, BT or None for rectangular pulses)
SIGNALS = ((2, 1.0, None), (4, 0.5, None), (2, 0.5, 0.5), (2, 0.32, 0.5), (4, 0.33, 0.5))
PHASES = (0.0, 0.37, 0.81)
N_SYM = 300


def _symbols_sent(r, idx, sps, off):
    """The indices the signal carries at the symbol instants the analysis chose (make_fsk stores symbol m at [m + 5])."""
    m = np.floor((r["delta"] + np.arange(r["K"]) * sps) / sps - off).astype(np.int64)
    return idx[m + 5]


# ---- the contract recovers the truth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("M,h,bt", SIGNALS)
def test_contract_recovers_clock_symbols_and_deviation(M, h, bt, sps):
    """300 random symbols, three clock phases, a carrier offset of 0.01 cycles per sample, white noise 40 dB and 25 dB
    down over the full sample rate, default B and L."""
    ratios = []
    for off in PHASES:
        for noise_db in (-40.0, -25.0):
            x, idx, centre = fc.make_fsk(M, sps, int(N_SYM * sps) + 8, h, bt, seed=3, offset=off, cfo=0.01, noise_db=noise_db)
            r = fc.analyse(x, sps, M)
            dt = (r["delta"] - centre) / sps
            dt -= round(dt)
            wrong = int(np.sum(r["indices"] != _symbols_sent(r, idx, sps, off)))
            ratio = float(r["dev"]) / (h / sps)             # half the adjacent spacing is h / sps half turns per sample
            ratios.append(ratio)
            print(f"M {M} h {h} BT {bt} sps {sps} phase {off} noise {noise_db:g} dB: K {r['K']}, clock error {dt:+.4f} symbol, "
                  f"{wrong} symbol errors, deviation / nominal {ratio:.4f}, offset {float(r['offset']) / 2:.5f} cycles/sample, "
                  f"|C|/P {abs(r['C']) / r['P']:.3f}, FSK error {r['fsk_error']:.4f}")
            assert abs(dt) <= 0.02
            assert wrong == 0
            assert not r["flags"]
            if bt is None:
                assert abs(ratio - 1.0) <= 0.03
            assert abs(float(r["offset"]) / 2 - 0.01) <= 0.1 * h / sps
    print(f"M {M} h {h} BT {bt} sps {sps}: deviation / nominal {min(ratios):.3f} .. {max(ratios):.3f}")


@pytest.mark.parametrize("sps", (8, 16, 33.3))
def test_default_boxcar_and_lag_keep_the_clock_that_one_sample_loses(sps):
    """GFSK at h = 0.32 and 25 dB: the line of e stands at a third of P with B = L = floor(sps / 2) and is all but gone
    with B = L = 1, where one sample's frequency step is small beside one sample's noise."""
    x, _, _ = fc.make_fsk(2, sps, int(N_SYM * sps) + 8, 0.32, 0.5, seed=3, noise_db=-25.0)
    q = {}
    for B in (fc.default_boxcar(sps), 1):
        r = fc.analyse(x, sps, 2, B=B, L=B)
        q[B] = abs(r["C"]) / r["P"]
    print(f"sps {sps}: |C|/P {q}")
    assert q[fc.default_boxcar(sps)] >= 0.3 and q[1] <= 0.05


def test_contract_pieces():
    assert fc.default_boxcar(4) == 2 and fc.default_boxcar(4.37) == 2 and fc.default_boxcar(33.3) == 16
    assert fc.boxcar_outputs(100, fc.IQ, 3) == 97 and fc.boxcar_outputs(100, fc.FREQ, 3) == 98
    assert fc.group_delay(fc.IQ, 4) == 2.0 and fc.group_delay(fc.FREQ, 4) == 1.5
    # B = 1 leaves d as it is, bit for bit
    d = np.random.default_rng(1).standard_normal(50).astype(np.float32)
    assert fc.boxcar32(d, 1).tobytes() == d.tobytes()
    assert np.array_equal(fc.boxcar32(np.arange(8, dtype=np.float32), 4), [1.5, 2.5, 3.5, 4.5, 5.5])
    # the tree is a sum: exact on integers, close to fsum elsewhere
    assert fc.tree_sum(np.arange(1000.0)) == 499500.0 and fc.tree_sum([]) == 0.0
    z = np.random.default_rng(2).standard_normal(4096)
    assert abs(fc.tree_sum(z) - math.fsum(z)) <= 24 * 2.0 ** -53 * float(np.abs(z).sum())
    # delta_fx: C = 0 is t = 0; a transition phase a quarter symbol on moves delta_fx by a quarter symbol
    one = fc.ONE
    assert fc.delta_of(0j, 4 * one, 2) == 3 * one and fc.delta_of(0j, 4 * one, 4) == 4 * one
    assert fc.delta_of(-1j, 8 * one, 4) == (2 + 2 + 4) * one
    for step in (4 * one, fc.step_of(4.37), 64 * one):
        for L in (1, 2, 33, 64):
            for t in np.linspace(0, 1, 41):
                assert one <= fc.delta_from_t(t, step, L) < step + one
    # an exact line on a binary grid: every figure exact
    for M in (2, 4, 8):
        i = np.random.default_rng(M).integers(0, M, 100)
        i[:M] = np.arange(M)
        v = (0.375 + (2 * i - (M - 1)) * 2.0 ** -5).astype(np.float32)
        r = fc.levels(v, M)
        assert (float(r["offset"]), float(r["dev"])) == (0.375, 2.0 ** -5) and np.array_equal(r["indices"], i)
        assert r["err_sumsq"] == 0.0 and r["err_peak"] == 0.0 and r["err_peak_k"] == 0 and r["flags"] == 0
        assert r["sum_l"] == int(np.sum(2 * i - (M - 1)))
        # hi = lo: every index 0, o = lo, g = 0, one level
        r = fc.levels(np.full(7, 0.3, dtype=np.float32), M)
        assert float(r["offset"]) == float(np.float32(0.3)) and float(r["dev"]) == 0.0 and not r["indices"].any()
        assert r["flags"] == fc.ONE_LEVEL and r["sum_l"] == -7 * (M - 1)
    assert np.array_equal(fc.decide(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 0.0, 1.0, 4), [0, 3, 0])
    # a level that is not finite flags the segment even where no difference exists to show it
    f = np.linspace(-0.1, 0.1, 16)
    assert fc.analyse(f, 4, 2, fc.FREQ, 1, 64, delta_fx=2 * one)["flags"] == 0
    for bad in (np.nan, np.inf):
        f[3] = bad
        r = fc.analyse(f, 4, 2, fc.FREQ, 1, 64, delta_fx=2 * one)
        assert r["flags"] == fc.NONFINITE and r["P"] == 0.0 and "dev" not in r
    # fmaf rounds once, also where the float64 sum lands on a float32 tie that the exact sum is not on
    # 3 (1 + 3 2^-23) = 3 + 4.5 ulp: a tie, which goes to the even 4 ulp alone and with c below, to 5 ulp with c above
    for c, ulps in ((0.0, 4), (2.0 ** -60, 5), (-2.0 ** -60, 4), (2.0 ** -30, 5), (-2.0 ** -30, 4)):
        got = float(fc.fmaf(np.float32(1 + 3 * 2.0 ** -23), np.array([3]), np.float32(c))[0])
        assert got == 3 + ulps * 2.0 ** -22, (c, got)
    a, c = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)
    assert float(fc.fmaf(a, np.array([3]), c)[0]) == float(np.float32(3 * float(a) + float(c)))


# ---- the arithmetic's accuracy, measured ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host compiler not available")
    exe = str(tmp_path_factory.mktemp("fsk") / "fsk_math_host")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "fsk_math_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    return r


def test_math_header_stays_within_the_contracts_constants(sweep):
    assert sweep.returncode == 0, sweep.stdout
    got = {k: float(v) for k, v in re.findall(r"^(t|dec|fit) ([0-9.]+)$", sweep.stdout, re.M)}
    print(got)
    bound = dict(t=fc.A_T, dec=fc.A_DEC, fit=fc.A_FIT)
    for name in ("t", "dec", "fit"):
        assert 0.3 < got[name] <= fc.MEASURED[name] <= bound[name], name     # measured, and not a sweep that compared nothing
        assert fc.MEASURED[name] - got[name] < 0.05 + 1e-9, name              # ... and the record is the measurement
    assert fc.A_T == pytest.approx(fc.A_ATAN / 2 + 1, abs=0.03)
    assert "special ok" in sweep.stdout


def test_design_document_states_the_section_and_the_constants():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.20" in txt and "tdsa_fsk_math.hpp" in txt
    for name in ("t", "dec", "fit"):
        assert f"{fc.MEASURED[name]:.2f}" in txt, name


# ---- segments ------------------------------------------------------------------------------------------------------------
def test_symbols_per_segment_is_the_integer_formula():
    sps_all = (4, 4.0000001, 4.37, 5, 7.999999, 8, 10.5, 16, 33.3, 63.99, 64, 4 + 2.0 ** -20)
    for sps in sps_all:
        step = sy.fixed_step(sps)
        assert step == fc.step_of(sps) and sy.phase_step(sps) == fc.nu_of(sps)
        for kind in (fc.IQ, fc.FREQ):
            for B in (1, 3, 64):
                for L in range(0, 601):
                    K = C.c_int(-5)
                    assert nat.lib.tdsa_fsk_symbols_per_segment(step, L, kind, B, C.byref(K)) == 0
                    nb = L - (1 if kind == fc.IQ else 0) - B + 1
                    want = ((nb - 4) << 32) // step - 1 if nb >= 4 else -1
                    assert K.value == max(want, 0), (sps, kind, B, L)
                    assert fk.symbols_per_segment(step, L, kind, B) == want == fc.symbols_per_segment(step, L, kind, B)
    K = C.c_int()
    lib = nat.lib
    assert lib.tdsa_fsk_symbols_per_segment((4 << 32) - 1, 100, 0, 1, C.byref(K)) == -1 and b"step=" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_symbols_per_segment((64 << 32) + 1, 100, 0, 1, C.byref(K)) == -1
    assert lib.tdsa_fsk_symbols_per_segment(4 << 32, 100, 2, 1, C.byref(K)) == -1 and b"input_kind=2" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_symbols_per_segment(4 << 32, 100, 0, 0, C.byref(K)) == -1 and b"boxcar=0" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_symbols_per_segment(4 << 32, 100, 0, 65, C.byref(K)) == -1 and b"boxcar=65" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_symbols_per_segment(4 << 32, 100, 0, 1, None) == -1 and b"null K" in lib.tdsa_last_error_string()
    # the first tap of the first symbol and the last tap of the last are inside b, whatever the offset
    for sps in (4, 4.37, 63.9, 64):
        step = fc.step_of(sps)
        for kind, B in ((fc.IQ, 1), (fc.FREQ, 3), (fc.IQ, 64)):
            for L in (int(3 * sps) + 8 + B, 255 + B, 1023):
                K = fc.symbols_per_segment(step, L, kind, B)
                nb = fc.boxcar_outputs(L, kind, B)
                for d in (fc.ONE, step + fc.ONE - 1):
                    i, _ = fc.sc.positions(d, step, K)
                    assert i[0] - 1 >= 0 and i[-1] + 2 <= nb - 1


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_python_layer_raises_before_the_library_is_called(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")
    monkeypatch.setattr(nat.lib, "tdsa_fsk_create", boom, raising=False)
    for kw, text in ((dict(samples_per_symbol=3.99), "samples_per_symbol"), (dict(samples_per_symbol=64.01), "samples_per_symbol"),
                     (dict(samples_per_symbol=float("nan")), "samples_per_symbol"), (dict(samples_per_symbol=4, levels=3), "levels=3"),
                     (dict(samples_per_symbol=4, levels=16), "levels=16"), (dict(samples_per_symbol=4, levels="qpsk"), "levels='qpsk'"),
                     (dict(samples_per_symbol=4, levels=2.5), "levels=2.5"), (dict(samples_per_symbol=4, input="audio"), "input='audio'"),
                     (dict(samples_per_symbol=4, boxcar=0), "boxcar=0"), (dict(samples_per_symbol=4, boxcar=65), "boxcar=65"),
                     (dict(samples_per_symbol=4, lag=0), "lag=0"), (dict(samples_per_symbol=4, lag=65), "lag=65"),
                     (dict(samples_per_symbol=4, timing="manual"), "timing='manual'"), (dict(samples_per_symbol=4, timing=0.5), "timing=0.5"),
                     (dict(samples_per_symbol=4, timing=5.0), "timing=5.0"), (dict(samples_per_symbol=4, max_host_samples=3), "max_host_samples")):
        with pytest.raises(ValueError, match=re.escape(text)):
            fk.FskAnalyzer(**kw)
    assert fk.level_count("msk") == 2 and fk.level_count("GMSK") == 2 and fk.level_count(8) == 8
    with pytest.raises(ValueError):                       # the symbol recovery still has no msk: its carrier stage cannot strip it
        sy.SymbolSync(4, modulation="msk")


def _bare(kind="iq", sps=4, B=2, M=2):
    a = object.__new__(fk.FskAnalyzer)                     # no device: the checks need the configuration only
    a.step, a.max_host_samples, a.samples_per_symbol = sy.fixed_step(sps), 1 << 12, float(sps)
    a.kind, a.input, a.boxcar, a.lag, a.levels = fk.KINDS[kind], kind, B, B, M
    a._h = None
    return a


def test_calls_are_checked_before_the_library_is_called():
    a = _bare()
    # n_b = seg_len - 2: K = floor((seg_len - 6) / 4) - 1
    assert a.symbols_per_segment(18) == 2 and a.symbols_per_segment(16394) == 4096
    for L in (0, 5, 17, 16398):
        with pytest.raises(ValueError, match="symbols per segment"):
            a.symbols_per_segment(L)
    f = _bare("freq", B=1)
    assert f.symbols_per_segment(16) == 2 and f._unit == 4 and a._unit == 8
    x = np.zeros(1000, dtype=np.complex64)
    for call, text in ((lambda: a.process(x.real, 100), "one complex stream"), (lambda: f.process(x, 100), "one real stream"),
                       (lambda: a.process(x.reshape(10, 100), 100), "one complex stream"),
                       (lambda: a.process(x[:50], 100), "less than one segment"), (lambda: a.process(x, 100, hop=0), "hop=0"),
                       (lambda: a.process(x, 100, out_stride=5), "out_stride=5"),
                       (lambda: a.process(np.zeros(8192, np.complex64), 100, hop=1), "max_host_samples"),
                       (lambda: a.process_device(None, 8, 100, 100, 1, 8, 5), "out_stride=5"),
                       (lambda: a.process_device(None, 4, 100, 100, 1, 8, 64), "8 bytes"),
                       (lambda: f.process_device(None, 6, 100, 100, 1, 8, 64), "4 bytes"),
                       (lambda: a.process_device(None, 8, 100, 100, 1, 6, 64), "float32"),
                       (lambda: a.process_device(None, 0, 100, 100, 1, 8, 64), "null pointer"),
                       (lambda: a.process_device(None, 8, 100, 0, 2, 8, 64), "hop=0"),
                       (lambda: a.process_device(None, 8, 100, 100, 0, 8, 64), "n_seg=0")):
        with pytest.raises(ValueError, match=re.escape(text)):
            call()


def test_result_figures_and_bits():
    rec = np.zeros(2, dtype=fk.RECORD)
    rec["delta_fx"], rec["c_re"], rec["c_im"], rec["p"] = 3 << 32, 0.3, 0.4, 1.0
    rec["offset"], rec["dev"], rec["err_sumsq"], rec["err_peak"] = 0.02, 0.05, 4 * 0.0009, 0.03
    idx = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=np.uint8)
    r = fk.result_from(rec, None, idx, 4, 4, 8.0, nat.FSK_IQ, 4)
    assert np.allclose(r.delta, 5.0) and np.allclose(r.timing_quality, 0.5) and np.allclose(r.deviation, 0.15)
    assert np.allclose(r.mod_index, 0.4) and np.allclose(r.fsk_error, 0.03 / 0.15) and np.allclose(r.peak_error, 0.2)
    assert np.allclose(r.offset_hz(1e6), 1e4) and np.allclose(r.deviation_hz(1e6), 7.5e4)
    assert r.bits("natural").tolist() == [[0, 0, 0, 1, 1, 0, 1, 1], [1, 1, 1, 0, 0, 1, 0, 0]]
    assert r.bits("gray").tolist() == [[0, 0, 0, 1, 1, 1, 1, 0], [1, 0, 1, 1, 0, 1, 0, 0]]
    assert np.allclose(fk.result_from(rec, None, idx, 4, 4, 8.0, nat.FSK_FREQ, 4).delta, 4.5)
    with pytest.raises(ValueError, match="mapping"):
        r.bits("binary")


def test_library_refuses_bad_arguments_without_touching_a_device():
    lib = nat.lib
    step, nu = 4 << 32, 1 << 30
    ok = (step, nu, 2, 0, 2, 2, 0, 0)
    bad = [(((4 << 32) - 1,) + ok[1:], b"step="), (((64 << 32) + 1, 1 << 26) + ok[2:], b"step="),
           ((step, nu + 2) + ok[2:], b"nu="), ((step, 0) + ok[2:], b"nu=0"),
           ((step, nu, 3) + ok[3:], b"levels=3"), ((step, nu, 16) + ok[3:], b"levels=16"),
           ((step, nu, 2, 2) + ok[4:], b"input_kind=2"), ((step, nu, 2, -1) + ok[4:], b"input_kind=-1"),
           ((step, nu, 2, 0, 0) + ok[5:], b"boxcar=0"), ((step, nu, 2, 0, 65) + ok[5:], b"boxcar=65"),
           ((step, nu, 2, 0, 2, 0) + ok[6:], b"lag=0"), ((step, nu, 2, 0, 2, 65) + ok[6:], b"lag=65"),
           ((step, nu, 2, 0, 2, 2, 2, 0), b"timing_mode=2"), ((step, nu, 2, 0, 2, 2, 1, (1 << 32) - 1), b"delta_fx="),
           ((step, nu, 2, 0, 2, 2, 1, step + (1 << 32)), b"delta_fx=")]
    for args, text in bad:
        assert lib.tdsa_fsk_configure(None, *args) == -1, args
        assert text in lib.tdsa_last_error_string(), (args, lib.tdsa_last_error_string())
    assert lib.tdsa_fsk_configure(None, *ok) == -1 and b"null FSK analyser" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_configure(None, step, nu, 8, 1, 64, 64, 1, step) == -1 and b"null FSK analyser" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_create(0, 0, None) == -1 and b"null out" in lib.tdsa_last_error_string()
    h = C.c_void_p()
    assert lib.tdsa_fsk_create(0, 8, C.byref(h)) == -1 and b"max_host_samples" in lib.tdsa_last_error_string()
    buf = (C.c_ubyte * 64)()
    assert lib.tdsa_fsk_process(None, buf, 8, 8, 8, 1, buf, 8, None, buf) == -1 and b"null FSK analyser" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_process_dev(None, None, buf, 8, 8, 1, buf, 8, None, buf) == -1
    assert lib.tdsa_fsk_timer_begin(None) == -1 and lib.tdsa_fsk_timer_end(None, None) == -1
    assert b"null FSK analyser" in lib.tdsa_last_error_string()
    assert lib.tdsa_fsk_destroy(None) == 0
    assert C.sizeof(C.c_uint64) * 8 == fk.RECORD.itemsize
    # the record's layout is the header's
    hdr = open(os.path.join(ROOT, "include", "tdsa_hip.h")).read()
    body = re.search(r"typedef struct tdsa_fsk_record \{(.*?)\} tdsa_fsk_record;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(fk.RECORD.names)
