"""The symbol recovery without a GPU: the float64 contract recovers timing, carrier and symbols of synthesised signals;
the accuracy of the device's arithmetic is measured by a host program that compiles the same header; the segment
arithmetic, the root-raised-cosine design and the argument errors, which the Python layer and the library report before
any device call."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import symsync_contract as sc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import symbols as sy

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SPS = (4, 4.37, 8)
MODS = ("bpsk", "qpsk", "8psk", "16qam", "64qam")
W, SEG = 0.01, 4096


# ---- the contract recovers the truth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("mod", MODS)
def test_contract_recovers_timing_carrier_and_symbols(mod, sps):
    """A random symbol stream through a raised-cosine pulse evaluated in float64 at the sample instants: timing offset
    0.37 symbols, carrier 0.01 rad / sample from phase 0.7, noise at -40 dB, one segment of 4096 samples."""
    x, _, off = sc.make_signal(mod, sps, SEG, seed=1, offset=0.37, w=W, phase=0.7, noise_db=-40.0)
    M = sc.ORDER[mod]
    r = sc.recover(x, sps, M, sc.reference_phase(sc.points(mod), M))
    dt = (r["delta_fx"] / sc.ONE - off) / sps
    dt -= round(dt)
    df = r["f"] / M - W * sps / (2 * math.pi)
    e = sc.evm(r["symbols"], mod)
    print(f"{mod} sps {sps}: K {r['K']}, timing error {dt:+.4f} symbol, carrier error {df:+.2e} cycles/symbol, EVM {e:.4f}")
    assert abs(dt) <= 0.02
    if mod in ("bpsk", "qpsk", "8psk"):
        assert abs(df) <= 1e-4
        assert e <= 0.02
    else:
        assert e <= 0.04
    # the step the device would use says the same as f
    assert abs(((r["step_f"] + (1 << 31)) % sc.ONE - (1 << 31)) / sc.ONE - r["f"] / M) <= 2.0 ** -32


def test_contract_pieces():
    assert sc.step_of(4) == 4 << 32 and sc.nu_of(4) == 1 << 30 and sc.nu_of(64) == 1 << 26
    assert [sc.grid(k) for k in (2, 3, 4, 5, 1022, 2048, 2049, 4096)] == [4, 8, 8, 16, 2048, 4096, 8192, 8192]
    assert np.array_equal(sc.coeffs(0.0), [0, 1, 0, 0])
    for name in MODS:
        want = math.pi if name in ("qpsk", "16qam", "64qam") else 0.0
        assert abs(abs(sc.reference_phase(sc.points(name), sc.ORDER[name])) - want) < 1e-9
        assert abs(abs(sy.reference_phase(sy.constellation_points(name), sy.carrier_order(name))) - want) < 1e-6
        assert sy.carrier_order(name) == sc.ORDER[name]
    # an all-zero segment: delta_fx = step, g = 0, f = 0
    r = sc.recover(np.zeros(64, dtype=np.complex128), 4, 4)
    assert r["delta_fx"] == 4 << 32 and r["g"] == 0 and r["f"] == 0.0 and r["step_f"] == 0
    # the first tap of the first symbol and the last tap of the last are inside the segment, whatever the offset
    for sps in (4, 4.37, 63.9, 64):
        step = sc.step_of(sps)
        for L in (int(3 * sps) + 8, 255, 1023):
            K = sc.symbols_per_segment(step, L)
            for d in (sc.ONE, step + sc.ONE - 1):
                i, _ = sc.positions(d, step, K)
                assert i[0] - 1 >= 0 and i[-1] + 2 <= L - 1


# ---- the arithmetic's accuracy, measured ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host compiler not available")
    exe = str(tmp_path_factory.mktemp("symsync") / "symsync_math_host")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "symsync_math_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    return r


def test_math_header_stays_within_the_contracts_constants(sweep):
    assert sweep.returncode == 0, sweep.stdout
    got = {k: float(v) for k, v in re.findall(r"^(coef|pow2|pow4|pow8|rot|atan) ([0-9.]+)$", sweep.stdout, re.M)}
    print(got)
    assert 0.3 < got["coef"] <= sc.A_C                 # measured, and not a sweep that compared nothing
    for M in (2, 4, 8):
        assert 0.3 < got[f"pow{M}"] <= sc.A_POW[M]
    assert 0.3 < got["rot"] <= sc.A_ROT
    assert 0.3 < got["atan"] <= sc.A_ATAN
    assert "special ok" in sweep.stdout                # mu = 0 gives exactly (0, 1, 0, 0), quarter turns are exact, ...


# ---- segments, taps ---------------------------------------------------------------------------------------------------
def test_symbols_per_segment_is_the_integer_formula():
    sps_all = (4, 4.0000001, 4.37, 5, 7.999999, 8, 10.5, 16, 33.3, 63.99, 64, 4 + 2.0 ** -20)
    for sps in sps_all:
        step = sy.fixed_step(sps)
        assert step == sc.step_of(sps) and sy.phase_step(sps) == sc.nu_of(sps)
        for L in range(0, 601):
            K = C.c_int(-5)
            assert nat.lib.tdsa_symsync_symbols_per_segment(step, L, C.byref(K)) == 0
            want = ((L - 4) << 32) // step - 1 if L >= 4 else -1
            assert K.value == max(want, 0), (sps, L)
            assert sy.symbols_per_segment(step, L) == want == sc.symbols_per_segment(step, L)
    K = C.c_int()
    assert nat.lib.tdsa_symsync_symbols_per_segment((4 << 32) - 1, 100, C.byref(K)) == -1
    assert nat.lib.tdsa_symsync_symbols_per_segment((64 << 32) + 1, 100, C.byref(K)) == -1
    assert nat.lib.tdsa_symsync_symbols_per_segment(4 << 32, 100, None) == -1


@pytest.mark.parametrize("sps,alpha,span", [(4, 0.35, 8), (2, 0.35, 12), (8, 0.22, 16), (5, 0.5, 10), (4, 1.0, 8)])
def test_rrc_taps_have_unit_energy_symmetry_and_no_isi_in_cascade(sps, alpha, span):
    h = sy.rrc_taps(sps, alpha, span)
    assert h.dtype == np.float32 and h.size % 2 == 1
    assert abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    assert np.array_equal(h, h[::-1])
    rc = np.convolve(h.astype(np.float64), h.astype(np.float64))
    mid = rc.size // 2
    isi = [abs(rc[mid + k * sps]) for k in range(1, span) if mid + k * sps < rc.size]
    print(f"sps {sps} alpha {alpha} span {span}: peak {rc[mid]:.6f}, worst ISI {max(isi):.2e}")
    assert abs(rc[mid] - 1.0) <= 1e-5 and max(isi) <= 1e-3


def test_rrc_taps_refuse_bad_arguments():
    for args in ((0.5,), (4, 0.0), (4, 1.5), (4, 0.35, 0)):
        with pytest.raises(ValueError):
            sy.rrc_taps(*args)


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_python_layer_raises_before_the_library_is_called(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")
    monkeypatch.setattr(nat.lib, "tdsa_symsync_create", boom, raising=False)
    for kw in (dict(samples_per_symbol=3.99), dict(samples_per_symbol=64.01), dict(samples_per_symbol=float("nan")),
               dict(samples_per_symbol=4, modulation="msk"), dict(samples_per_symbol=4, order=3),
               dict(samples_per_symbol=4, timing="manual"), dict(samples_per_symbol=4, timing=0.5),
               dict(samples_per_symbol=4, timing=5.0), dict(samples_per_symbol=4, max_host_samples=3),
               dict(samples_per_symbol=4, ref_arg=float("inf"))):
        with pytest.raises(ValueError):
            sy.SymbolSync(**kw)
    with pytest.raises(ValueError):
        sy.carrier_order("ofdm")


def test_calls_are_checked_before_the_library_is_called():
    s = object.__new__(sy.SymbolSync)                      # no device: the checks need the configuration only
    s.step, s.max_host_samples = sy.fixed_step(4), 1 << 12
    s._h = None
    assert s.symbols_per_segment(20) == 3 and s.symbols_per_segment(16392) == 4096
    for L in (0, 3, 15, 16, 16396):                        # K = -1, -1, 1, 2 is the first accepted, 4097
        if L == 16:
            assert s.symbols_per_segment(L) == 2
            continue
        with pytest.raises(ValueError):
            s.symbols_per_segment(L)
    x = np.zeros(1000, dtype=np.complex64)
    for call in (lambda: s.process(x.real, 100), lambda: s.process(x[:50], 100), lambda: s.process(x, 100, hop=0),
                 lambda: s.process(x, 100, out_stride=5), lambda: s.process(np.zeros(8192, np.complex64), 100, hop=1),
                 lambda: s.process_device(None, 8, 100, 100, 1, 8, 5), lambda: s.process_device(None, 4, 100, 100, 1, 8, 64),
                 lambda: s.process_device(None, 8, 100, 100, 1, 12, 64), lambda: s.process_device(None, 8, 100, 100, 1, 8, 64, 4),
                 lambda: s.process_device(None, 0, 100, 100, 1, 8, 64), lambda: s.process_device(None, 8, 100, 0, 2, 8, 64),
                 lambda: s.process_device(None, 8, 100, 100, 0, 8, 64)):
        with pytest.raises(ValueError):
            call()


def test_library_refuses_bad_arguments_without_touching_a_device():
    lib = nat.lib
    step, nu = 4 << 32, 1 << 30
    bad = [((4 << 32) - 1, nu, 4, 0.0, 0, 0), ((64 << 32) + 1, 1 << 26, 4, 0.0, 0, 0), (step, nu + 2, 4, 0.0, 0, 0),
           (step, 0, 4, 0.0, 0, 0), (step, nu, 3, 0.0, 0, 0), (step, nu, 16, 0.0, 0, 0), (step, nu, 4, float("nan"), 0, 0),
           (step, nu, 4, 0.0, 2, 0), (step, nu, 4, 0.0, 1, (1 << 32) - 1), (step, nu, 4, 0.0, 1, step + (1 << 32))]
    for args in bad:
        assert lib.tdsa_symsync_configure(None, *args) == -1, args
        assert b"null" not in lib.tdsa_last_error_string(), args        # the argument was refused, not the handle
    assert lib.tdsa_symsync_configure(None, step, nu, 4, 0.0, 1, step) == -1 and b"null" in lib.tdsa_last_error_string()
    assert lib.tdsa_symsync_create(0, 0, None) == -1
    h = C.c_void_p()
    assert lib.tdsa_symsync_create(0, 8, C.byref(h)) == -1 and b"max_host_samples" in lib.tdsa_last_error_string()
    buf = (C.c_ubyte * 64)()
    assert lib.tdsa_symsync_process(None, buf, 8, 8, 8, 1, buf, 8, None, buf) == -1
    assert lib.tdsa_symsync_process_dev(None, None, buf, 8, 8, 1, buf, 8, None, buf) == -1
    assert lib.tdsa_symsync_timer_begin(None) == -1 and lib.tdsa_symsync_timer_end(None, None) == -1
    assert lib.tdsa_symsync_destroy(None) == 0
    assert C.sizeof(C.c_uint64) * 6 == sy.RECORD.itemsize
