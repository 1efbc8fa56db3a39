"""The analog demodulator without a GPU: the float64 contract on synthesised FM and AM signals, the pinned special cases
of the discriminator, the default audio filter, the accuracy of the device's discriminator arithmetic measured by a
host program that compiles the same header, and the argument errors, which the Python layer and the library report
before any device call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import demod_contract as dc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import demod as dm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_contract_recovers_the_phase_increments_of_an_fm_signal():
    rng = np.random.default_rng(1)
    n = 5000
    inc = 0.2 + 0.7 * np.sin(2 * np.pi * 0.003 * np.arange(n)) * rng.uniform(0.5, 1.0, n)     # half turns, |inc| < 0.9
    phase = np.pi * np.cumsum(inc)                                # float64
    x = np.exp(1j * phase) * (0.2 + 0.1 * rng.random(n))          # the amplitude must not matter
    d64 = dc.discriminator(x, dc.FM, as_stored=False)
    assert d64[0] == 0.0                                          # x[-1] = 0
    assert np.abs(d64[1:] - inc[1:]).max() <= 1e-12
    # ... and on the complex64 it is stored as, to float32 input rounding (2^-24 relative per component)
    d32 = dc.discriminator(x.astype(np.complex64), dc.FM)
    assert d32[0] == 0.0 and np.abs(d32[1:] - inc[1:]).max() <= 4 * dc.U


def test_contract_recovers_the_envelope_of_an_am_signal():
    rng = np.random.default_rng(2)
    n = 5000
    env = 0.5 * (1.0 + 0.8 * np.sin(2 * np.pi * 0.01 * np.arange(n)))
    x = env * np.exp(2j * np.pi * rng.random(n))
    assert np.abs(dc.discriminator(x, dc.AM, as_stored=False) - env).max() <= 1e-12
    d = dc.discriminator(x.astype(np.complex64), dc.AM)
    assert np.abs(d - env).max() <= 2 * dc.U * env.max()


def test_pinned_special_cases_of_the_contract():
    x = np.array([0, 1, 1j, -1j, -1j, 2j, 0, 0, 3, -0.5], dtype=np.complex64)
    d = dc.discriminator(x, dc.FM)
    #             x[-1]=0  0->1  +1/4   -1/2->1  same  half   p=0 p=0 p=0  half turn
    assert list(d) == [0.0, 0.0, 0.5, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    # Im p = -0 with Re p < 0 is +1, not -1
    x = np.array([1.0, complex(-1.0, -0.0)], dtype=np.complex64)
    assert dc.discriminator(x, dc.FM)[1] == 1.0
    x = np.array([complex(1.0, 0.0), complex(-1.0, 0.0)], dtype=np.complex64)
    assert dc.discriminator(x, dc.FM)[1] == 1.0
    assert list(dc.discriminator(np.array([3 + 4j, -5 + 12j, 0, -7j]), dc.AM)) == [5.0, 13.0, 0.0, 7.0]


def test_filter_pole_and_counts_of_the_contract():
    rng = np.random.default_rng(3)
    d = rng.standard_normal(100)
    g = rng.standard_normal(7).astype(np.float32)
    a = dc.fir(d, g, 3)
    assert a.size == dc.n_outputs(100, 3) == 34
    for m in (0, 1, 5, 33):
        want = sum(float(g[k]) * d[3 * m - k] for k in range(7) if 3 * m - k >= 0)
        assert abs(a[m] - want) <= 1e-12
    y = dc.one_pole(a, 0.75)
    assert abs(y[0] - 0.25 * a[0]) <= 1e-15 and abs(y[2] - (0.75 * y[1] + 0.25 * a[2])) <= 1e-15
    assert np.allclose(dc.output(a, dc.POLE_HIGH, 0.75, 2.0), 2.0 * (a - y), rtol=0, atol=1e-15)
    assert np.allclose(dc.output(a, dc.POLE_OFF, 0.75, 0.5), 0.5 * a, rtol=0, atol=0)
    assert dm.outputs_completed(0, 1, 3) == 1 and dm.outputs_completed(1, 2, 3) == 0 and dm.outputs_completed(3, 10, 3) == 4


def test_default_audio_filter_and_deemphasis_pole():
    assert list(dm.design_audio_filter(1)) == [1.0]
    for R in (2, 6, 64):
        g = dm.design_audio_filter(R)
        assert g.dtype == np.float32 and g.size == 34 * R
        assert abs(float(g.astype(np.float64).sum()) - 1.0) <= g.size * 2.0 ** -25 * float(np.abs(g).sum())
        dm.check_parameters("fm", 1, R, g.size)
    c = dm.deemphasis_pole(75e-6, 48000.0)
    assert abs(c - np.exp(-1.0 / (48000.0 * 75e-6))) <= 1e-15 and 0.75 < c < 0.76
    with pytest.raises(ValueError):
        dm.deemphasis_pole(0.0, 48000.0)
    with pytest.raises(ValueError):
        dm.design_audio_filter(65)


def test_derived_figures():
    a = np.array([[0.10, 0.12, 0.08, 0.10], [0.5, 1.5, 0.5, 1.5]])
    cnt, mx, mn, s, ss = dc.measurements(a)
    fm = dm.derive("fm", 200e3, cnt, mx, mn, s, ss)
    assert np.allclose(fm.offset_hz, [10e3, 100e3]) and np.allclose(fm.peak_plus_hz[0], 2e3) and np.allclose(fm.peak_minus_hz[0], 2e3)
    assert np.allclose(fm.rms_hz[0], 1e5 * np.std(a[0]))
    am = dm.derive("am", 200e3, cnt, mx, mn, s, ss)
    assert np.allclose(am.carrier, [0.1, 1.0]) and np.allclose(am.depth[1], 0.5)
    none = dm.derive("am", 1.0, [0], [-np.inf], [np.inf], [0.0], [0.0])
    assert np.isnan(none.carrier[0]) and np.isnan(none.depth[0])


# ---- the discriminator's accuracy, measured -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host compiler not available")
    exe = str(tmp_path_factory.mktemp("demod") / "demod_math_host")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "demod_math_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    return r


def test_discriminator_accuracy_stays_within_the_recorded_constant(sweep):
    assert sweep.returncode == 0, sweep.stdout
    fm = float(re.search(r"^fm ([0-9.]+)$", sweep.stdout, re.M).group(1))
    am = float(re.search(r"^am ([0-9.]+)$", sweep.stdout, re.M).group(1))
    print(f"worst discriminator error: FM {fm} u of a half turn, AM {am} u of |x|")
    assert 0.3 < fm <= dc.A_D_FM and 0.3 < am <= dc.A_D_AM        # measured, and not a sweep that compared nothing
    assert "special ok" in sweep.stdout


def test_discriminator_gives_nan_for_every_non_finite_sample(sweep):
    """The enumeration of demod_math_host.cpp: FM is NaN for every (x[n], x[n-1]) with a part that is not finite and a
    number in (-1, 1] otherwise, AM is IEEE's |x|; and the finite path is untouched - the accuracy sweep of the same run
    still prints the figures the constants were rounded up from."""
    assert sweep.returncode == 0, sweep.stdout
    m = re.search(r"^nonfinite ok ([0-9]+)$", sweep.stdout, re.M)
    assert m, sweep.stdout
    assert int(m.group(1)) == 9 ** 4 - 6 ** 4                       # every combination with a non-finite part was looked at
    assert re.search(r"^fm 1\.29$", sweep.stdout, re.M) and re.search(r"^am 1\.88$", sweep.stdout, re.M), sweep.stdout
    assert (dc.A_D_FM, dc.A_D_AM) == (1.30, 1.90)


def test_contract_discriminator_follows_the_non_finite_rule():
    nan, inf = np.nan, np.inf
    x = np.array([1, 1j, complex(nan, 0.1), 1, complex(inf, 0), -1, 2, complex(0, -inf), complex(nan, nan), 1, 1],
                 dtype=np.complex64)
    d = dc.discriminator(x, dc.FM)
    assert list(np.isnan(d)) == [False, False, True, True, True, True, False, True, True, True, False]
    assert list(d[[0, 1, 6, 10]]) == [0.0, 0.5, 1.0, 0.0]
    e = dc.discriminator(x, dc.AM)
    assert list(np.isfinite(e)) == [True, True, False, True, False, True, True, False, False, True, True]
    assert e[4] == inf and e[7] == inf and np.isnan(e[2]) and np.isnan(e[8])
    # the filter: an output is non-finite exactly where a non-zero tap meets the sample
    g = np.array([0.5, 0.0, 0.25, 0.0], dtype=np.float32)             # the last phase's padding and an inner zero
    dd = np.ones(12)
    dd[5] = nan
    with np.errstate(invalid="ignore"):
        a = dc.fir(dd, g, 1)
    assert list(np.nonzero(~np.isfinite(a))[0]) == [5, 6, 7, 8]         # np.convolve multiplies the zero taps too ...
    hit = [m for m in range(12) if 0 <= m - 5 < g.size and g[m - 5] != 0]
    assert hit == [5, 7]                                                # ... the rule names only these
    cnt, mx, mn, s, ss = dc.measurements(np.array([[1.0, nan, 3.0], [inf, 2.0, -1.0]]))
    assert list(cnt) == [3, 3] and list(mx) == [3.0, inf] and list(mn) == [1.0, -1.0]
    assert np.isnan(s[0]) and np.isnan(ss[0]) and s[1] == inf and ss[1] == inf


def test_design_document_states_the_measured_accuracy():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.13" in txt and f"{dc.A_D_FM:.2f}" in txt and f"{dc.A_D_AM:.2f}" in txt


# ---- argument errors ------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    bad = [("pm", 1, 1, 1), ("fm", 0, 1, 1), ("fm", 257, 1, 1), ("am", 1, 0, 1), ("am", 1, 65, 1), ("fm", 1, 2, 0),
           ("fm", 1, 2, 129), (2, 1, 1, 1)]
    for mode, chans, R, T in bad:
        with pytest.raises(ValueError):
            dm.check_parameters(mode, chans, R, T)
        with pytest.raises(ValueError):
            dm.Demodulator(mode, 48e3, R, chans, taps=np.ones(T, np.float32))
    for c in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dm.check_parameters("fm", 1, 1, 1, c)
    with pytest.raises(ValueError):
        dm.Demodulator("fm", 0.0)
    with pytest.raises(ValueError):
        dm.Demodulator("fm", 48e3, taps=[np.inf])
    with pytest.raises(ValueError):
        dm.Demodulator("fm", 48e3, deemphasis=-1.0)
    dm.check_call(10, 10, 4096, 4, 4, 4100)
    for args in [(10, 9, 4096, 4, 4, 4096), (10, 10, 4096, 4, 3, 4096), (10, 10, 4100, 4, 4, 4096),
                 (10, 10, 4096, 4, 4, 4098), (10, 10, 0, 4, 4, 4096), (10, 10, 4096, 4, 4, 0), (-1, 10, 4096, 0, 0, 4096)]:
        with pytest.raises(ValueError):
            dm.check_call(*args)
    with pytest.raises(ValueError):
        dm.check_same_device(1, 0)


def test_library_argument_errors_without_a_device():
    h, n, ms = C.c_void_p(), C.c_size_t(), C.c_float()
    err = nat.lib.tdsa_last_error_string
    bad_create = [(2, 1, 1, 1, 16), (-1, 1, 1, 1, 16),                         # mode
                  (0, 0, 1, 1, 16), (0, 257, 1, 1, 16),                        # channels
                  (0, 1, 0, 1, 16), (1, 1, 65, 1, 16),                         # R
                  (0, 1, 2, 0, 16), (0, 1, 2, 129, 16),                        # T
                  (0, 4, 1, 1, 3)]                                             # less than a sample per channel
    for mode, chans, R, T, mh in bad_create:
        assert nat.lib.tdsa_demod_create(0, mode, chans, R, T, mh, C.byref(h)) == -1, (mode, chans, R, T, mh)
        assert not h.value and err()
    assert nat.lib.tdsa_demod_create(0, 0, 1, 1, 1, 16, None) == -1 and b"null" in err()
    # pointers not aligned to 8 / 4 bytes, and a stride below n_in, are seen before the handle is
    assert nat.lib.tdsa_demod_process_dev(None, None, C.c_void_p(4100), 4, 4, C.c_void_p(4096), 4, C.byref(n)) == -1
    assert b"8 bytes" in err()
    assert nat.lib.tdsa_demod_process_dev(None, None, C.c_void_p(4096), 4, 4, C.c_void_p(4098), 4, C.byref(n)) == -1
    assert b"4 bytes" in err()
    assert nat.lib.tdsa_demod_process(None, C.c_void_p(4100), 4, 4, C.c_void_p(4096), 4, C.byref(n)) == -1 and b"8 bytes" in err()
    assert nat.lib.tdsa_demod_process_dev(None, None, C.c_void_p(4096), 5, 4, C.c_void_p(4096), 4, C.byref(n)) == -1
    assert b"in_stride" in err()
    # null handles, null results
    assert nat.lib.tdsa_demod_process(None, None, 0, 0, None, 0, C.byref(n)) == -1 and b"null" in err()
    assert nat.lib.tdsa_demod_process_dev(None, None, None, 0, 0, None, 0, C.byref(n)) == -1
    assert nat.lib.tdsa_demod_set_taps(None, None, 1) == -1 and nat.lib.tdsa_demod_set_pole(None, 0, 0.0, 1.0) == -1
    assert nat.lib.tdsa_demod_reset(None) == -1 and nat.lib.tdsa_demod_reset_meas(None) == -1
    assert nat.lib.tdsa_demod_read_meas(None, None, None, None, None, None) == -1
    assert nat.lib.tdsa_demod_timer_begin(None) == -1 and nat.lib.tdsa_demod_timer_end(None, C.byref(ms)) == -1
    assert nat.lib.tdsa_demod_destroy(None) == 0
