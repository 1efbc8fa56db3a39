"""Zoom front end, host side (no GPU): the default decimating filter meets its figures, the float64 restatement in
tests/zoom_contract.py checks itself, offsets quantise and wrap, the zoomed axis is right, tdsa_ddc.hip compiles for
gfx950 without scratch, and the C-ABI refuses bad arguments before it touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import zoom_contract as zc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd.zoom import (alias_free_bins, design_decimator, nco_step, zoom_freq_bins)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _response_db(h: np.ndarray, D: int):
    """|H(f)| in dB on a grid of f in cycles per input sample, from a zero-padded real FFT."""
    n = 1 << int(np.ceil(np.log2(32 * h.size)))
    H = np.abs(np.fft.rfft(h.astype(np.float64), n))
    f = np.arange(H.size) / n
    return f, 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("D", [2, 3, 8, 64, 1000, 4096])
def test_default_filter_design(D):
    h = design_decimator(D)
    assert h.dtype == np.float32 and h.size == 34 * D
    assert np.max(np.abs(h - h[::-1])) <= np.spacing(np.float32(h.max()))
    assert abs(float(np.sum(h, dtype=np.float64)) - 1.0) <= 1e-6
    f, db = _response_db(h, D)
    stop = db[f >= 0.6 / D].max()
    pas = db[f <= 0.4 / D]
    assert stop <= -100.0, (D, stop)
    assert pas.max() - pas.min() <= 0.001, (D, pas.max() - pas.min())


def test_design_refuses_out_of_range():
    for bad in (1, 4097):
        with pytest.raises(ValueError):
            design_decimator(bad)
    with pytest.raises(ValueError):
        design_decimator(8, taps_per_phase=65)


@pytest.mark.parametrize("D,T", [(2, 68), (3, 10), (4, 9), (5, 3), (8, 1), (7, 64 * 7)])
def test_restatement_checks_itself(D, T):
    """The defining sum at chosen m equals np.convolve(v, h)[::D], including T not a multiple of D and T < D."""
    rng = np.random.default_rng(D * 1000 + T)
    n = 5 * T + 3 * D + 7
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.standard_normal(T).astype(np.float32)
    full = zc.by_convolution(v, h, D)
    assert full.size == zc.n_outputs(n, D)
    ms = np.unique(np.concatenate([[0, 1, full.size - 1], rng.integers(0, full.size, 20)]))
    np.testing.assert_allclose(zc.direct(v, h, D, ms), full[ms], rtol=0, atol=1e-12 * np.abs(h).sum() * 4)


def test_restatement_phase_track_is_continuous():
    s1, s2 = 123456789, (-987654321) % (1 << 32)
    p = zc.phases(100, [(0, s1), (40, s2)])
    assert p[0] == 0 and p[39] == (39 * s1) % (1 << 32)
    assert p[40] == (40 * s1) % (1 << 32) and p[41] == (40 * s1 + s2) % (1 << 32)


def test_integer_reference_checks_itself():
    """zc.integer_fir (the exact reference of test_gpu_zoom_shapes.py) against np.convolve in int64."""
    rng = np.random.default_rng(5)
    for D, T in [(2, 1), (3, 7), (5, 11), (13, 3 * 13 + 1), (64, 130)]:
        n = 3 * T + 9 * D + 4
        re, im = rng.integers(-7, 8, (2, n))
        h = rng.integers(-7, 8, T).astype(np.float32)
        yr, yi = zc.integer_fir(re, im, h, D)
        hi = h.astype(np.int64)
        assert np.array_equal(yr, np.convolve(re, hi)[::D][:zc.n_outputs(n, D)])
        assert np.array_equal(yi, np.convolve(im, hi)[::D][:zc.n_outputs(n, D)])
    assert [zc.lanes(D) for D in (2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 4096)] == [2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]


def _fmaf(a, b, c):
    """fmaf of float32 arrays: the float64 product of two float32 values is exact, so this is one float64 addition
    rounded to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_rotator_arithmetic_stays_within_one_ulp():
    """ddc_mix's rotator (tdsa_ddc.hip) written out in numpy float32, operation by operation, for x = 1: every one of
    the 4096 table entries against some 200 values of the low 20 phase bits, their extremes included.  DESIGN.md section 4.8
    documents 1.5 ulp of |h|; the arithmetic itself stays within 1.0 x spacing(1) (0.50 measured), which pins the
    documented margin without a GPU.  test_gpu_zoom_shapes.py measures the kernel."""
    f32 = np.float32
    rng = np.random.default_rng(20)
    lows = np.unique(np.concatenate([[0, 1, 0x7FFFF, 0x80000, 0xFFFFE, 0xFFFFF], rng.integers(0, 1 << 20, 200)]))
    assert lows.size >= 200
    top = np.arange(4096)
    th = 2.0 * np.pi * top / 4096.0
    hx = np.cos(th).astype(f32)[:, None]                   # the table: (cos, -sin) rounded from float64
    hy = (-np.sin(th)).astype(f32)[:, None]
    low = np.broadcast_to(lows[None, :], (4096, lows.size))
    t = low.astype(f32) * f32(1.46291807926715968e-9)      # 2 pi / 2^32
    t2 = t * t
    sl = _fmaf(t * t2, np.full_like(t, f32(0.16666667)), -t)
    cm1 = t2 * f32(-0.5)
    rr = hx + _fmaf(np.broadcast_to(hx, t.shape), cm1, -(hy * sl))
    ri = hy + _fmaf(np.broadcast_to(hy, t.shape), cm1, hx * sl)
    for a in (t, t2, sl, cm1, rr, ri):
        assert a.dtype == f32
    # x = 1 + 0j: (fma(1, rr, -(0 * ri)), fma(1, ri, 0 * rr)) = (rr, ri)
    p = (top[:, None].astype(np.int64) << 20) + low
    want = np.exp(-2j * np.pi * (p.astype(np.float64) / 2.0 ** 32))
    err = np.maximum(np.abs(rr.astype(np.float64) - want.real), np.abs(ri.astype(np.float64) - want.imag))
    worst = err.max() / float(np.spacing(f32(1)))
    assert worst <= 1.0, (worst, hex(int(p.reshape(-1)[np.argmax(err)])))


def test_offset_quantisation_and_wrapping():
    fs = 20e6
    step, actual = nco_step(1e6, fs)
    assert step == round(1e6 * 2 ** 32 / fs) and actual == step * fs / 2 ** 32
    assert abs(actual - 1e6) <= fs / 2 ** 33
    step, actual = nco_step(-1e6, fs)
    assert step == (1 << 32) - round(1e6 * 2 ** 32 / fs) and actual < 0 and abs(actual + 1e6) <= fs / 2 ** 33
    assert nco_step(0.0, fs) == (0, 0.0)
    assert nco_step(fs / 2, fs)[0] == 1 << 31 and nco_step(-fs / 2, fs)[0] == 1 << 31
    assert nco_step(fs / 2, fs)[1] == fs / 2 and nco_step(-fs / 2, fs)[1] == -fs / 2
    for bad in (fs / 2 * (1 + 1e-12), -fs, 3 * fs):
        with pytest.raises(ValueError):
            nco_step(bad, fs)


def test_zoomed_axis():
    fs, D, N = 20e6, 64, 4096
    fb = zoom_freq_bins(N, D, fs, 100e6, 1.25e6)
    assert np.allclose(np.diff(fb), fs / (D * N))
    assert fb[N // 2] == 100e6 + 1.25e6
    assert np.isclose(fb[0], 100e6 + 1.25e6 - fs / D / 2)
    sl = alias_free_bins(N, D, fs)
    base = fb - 100e6 - 1.25e6
    inside = np.abs(base) <= 0.4 * fs / D
    assert np.array_equal(np.nonzero(inside)[0], np.arange(sl.start, sl.stop))
    assert sl.stop - sl.start == 2 * int(0.4 * N) + 1


def test_ddc_kernels_compile_scratch_free():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/tdsa_ddc.o" in mk
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "tdsa_ddc.hip", "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)\s+\[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = [k for k in kernels if "ddc_" in k]
    assert len(names) >= 7, sorted(kernels)
    for k in names:
        assert kernels[k]["ScratchSize [bytes/lane]"] == "0", (k, kernels[k])
        assert kernels[k].get("VGPRs Spill", "0") == "0", (k, kernels[k])
        assert int(kernels[k]["LDS Size [bytes/block]"]) <= 64 * 1024, (k, kernels[k])


def _err():
    return nat.lib.tdsa_last_error_string().decode()


def test_c_abi_refuses_bad_arguments_without_a_device():
    h = C.c_void_p()
    assert nat.lib.tdsa_ddc_create(0, 1, 34, 1024, C.byref(h)) == nat_ERR_ARG and "decimation" in _err()
    assert nat.lib.tdsa_ddc_create(0, 4097, 34, 1024, C.byref(h)) == nat_ERR_ARG and "decimation" in _err()
    assert nat.lib.tdsa_ddc_create(0, 8, 0, 1024, C.byref(h)) == nat_ERR_ARG and "max_taps" in _err()
    assert nat.lib.tdsa_ddc_create(0, 8, 64 * 8 + 1, 1024, C.byref(h)) == nat_ERR_ARG and "max_taps" in _err()
    assert nat.lib.tdsa_ddc_create(0, 8, 34, 0, C.byref(h)) == nat_ERR_ARG
    assert nat.lib.tdsa_ddc_create(0, 8, 34, 1024, None) == nat_ERR_ARG and "null" in _err()
    n = C.c_size_t()
    buf = (C.c_float * 64)()
    assert nat.lib.tdsa_ddc_process(None, 7, buf, 4, buf, C.byref(n)) == nat_ERR_ARG and "in_format" in _err()
    assert nat.lib.tdsa_ddc_process_dev(None, None, 3, buf, 4, buf, C.byref(n)) == nat_ERR_ARG and "in_format" in _err()
    assert nat.lib.tdsa_ddc_process(None, 2, buf, 4, buf, C.byref(n)) == nat_ERR_ARG and "null" in _err()
    assert nat.lib.tdsa_ddc_process_dev(None, None, 0, buf, 4, buf, C.byref(n)) == nat_ERR_ARG and "null" in _err()
    assert nat.lib.tdsa_ddc_set_taps(None, buf, 4) == nat_ERR_ARG and "null" in _err()
    assert nat.lib.tdsa_ddc_set_nco(None, 5) == nat_ERR_ARG and "null" in _err()
    assert nat.lib.tdsa_ddc_reset(None) == nat_ERR_ARG and "null" in _err()
    assert nat.lib.tdsa_ddc_destroy(None) == 0
    assert nat.lib.tdsa_plan_copy(None, buf, buf, 4, 1) == nat_ERR_ARG and "null" in _err()


nat_ERR_ARG = -1
