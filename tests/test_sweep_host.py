"""Stepped sweeps, host side (no GPU): the float64 restatement in tests/sweep_contract.py checks itself against np.interp
and against the reference's recorded sweep (tests/golden/sweep.npz; live against the reference class where its tree is
there), plan_steps covers its span on the fftshift(fftfreq) axis, bad geometry is refused, the peak rule holds on
hand-made cases, tdsa_sweep.hip compiles for gfx950 without scratch, the inputs of tests/test_gpu_sweep_shapes.py tell
the contract from every mutant of it, and the C-ABI refuses bad arguments before it touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sweep_contract as sc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import IqSweepDataSource, SweepAssembler, plan_steps  # noqa: F401  (the public names)
from topdogspectrumanalyser_amd.sweep import check_geometry, frequency_grid, step_frequencies

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
ERR_ARG = -1


def _same(a, b):
    """Bit for bit, any NaN equal to any NaN (and -0.0 not equal to 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)):
        return False
    num = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[num]), np.signbit(b[num])))


# ---------------------------------------------------------------------------------------------------- the contract
@pytest.mark.parametrize("seed", range(8))
def test_spelled_out_interpolation_is_np_interp(seed):
    rng = np.random.default_rng(seed)
    for _ in range(25):
        n = int(rng.integers(2, 60))
        xp = np.cumsum(rng.uniform(0.1, 5000.0, n)) + rng.uniform(-1e9, 6e9)
        fp = (-90 + 20 * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
        for v in (np.nan, np.inf, -np.inf):
            fp[rng.integers(0, n, 2)] = v
        if rng.random() < 0.3:
            fp[:] = np.inf                                  # inf - inf slopes: the fallbacks of np.interp
        grid = np.concatenate([rng.uniform(xp[0] - 1e4, xp[-1] + 1e4, 80), xp[rng.integers(0, n, 10)],
                               [xp[0], xp[-1], np.nextafter(xp[0], -np.inf), np.nextafter(xp[-1], np.inf)]])
        assert _same(sc.interp_spelled(grid, xp, fp), np.interp(grid, xp, fp))


def _golden():
    z = np.load(GOLDEN)
    fs, N, k0, k1, bin_hz, start, stop, bin_size = z["geometry"]
    return z, float(fs), int(N), int(k0), int(k1), float(bin_hz), int(start), int(stop), int(bin_size)


def test_contract_equals_the_recorded_reference_sweep():
    z, fs, N, k0, k1, bin_hz, start, stop, bin_size = _golden()
    assert bin_hz == 1.0 / (N * (1.0 / fs)) == 2000.0
    assert _same(z["grid"], frequency_grid(start, stop, bin_size))
    xp = sc.frequencies(z["centres"], k0, k1, N, bin_hz)
    assert np.all(xp == np.round(xp)) and np.all(np.diff(xp) > 0)
    assert np.max(np.diff(xp)) > 2 * bin_hz                       # the gap of the missing step
    want = z["full_power_array"]
    assert want.dtype == np.float64 and np.isnan(want).any() and np.isinf(want).any()
    present = np.ones(len(z["centres"]), dtype=bool)
    assert _same(sc.assemble(z["traces"], present, z["centres"], k0, k1, N, bin_hz, z["grid"]), want)
    assert _same(sc.interp_spelled(z["grid"], xp, z["traces"].reshape(-1)), want)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "datasources")), reason="the reference tree is not here")
def test_live_differential_against_the_reference_class(tmp_path):
    """The generator run afresh against the reference's HackRFSweepDataSource._parse: the same file as the committed one."""
    out = str(tmp_path / "sweep_live.npz")
    env = dict(os.environ, TDSA_REFERENCE=REF, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_sweep.py"), out],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    live, gold = np.load(out), np.load(GOLDEN)
    assert sorted(live.files) == sorted(gold.files)
    for k in gold.files:
        assert _same(live[k], gold[k]), k
    _, fs, N, k0, k1, bin_hz, *_ = _golden()
    present = np.ones(len(live["centres"]), dtype=bool)
    assert _same(sc.assemble(live["traces"], present, live["centres"], k0, k1, N, bin_hz, live["grid"]),
                 live["full_power_array"])


def test_detector_restatement():
    rng = np.random.default_rng(5)
    rows = (-80 + 10 * rng.standard_normal((5, 64))).astype(np.float32)
    rows[1, 10] = np.nan
    rows[:, 11] = -np.inf
    rows[2, 12] = -np.inf
    assert _same(sc.detector(rows, 3, 40, "sample"), rows[4, 3:40])
    mx, mn, av = (sc.detector(rows, 3, 40, d) for d in ("max", "min", "avg"))
    assert np.isnan(mx[7]) and np.isnan(mn[7]) and np.isnan(av[7])
    assert mx[8] == -np.inf and av[8] == -300.0                    # no power at all: the 1e-30 floor
    assert np.isclose(av[9], 10 * np.log10(np.sum(10 ** (rows[[0, 1, 3, 4], 12].astype(np.float64) / 10)) / 5))
    one = sc.detector(rows[:1], 0, 64, "avg")
    finite = np.isfinite(rows[0])
    assert np.allclose(one[finite], rows[0, finite].astype(np.float64), rtol=0, atol=1e-9) and one[11] == -300.0


# ---------------------------------------------------------------------------------------------------- planning
@pytest.mark.parametrize("start,stop,fs,N,keep", [(0.0, 6e9, 20e6, 8192, 0.75), (100e6, 130e6, 8.192e6, 4096, 0.75),
                                                  (88e6, 108e6, 2.4e6, 1024, 0.5), (433e6, 434e6, 2.048e6, 2048, 1.0)])
def test_plan_steps_covers_the_span(start, stop, fs, N, keep):
    centres, (k0, k1), bin_hz = plan_steps(start, stop, fs, N, keep)
    K = k1 - k0
    assert bin_hz == 1.0 / (N * (1.0 / fs))
    assert K % 2 == 0 and K <= keep * N < K + 2 and k0 + K // 2 == N // 2 and 0 <= k0 < k1 <= N
    assert centres.dtype == np.float64 and np.all(np.diff(centres) > 0)
    if (start, stop, fs, N) == (0.0, 6e9, 20e6, 8192):
        assert centres.size == 400 and K == 6144
    xp = step_frequencies(centres, k0, k1, N, bin_hz)
    assert _same(xp, sc.frequencies(centres, k0, k1, N, bin_hz))
    for s in (0, centres.size // 2, centres.size - 1):              # the axis of a tuned capture, bit for bit
        axis = np.fft.fftshift(np.fft.fftfreq(N, 1 / fs)) + centres[s]
        assert _same(xp[s * K:(s + 1) * K], axis[k0:k1])
    assert np.all(np.diff(xp) > 0)
    check_geometry(centres, k0, k1, N, bin_hz)
    # abutting kept ranges: one bin from the last bin of a step to the first of the next, the span covered bin by bin
    assert np.allclose(np.diff(xp), bin_hz, rtol=1e-6)
    assert abs(xp[0] - start) <= 1e-6 * bin_hz and xp[-1] + bin_hz >= stop - 1e-6 * bin_hz
    assert xp[-1] - K * bin_hz < stop                               # and not a step more than that


def test_plan_steps_refuses_nonsense():
    for bad in ((1e6, 1e6, 2e6, 1024, 0.75), (0, 1e6, 0, 1024, 0.75), (0, 1e6, 2e6, 1023, 0.75), (0, 1e6, 2e6, 1024, 0.0),
                (0, 1e6, 2e6, 1024, 1.5), (0, 6e9, 20e3, 1024, 0.75)):
        with pytest.raises(ValueError):
            plan_steps(*bad)


def test_overlapping_or_descending_steps_are_refused():
    centres, (k0, k1), bin_hz = plan_steps(100e6, 130e6, 8.192e6, 4096)
    K, grid = k1 - k0, np.linspace(100e6, 130e6, 500)
    check_geometry(centres, k0, k1, 4096, bin_hz)
    cases = {"descending": centres[::-1], "overlap by one bin": centres - np.arange(centres.size) * bin_hz,
             "equal": np.array([1e8, 1e8]), "not finite": np.array([1e8, np.nan])}
    for name, c in cases.items():
        with pytest.raises(ValueError):
            check_geometry(c, k0, k1, 4096, bin_hz)
        with pytest.raises(ValueError):                              # before any handle exists: no device needed
            SweepAssembler(4096, c, (k0, k1), bin_hz, grid)
    check_geometry(centres + np.arange(centres.size) * bin_hz, k0, k1, 4096, bin_hz)   # gaps are fine
    for k in ((-1, 10), (10, 10), (10, 4097)):
        with pytest.raises(ValueError):
            check_geometry(centres, k[0], k[1], 4096, bin_hz)
    with pytest.raises(ValueError):
        check_geometry(centres, k0, k1, 4096, 0.0)
    with pytest.raises(ValueError):
        SweepAssembler(4096, centres, (k0, k1), bin_hz, [1e8])


# ---------------------------------------------------------------------------------------------------- peak cells
def test_peak_cell_rule_on_hand_made_cases():
    xp = np.array([10.0, 11.0, 12.0, 13.0, 20.0, 21.0])
    fp = np.array([1.0, 5.0, 2.0, 7.0, 3.0, 4.0], dtype=np.float32)
    grid = np.array([10.0, 12.0, 14.0, 16.0, 18.0, 20.0, 22.0])       # h = 2: cell i is [grid - 1, grid + 1)
    out = sc.stitch(grid, xp, fp, "peak")
    #  [9,11) -> {10}; [11,13) -> {11,12}; [13,15) -> {13}; [15,17) and [17,19) empty -> interp; [19,21) -> {20}; [21,23) -> {21}
    want = np.array([1.0, 5.0, 7.0, np.interp(16.0, xp, fp), np.interp(18.0, xp, fp), 3.0, 4.0])
    assert _same(out, want)
    assert want[3] == 7.0 + (3.0 - 7.0) / 7.0 * 3.0
    fp_nan = fp.copy()
    fp_nan[2] = np.nan
    out = sc.stitch(grid, xp, fp_nan, "peak")
    assert np.isnan(out[1]) and _same(out[[0, 2, 5, 6]], want[[0, 2, 5, 6]])
    # the lower bound belongs to the cell, the upper does not
    out = sc.stitch(np.array([11.5, 12.5]), np.array([11.0, 12.0, 13.0]), np.array([9.0, 1.0, 8.0]), "peak")
    assert _same(out, np.array([9.0, 1.0]))
    # a grid finer than the bins: every cell without a bin interpolates
    fine = np.linspace(10.0, 13.0, 31)
    out, lin = sc.stitch(fine, xp, fp, "peak"), np.interp(fine, xp, fp)
    has_bin = np.array([np.any((xp >= g - 0.5 * (fine[1] - fine[0])) & (xp < g + 0.5 * (fine[1] - fine[0]))) for g in fine])
    assert _same(out[~has_bin], lin[~has_bin]) and has_bin.sum() == 4
    assert np.isnan(sc.stitch(grid, np.empty(0), np.empty(0), "peak")).all()
    assert np.isnan(sc.stitch(grid, np.empty(0), np.empty(0), "interp")).all()


# ---------------------------------------------------------------------------------------------------- the kernels
def test_sweep_kernels_compile_scratch_free():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/tdsa_sweep.o" in mk and re.search(r"^CAPI\s*=.*\bsweep\b", mk, re.M)
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "tdsa_sweep.hip", "-o", os.devnull]
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
    names = [k for k in kernels if "sweep_" in k]
    assert len(names) == 5, sorted(kernels)                          # four detectors and the stitch
    for k in names:
        assert kernels[k]["ScratchSize [bytes/lane]"] == "0", (k, kernels[k])
        assert kernels[k].get("VGPRs Spill", "0") == "0", (k, kernels[k])
        assert int(kernels[k]["LDS Size [bytes/block]"]) <= 64 * 1024, (k, kernels[k])
    # the stitch takes its step table as dynamic LDS: 16 bytes for each of at most 4096 steps
    assert 4096 * 16 <= 64 * 1024


# ---------------------------------------------------------------------------------------------------- the shapes suite
def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, "tdsa_sweep.hip")).read()).group(1))


def _differs(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def test_inputs_of_the_shapes_suite_discriminate():
    """The CPU half of tests/test_gpu_sweep_shapes.py: the cases reach every path of the two kernels, and on the very
    arrays the GPU half feeds every mutant of tests/sweep_contract.py gives another result than the contract."""
    block, batch = _const("kDetBlock"), _const("kDetBatch")
    sblock, smax = _const("kStitchBlock"), _const("kStitchMaxBlocks")
    Fs = sc.frame_counts(batch)
    if batch == 8:
        assert Fs == (1, 2, 7, 8, 9, 10, 16, 17, 25)
    cases = sc.detector_cases(block, batch)
    assert len(cases) == len(set(cases)) <= 40

    # ---- the detector cases reach what they are for
    quads = [c for c in cases if sc.takes_quads(c[0], *c[3:])]
    wide = [c for c in quads if c[2] - c[1] > 2 * 4 * block]
    assert {(k0 % 4, k1 % 4) for _, k0, k1, *_ in wide} == {(a, b) for a in range(4) for b in range(4)}
    for N, k0, k1, *_ in wide:
        assert ((k1 + 3) // 4 - k0 // 4 + block - 1) // block >= 3          # workgroups in x, as the launch counts them
    assert {c[3] for c in wide} == set(Fs)
    assert any(k0 == 0 and k1 == N for N, k0, k1, *_ in wide)
    small = {(k0, k1) for N, k0, k1, *_ in quads if N <= 64}
    assert {k1 - k0 for k0, k1 in small if k0 // 4 == (k1 - 1) // 4} >= {1, 2, 3}
    assert any(k1 - k0 == 2 and k0 // 4 != (k1 - 1) // 4 for k0, k1 in small)
    assert any(k1 - k0 == 4 and k0 % 4 == 0 for k0, k1 in small)
    scalar = [c for c in cases if not sc.takes_quads(c[0], *c[3:])]
    assert {c[3] for c in scalar} == set(Fs) and all(k1 - k0 > 4 * block for _, k0, k1, *_ in scalar)
    alone = lambda N, F, pad, off: ((off % 16 != 0) + (N % 4 != 0) + ((F * N + pad) % 4 != 0 and N % 4 == 0)) == 1
    assert all(alone(N, F, pad, off) for N, _, _, F, pad, off in scalar)
    assert {off for *_, pad, off in scalar if off} == {4, 8, 12} and {pad for *_, pad, off in scalar if pad} == {1, 2, 3}
    assert any(N % 4 for N, *_ in scalar)

    # ---- on their rows every mutant shows
    for i, (N, k0, k1, F, pad, off) in enumerate(cases):
        S, K = sc.case_steps(N), k1 - k0
        rows, special = sc.spiky_rows(S, F, N, seed=i)
        level = sc.level_rows(S, F, N, seed=i)
        buf, stride = sc.lay_out(rows, pad, off)
        assert stride == F * N + pad and buf.size == off // 4 + S * stride
        assert np.array_equal(buf[off // 4:].reshape(S, stride)[:, :F * N].reshape(S, F, N), rows, equal_nan=True)
        assert (buf == sc.SENTINEL).sum() == off // 4 + S * pad and not (rows == 0).any()
        b = np.arange(N)
        for s in range(S):
            plain = rows[s][~special[s]]
            assert np.unique(plain).size == plain.size                       # all distinct
            clean = ~special[s].any(axis=0)
            assert clean.sum() > 0.3 * N or N <= 64
            assert np.array_equal(np.argmax(rows[s][:, clean], axis=0), ((b + s) % F)[clean])
            assert F == 1 or np.array_equal(np.argmin(rows[s][:, clean], axis=0), ((b + s + 1) % F)[clean])
            for det in ("sample", "max", "min"):
                want = sc.detector(rows[s], k0, k1, det)
                if K > 4 * block + 8:
                    assert _differs(want, sc.detector_quad_shifted(rows[s], k0, k1, det, 4 * block)).any(), (i, det)
            if K > 4 * block and F > 1:               # every frame holds the maximum of many kept bins and the minimum of others
                for det in ("max", "min"):
                    want = sc.detector(rows[s], k0, k1, det)
                    for f in range(F):
                        assert _differs(want, sc.detector_skipping(rows[s], k0, k1, det, f)).any(), (i, det, f)
            if F > 1:
                assert _differs(sc.detector(rows[s], k0, k1, "sample"),
                                sc.detector_skipping(rows[s], k0, k1, "sample", F - 1)).any(), i
            # avg: the level rows; a frame left out moves every kept bin by ten times the allowance or more
            want = sc.detector(level[s], k0, k1, "avg")
            assert np.isfinite(want).all()
            lv = level[s][:, k0:k1]
            assert (lv.max(axis=0) - lv.min(axis=0)).max() <= 6.0
            for f in range(F):
                moved = np.abs(sc.detector_skipping(level[s], k0, k1, "avg", f) - want)
                assert moved.min() >= 10 * sc.AVG_BOUND_DB, (i, f, float(moved.min()))
            if K > 4 * block + 8:
                moved = np.abs(sc.detector_quad_shifted(level[s], k0, k1, "avg", 4 * block) - want)[4 * block:-4]
                assert (moved >= 10 * sc.AVG_BOUND_DB).mean() > 0.9
    # the special values come out as the contract says
    sp = sc.special_rows(2, 9, 64, seed=1)
    mx, mn, av, sm = (sc.detector(sp[0], 0, 64, d) for d in ("max", "min", "avg", "sample"))
    for pattern in (0, 1, 2, 3, 11):
        assert np.isnan(mx[pattern]) and np.isnan(mn[pattern]) and np.isnan(av[pattern])
    assert np.isnan(sm[1]) and np.isnan(sm[3]) and not np.isnan(sm[0]) and not np.isnan(sm[2])
    assert av[4] == -300.0 and mx[4] == -np.inf and np.isfinite(av[5]) and mn[5] == -np.inf and np.isfinite(mx[6])
    assert abs(av[7] - 299.0) < 1e-9 and abs(av[8] + 299.0) < 1e-9 and mx[9] == 299.0 and mn[10] == -299.0
    assert np.isfinite(av[12:16]).all() and np.isnan(av).sum() == 5 * 4

    # ---- the stitch cases
    stitch_cases = sc.stitch_cases(sblock)
    reached, long_seen = set(), 0
    for name, tag, grid_tag in stitch_cases:
        N, k0, k1, bin_hz, centres, T, present, grid = sc.stitch_inputs(name, tag, grid_tag, sblock, smax)
        K = k1 - k0
        assert bin_hz == 1.0 / (N * (1.0 / 1e6)) and np.all(np.isfinite(grid)) and np.all(np.diff(grid) > 0)
        assert grid[1] - grid[0] > 0 and grid.size <= max(60000, sblock * smax + sblock + 1)
        xp = sc.frequencies(centres[present], k0, k1, N, bin_hz)
        fp = T[present].reshape(-1)
        assert xp[0] == 0.0 or not present[0]
        assert np.all(np.diff(sc.frequencies(centres, k0, k1, N, bin_hz)) > 0)
        reached.add(int(present.sum()))
        if grid_tag == "long":
            long_seen = max(long_seen, grid.size)
            continue
        assert grid[0] < xp[0] and (grid[-1] > xp[-1] or grid_tag.startswith("cells"))
        if grid_tag == "ulp":
            assert grid[1] < xp[0] and grid[-2] > xp[-1]
            on, below, above = np.isin(grid, xp), np.isin(grid, np.nextafter(xp, -np.inf)), np.isin(grid, np.nextafter(xp, np.inf))
            assert on.sum() == below.sum() == above.sum() >= min(xp.size, 8000)
            if present.sum() > sblock:                   # a table cut at the first round of its load shows, in both modes
                for mode in ("interp", "peak"):
                    want = sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, mode)
                    assert _differs(want, sc.assemble_table_cut(T, present, centres, k0, k1, N, bin_hz, grid, mode, sblock)).any()
        if grid_tag.startswith("cells"):
            h = grid[1] - grid[0]
            assert abs(h / bin_hz - (8.0 if grid_tag == "cells8" else 3.5 * K)) < 1e-6
            lower_on, upper_on = np.isin(grid - 0.5 * h, xp), np.isin(grid + 0.5 * h, xp)
            assert lower_on.sum() >= 30 and upper_on.sum() >= 30, (name, tag, grid_tag)
            want = sc.stitch(grid, xp, fp, "peak")
            assert _differs(want, sc.stitch_upper_closed(grid, xp, fp)).sum() >= 5, (name, tag, grid_tag)
            assert np.isfinite(want).sum() >= 30
    assert {sblock - 1, sblock, sblock + 1, 4096} <= reached and long_seen > sblock * smax
    assert {(n, g) for n, _, g in stitch_cases} >= {(n, g) for n in ("inexact", "k1", "k2", "k3") for g in ("ulp", "cells8", "cellswide")}

    # ---- the inexact geometry: one rounding or two, a guess or the exact expression
    N, k0, k1, bin_hz, centres, T, present, grid = sc.stitch_inputs("inexact", "all", "ulp", sblock, smax)
    K = k1 - k0
    assert bin_hz * N != 1e6 or bin_hz != np.round(bin_hz)                 # 1302.0833...: not a number of Hz
    xp, fp = sc.frequencies(centres, k0, k1, N, bin_hz), T.reshape(-1).astype(np.float64)
    fused = sc.frequencies_fused(centres, k0, k1, N, bin_hz)
    assert (fused != xp).sum() >= 100 and np.max(np.diff(xp)) > 30 * bin_hz
    assert _differs(sc.stitch(grid, xp, fp, "interp"), sc.stitch(grid, fused, fp, "interp")).sum() >= 100
    cells = sc.stitch_inputs("inexact", "all", "cells8", sblock, smax)[7]   # cell edges on the bins: there peak shows it
    assert _differs(sc.stitch(cells, xp, fp, "peak"), sc.stitch(cells, fused, fp, "peak")).sum() >= 30
    inside = grid[grid >= xp[0]]
    wrong = sc.locate_by_guess(inside, xp, K, bin_hz) != sc.locate(inside, xp)
    assert wrong.sum() >= 1000
    want = np.interp(grid, xp, fp)
    assert _same(sc.interp_spelled(grid, xp, fp), want)
    guessed = sc.interp_spelled(grid, xp, fp, locator=lambda x: sc.locate_by_guess(np.float64(x), xp, K, bin_hz))
    assert _differs(guessed, want).sum() >= 100
    hit = np.isin(grid, xp)
    assert _same(want[hit], fp[np.searchsorted(xp, grid[hit])])           # a grid point on a bin takes that bin's value


def _err():
    return nat.lib.tdsa_last_error_string().decode()


def test_c_abi_refuses_bad_arguments_without_a_device():
    h = C.c_void_p()
    lib = nat.lib
    assert lib.tdsa_sweep_create(0, 1, 4, 100, C.byref(h)) == ERR_ARG and "nfft" in _err()
    assert lib.tdsa_sweep_create(0, (1 << 20) + 1, 4, 100, C.byref(h)) == ERR_ARG and "nfft" in _err()
    assert lib.tdsa_sweep_create(0, 1024, 0, 100, C.byref(h)) == ERR_ARG and "n_steps" in _err()
    assert lib.tdsa_sweep_create(0, 1024, 4097, 100, C.byref(h)) == ERR_ARG and "n_steps" in _err()
    assert lib.tdsa_sweep_create(0, 1024, 4, 1, C.byref(h)) == ERR_ARG and "n_grid" in _err()
    assert lib.tdsa_sweep_create(0, 1024, 4, (1 << 24) + 1, C.byref(h)) == ERR_ARG and "n_grid" in _err()
    assert lib.tdsa_sweep_create(0, 1024, 4, 100, None) == ERR_ARG and "null" in _err()
    buf = (C.c_double * 64)()
    assert lib.tdsa_sweep_set_geometry(None, buf, 1.0, 0, 4, buf) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_reset(None) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_set_chunk_bytes(None, 1) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_update_dev(None, None, 0, 1, buf, 1, 0, 9) == ERR_ARG and "detector" in _err()
    assert lib.tdsa_sweep_update_dev(None, None, 0, 1, buf, 1, 0, 3) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_run_dev(None, None, 0, buf, 0, 0, 1, 1024, 1024, 1, -1) == ERR_ARG and "detector" in _err()
    assert lib.tdsa_sweep_run_dev(None, None, 0, buf, 0, 0, 1, 1024, 1024, 1, 0) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_read(None, 0, buf, None) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_get_steps(None, buf, buf) == ERR_ARG and "null" in _err()
    assert lib.tdsa_sweep_timer_begin(None) == ERR_ARG and lib.tdsa_sweep_timer_end(None, None) == ERR_ARG
    assert lib.tdsa_sweep_destroy(None) == 0
