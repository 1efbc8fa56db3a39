"""Stepped sweeps on the MI355X: the step detector and the stitch against the float64 restatement of
tests/sweep_contract.py - bit for bit where the contract fixes the bits (sample / max / min, both stitch modes, any split
of the steps into calls, any chunk bound), within the row allowance of 1e-3 dB for the avg detector - and
IqSweepDataSource end to end on a synthetic wide-band scene."""
import ctypes as C
import os
import time
import types

import numpy as np
import pytest

import sweep_contract as sc
from topdogspectrumanalyser_amd import DeviceBuffer, IqSweepDataSource, SpectrumEngine, SweepAssembler, _native as nat, plan_steps
from topdogspectrumanalyser_amd.core.display_data_processor import DataProcessor
from topdogspectrumanalyser_amd.sweep import frequency_grid, step_frequencies
from topdogspectrumanalyser_amd.zoom import zoom_window

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]        # every test under a time limit of its own

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep.npz")
AVG_BOUND_DB = 1e-3          # the project's row allowance (DESIGN.md section 4.9 derives the room it leaves; worst seen 1.8e-5)


def _same(a, b):
    """Bit for bit, any NaN equal to any NaN (and -0.0 not equal to 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)):
        return False
    num = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[num]), np.signbit(b[num])))


def _centres(S, K, bin_hz, start=100e6):
    return start + (np.arange(S) + 0.5) * K * bin_hz


def _rows(rng, S, F, N, stride):
    """[S][stride] float32 with F rows of N dB values each at the front: noise, outliers of the +-300 dB domain, NaN, -inf."""
    buf = np.full((S, stride), 12345.0, dtype=np.float32)
    rows = (-90 + 15 * rng.standard_normal((S, F, N))).astype(np.float32)
    rows[rng.random(rows.shape) < 0.01] = np.nan
    rows[rng.random(rows.shape) < 0.02] = -np.inf
    rows[rng.random(rows.shape) < 0.01] = 299.0
    rows[rng.random(rows.shape) < 0.01] = -299.0
    rows[0, :, 5 % N] = -np.inf                         # a bin without any power at all
    buf[:, :F * N] = rows.reshape(S, F * N)
    return buf, rows


# ---------------------------------------------------------------------------------------------------- the detector
@pytest.mark.parametrize("N,k0,k1,pad", [(256, 0, 256, 0), (256, 3, 53, 0), (256, 37, 38, 0), (1024, 128, 896, 0),
                                         (1024, 129, 900, 8), (1024, 128, 896, 3), (250, 1, 248, 0)])
@pytest.mark.parametrize("F", [1, 2, 11, 16])
def test_update_dev_detectors(N, k0, k1, pad, F):
    rng = np.random.default_rng(N * 1000 + k0 * 10 + F)
    S, K = 3, k1 - k0
    stride = F * N + pad
    buf, rows = _rows(rng, S, F, N, stride)
    centres = _centres(S, K, 1000.0)
    grid = np.linspace(centres[0], centres[-1], 50)
    worst = 0.0
    with SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm, DeviceBuffer(buf.nbytes) as d:
        d.put(buf)
        for det in sc.DETECTORS:
            asm.reset()
            asm.update_device(None, 0, S, d.ptr, F, det, stride)
            T, valid = asm.steps()
            assert valid.all() and T.shape == (S, K)
            for s in range(S):
                want = sc.detector(rows[s], k0, k1, det)
                if det != "avg":
                    assert _same(T[s], want), (det, s)
                    continue
                assert np.array_equal(np.isnan(T[s]), np.isnan(want)), (det, s)
                ok = ~np.isnan(want)
                if not ok.any():
                    continue
                err = np.abs(T[s][ok].astype(np.float64) - want[ok])
                worst = max(worst, float(err.max()))
                print(f"avg detector N={N} [{k0},{k1}) F={F} step {s}: max |dB error| {err.max():.3e}")
                assert err.max() <= AVG_BOUND_DB, (s, float(err.max()))
    print(f"worst avg detector error: {worst:.3e} dB")


def test_update_dev_marks_only_its_steps_and_refuses_bad_calls():
    N, k0, k1, S, F = 256, 32, 224, 5, 2
    rng = np.random.default_rng(1)
    buf, rows = _rows(rng, S, F, N, F * N)
    centres = _centres(S, k1 - k0, 1000.0)
    grid = np.linspace(centres[0], centres[-1], 64)
    with SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm, DeviceBuffer(buf.nbytes) as d:
        d.put(buf)
        assert not asm.steps()[1].any()
        asm.update_device(None, 1, 2, d.at(4 * F * N), F, "max")
        T, valid = asm.steps()
        assert list(valid) == [False, True, True, False, False]
        assert _same(T[1], sc.detector(rows[1], k0, k1, "max")) and _same(T[2], sc.detector(rows[2], k0, k1, "max"))
        for first, n in ((-1, 1), (4, 2), (0, 6)):
            with pytest.raises(nat.TdsaError):
                asm.update_device(None, first, n, d.ptr, F, "max")
        with pytest.raises(nat.TdsaError):
            asm.update_device(None, 0, 1, d.ptr, 0, "max")
        with pytest.raises(nat.TdsaError):
            asm.update_device(None, 0, 1, d.at(2), F, "max")
        # the C-ABI refuses geometry the Python layer would have refused first
        bad = np.ascontiguousarray(centres[::-1])
        rc = nat.lib.tdsa_sweep_set_geometry(asm._h, bad.ctypes.data_as(C.c_void_p), 1000.0, k0, k1,
                                             grid.ctypes.data_as(C.c_void_p))
        assert rc == -1 and "overlap" in nat.lib.tdsa_last_error_string().decode()
        touching = centres - np.arange(S) * 1000.0
        rc = nat.lib.tdsa_sweep_set_geometry(asm._h, touching.ctypes.data_as(C.c_void_p), 1000.0, k0, k1,
                                             grid.ctypes.data_as(C.c_void_p))
        assert rc == -1
        assert list(asm.steps()[1]) == [False, True, True, False, False]      # a refused call changes nothing


# ---------------------------------------------------------------------------------------------------- the stitch
def _load_steps(asm, T, present, N, k0):
    """T[s] of the steps flagged in `present` into the handle, exactly: one frame per step, sample detector."""
    S, K = T.shape
    rows = np.zeros((S, N), dtype=np.float32)
    rows[:, k0:k0 + K] = T
    with DeviceBuffer(rows.nbytes) as d:
        d.put(rows)
        asm.reset()
        for s in np.nonzero(present)[0]:
            asm.update_device(None, int(s), 1, d.at(4 * int(s) * N, 4 * N), 1, "sample")
        got, valid = asm.steps()
    assert np.array_equal(valid, present)
    assert _same(got[present], T[present])


def test_read_equals_the_recorded_reference_sweep():
    z = np.load(GOLDEN)
    fs, N, k0, k1, bin_hz = z["geometry"][:5]
    N, k0, k1 = int(N), int(k0), int(k1)
    T, centres, grid = z["traces"], z["centres"], z["grid"]
    present = np.ones(len(centres), dtype=bool)
    with SweepAssembler(N, centres, (k0, k1), float(bin_hz), grid) as asm:
        assert np.isnan(asm.read("interp")).all() and np.isnan(asm.read("peak")).all()     # before the first step
        _load_steps(asm, T, present, N, k0)
        out = asm.read("interp")
        assert out.dtype == np.float64 and _same(out, z["full_power_array"])
        assert _same(out, sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, "interp"))
        assert _same(asm.read("peak"), sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, "peak"))
        with DeviceBuffer(8 * grid.size) as d:                                   # to a device buffer, no host pointer
            assert asm.read("interp", out_dev=d.ptr, to_host=False) is None
            asm.steps()                                                  # waits for the handle's stream
            assert _same(d.get(grid.size, np.float64), out)
        asm.reset()
        assert np.isnan(asm.read("interp")).all() and np.isnan(asm.read("peak")).all()


def _grids(xp, bin_hz, rng):
    lo, hi = xp[0], xp[-1]
    beyond = np.linspace(lo - 40.5 * bin_hz, hi + 77.25 * bin_hz, 4001)
    on_bins = np.sort(np.concatenate([xp[rng.integers(0, xp.size, 300)], [xp[0], xp[-1]],
                                      rng.uniform(lo, hi, 300)]))
    on_bins = np.unique(on_bins)
    coarse = np.linspace(lo - 3.0 * bin_hz, hi + 3.0 * bin_hz, 301)           # many bins per cell
    coarse_aligned = lo + 8.0 * bin_hz * np.arange(-2, (hi - lo) / (8.0 * bin_hz) + 3)   # cell edges exactly on bins
    between_bins = lo + 0.5 * bin_hz + 8.0 * bin_hz * np.arange(0, 200)       # cell edges half-way between bins
    fine = np.linspace(lo - bin_hz, lo + 60 * bin_hz, 1500)                  # finer than the bins: mostly empty cells
    return {"beyond": beyond, "on_bins": on_bins, "coarse": coarse, "coarse_aligned": coarse_aligned,
            "between_bins": between_bins, "fine": fine}


@pytest.mark.parametrize("case", ["all", "missing", "first_and_last_missing", "one_step"])
def test_read_both_modes_bit_exact(case):
    rng = np.random.default_rng(11)
    fs, N = 8.192e6, 1024
    centres, (k0, k1), bin_hz = plan_steps(400e6, 448e6, fs, N, 0.75)
    centres = centres.copy()
    centres[4:] += 1.0e6                                                 # a gap between steps 3 and 4
    S, K = centres.size, k1 - k0
    T = (-95 + 12 * rng.standard_normal((S, K))).astype(np.float32)
    T[rng.random(T.shape) < 0.003] = np.nan
    T[rng.random(T.shape) < 0.003] = np.inf
    T[rng.random(T.shape) < 0.003] = -np.inf
    T[1, K - 1] = np.nan                                                 # NaN next to a step boundary
    T[2, 0] = np.inf
    T[3, K - 1] = -np.inf                                                # ... and next to the gap
    present = np.ones(S, dtype=bool)
    if case == "missing":
        present[[2, 5]] = False
    elif case == "first_and_last_missing":
        present[[0, S - 1]] = False
    elif case == "one_step":
        present[:] = False
        present[3] = True
    xp_all = step_frequencies(centres, k0, k1, N, bin_hz)
    for name, grid in _grids(xp_all, bin_hz, rng).items():
        with SweepAssembler(N, centres, (k0, k1), bin_hz, grid) as asm:
            _load_steps(asm, T, present, N, k0)
            for mode in ("interp", "peak"):
                got = asm.read(mode)
                want = sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, mode)
                bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
                assert bad.size == 0, (name, mode, bad[:5], got[bad[:5]], want[bad[:5]])
                assert _same(got, want), (name, mode)
            if name == "on_bins":                                        # a grid point equal to a bin takes that bin
                xp = sc.frequencies(centres[present], k0, k1, N, bin_hz)
                hit = np.isin(grid, xp)
                assert hit.sum() >= 30
                assert _same(asm.read("interp")[hit], T[present].reshape(-1)[np.searchsorted(xp, grid[hit])].astype(np.float64))


def test_peak_needs_an_ascending_grid():
    centres, (k0, k1), bin_hz = plan_steps(100e6, 104e6, 2.048e6, 256)
    grid = np.linspace(104e6, 100e6, 100)
    with SweepAssembler(256, centres, (k0, k1), bin_hz, grid) as asm:
        assert np.isnan(asm.read("interp")).all()
        with pytest.raises(nat.TdsaError):
            asm.read("peak")


# ---------------------------------------------------------------------------------------------------- from raw IQ
def _engine(N, F):
    e = SpectrumEngine(N, max_frames=F)
    e.set_window(zoom_window(N))
    e.configure(db_mode="mag", log_floor=1e-12, dc_alpha=-1.0)
    return e


@pytest.mark.parametrize("fmt", ["i8", "c64"])
def test_run_dev_any_split_any_chunk_same_bits(fmt):
    rng = np.random.default_rng(3)
    N, F, hop, S = 1024, 3, 512, 7
    n_per = (F - 1) * hop + N
    centres, (k0, k1), bin_hz = plan_steps(100e6, 100e6 + S * 768 * 2000.0, 2.048e6, N)
    assert centres.size == S
    grid = frequency_grid(100e6, centres[-1] + 1e6, 1500)
    if fmt == "i8":
        iq, in_format, stride = rng.integers(-128, 128, (S, 2 * n_per + 6)).astype(np.int8), nat.IN_I8, 2 * n_per + 6
    else:
        iq = ((rng.standard_normal((S, n_per + 1)) + 1j * rng.standard_normal((S, n_per + 1))) * 0.2).astype(np.complex64)
        in_format, stride = nat.IN_C64, 8 * (n_per + 1)
    with _engine(N, F) as eng, DeviceBuffer(iq.nbytes) as d_iq, DeviceBuffer(4 * S * F * N) as d_rows, \
            SweepAssembler(N, centres, (k0, k1), bin_hz, grid) as asm:
        d_iq.put(iq)
        # the parent's path plus the detector: rows of all steps, then one update
        eng.process_device_batch(in_format, d_iq.ptr, stride, S, n_per, hop, F, d_rows.ptr)
        eng.synchronize()
        rows = d_rows.get(S * F * N, np.float32).reshape(S, F, N)
        assert np.isfinite(rows).all()
        results = {}
        for det in sc.DETECTORS:
            asm.reset()
            asm.update_device(eng, 0, S, d_rows.ptr, F, det)
            ref_T = asm.steps()[0]
            ref_out = {m: asm.read(m) for m in ("interp", "peak")}
            for s in range(S):
                want = sc.detector(rows[s], k0, k1, det)
                if det == "avg":
                    assert np.max(np.abs(ref_T[s] - want)) <= AVG_BOUND_DB
                else:
                    assert _same(ref_T[s], want)
            for m in ("interp", "peak"):
                assert _same(ref_out[m], sc.assemble(ref_T, np.ones(S, bool), centres, k0, k1, N, bin_hz, grid, m))
            # any split of the steps into update calls, in any order
            for cuts in ([(4, 3), (0, 4)], [(6, 1), (0, 1), (1, 5)], [(s, 1) for s in range(S)]):
                asm.reset()
                for first, n in cuts:
                    asm.update_device(eng, first, n, d_rows.at(4 * first * F * N, 4 * n * F * N), F, det)
                assert _same(asm.steps()[0], ref_T), (det, cuts)
                assert _same(asm.read("interp"), ref_out["interp"])
            # run_dev: one call, any chunk bound, any split
            step_bytes = 4 * F * N
            for bound, cuts in ((1 << 28, [(0, S)]), (1, [(0, S)]), (2 * step_bytes, [(0, S)]),
                                (3 * step_bytes + 5, [(0, S)]), (2 * step_bytes, [(3, 4), (0, 3)])):
                asm.reset()
                asm.set_chunk_bytes(bound)
                for first, n in cuts:
                    asm.run_device(eng, in_format, d_iq.at(first * stride), stride, first, n, n_per, hop, F, det)
                assert _same(asm.steps()[0], ref_T), (det, bound, cuts)
                for m in ("interp", "peak"):
                    assert _same(asm.read(m), ref_out[m]), (det, bound, cuts, m)
            results[det] = ref_T
        assert not _same(results["max"], results["min"])
        with pytest.raises(nat.TdsaError):
            asm.run_device(eng, 7, d_iq.ptr, stride, 0, S, n_per, hop, F, "max")
        with _engine(2 * N, F) as other, pytest.raises(nat.TdsaError):
            asm.run_device(other, in_format, d_iq.ptr, stride, 0, S, n_per, hop, F, "max")


# ---------------------------------------------------------------------------------------------------- end to end
FS, NFFT = 2.048e6, 1024
START, STOP, BIN_SIZE = 430_000_000, 442_000_000, 2000
TONES = [(430_512_000.0, 0.5), (433_920_000.0, 0.25), (436_001_000.0, 0.4), (439_777_000.0, 0.1), (441_700_500.0, 0.3)]


def _scene(centre_hz, n):
    """What a tuner at centre_hz would deliver: the tones within its band, and a little noise."""
    rng = np.random.default_rng(int(centre_hz) % (1 << 31))
    t = np.arange(n) / FS
    x = 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in TONES:
        if abs(f - centre_hz) < 0.45 * FS:
            x = x + a * np.exp(2j * np.pi * (f - centre_hz) * t)
    return x.astype(np.complex64)


def _source(**kw):
    return IqSweepDataSource(START, STOP, BIN_SIZE, capture=_scene, sample_rate=FS, nfft=NFFT, **kw)


@pytest.mark.parametrize("detector,frames,hop", [("max", 4, 512), ("avg", 5, 1024), ("sample", 1, None)])
def test_sweep_once_end_to_end(detector, frames, hop):
    src = _source(frames_per_step=frames, hop=hop, detector=detector)
    try:
        assert np.isnan(src.get_data()).all() and src.get_number_of_points() == (STOP - START) // BIN_SIZE
        assert _same(src.frequency_grid, np.linspace(START, STOP, (STOP - START) // BIN_SIZE))
        trace = src.sweep_once()
        assert _same(src.get_data(), trace) and src.get_data() is not src.get_data()
        assert trace.dtype == np.float64 and np.isfinite(trace).all() and src.sweep_rate > 0
        grid, cell = src.frequency_grid, src.frequency_grid[1] - src.frequency_grid[0]
        for f, a in TONES:                                               # every tone within one grid cell of its place
            near = np.nonzero(np.abs(grid - f) <= 40 * cell)[0]
            peak = near[np.argmax(trace[near])]
            assert abs(grid[peak] - f) <= cell, (f, grid[peak])
            assert trace[peak] > np.median(trace) + 40.0
        # the same from the engine's own rows of those captures, through the contract
        S, n_per = src.centres.size, src.n_samples_per_step
        k0, k1 = src.kept
        with DeviceBuffer(4 * S * frames * NFFT) as d_rows:
            src.engine.process_device_batch(nat.IN_C64, src._d_in.ptr, 8 * n_per, S, n_per, src.hop, frames, d_rows.ptr)
            src.engine.synchronize()
            rows = d_rows.get(S * frames * NFFT, np.float32).reshape(S, frames, NFFT)
        T_dev = src.assembler.steps()[0]
        T = np.stack([sc.detector(rows[s], k0, k1, detector) for s in range(S)])
        if detector == "avg":
            assert np.max(np.abs(T_dev - T)) <= AVG_BOUND_DB
            T = T_dev                                                    # the stitch is exact on the device's own T
        else:
            assert _same(T_dev, T)
        assert _same(trace, sc.assemble(T, np.ones(S, bool), src.centres, k0, k1, NFFT, src.bin_hz, grid))
    finally:
        src.close()


def test_data_processor_takes_the_source():
    class Span:
        start, stop = float(START), float(STOP)

        def set_start_stop(self, a, b):
            self.start, self.stop = a, b

    src = _source(frames_per_step=2, detector="max")
    try:
        mw = types.SimpleNamespace(current_source=src, frequency=Span(), calibration_manager=None,
                                   source_manager=types.SimpleNamespace(last_source_type=None), live_power_levels=None,
                                   max_power_levels=None, min_power_levels=None, frequency_bins=None, min_hold_enabled=False,
                                   frequency_manager=types.SimpleNamespace(update_frequency_values=lambda: None))
        dm = types.SimpleNamespace(max_peak_search_enabled=False, peak_list_enabled=False)
        dp = DataProcessor.__new__(DataProcessor)
        dp.mw, dp.dm, dp._fused, dp._sweeps_since_axis_refresh, dp.reference_hold_alias = mw, dm, None, 0, False
        dp._sweep_averager = types.SimpleNamespace(is_active=False)
        dp._process_sweep_data()                                         # all NaN before the first sweep: nothing shown
        assert mw.live_power_levels is None
        trace = src.sweep_once()
        dp._process_sweep_data()
        assert _same(np.asarray(mw.live_power_levels, dtype=np.float64), trace)
        assert _same(mw.frequency_bins, src.frequency_grid)
    finally:
        src.close()


def test_start_stop_thread_completes_a_sweep_and_joins():
    src = _source(frames_per_step=2, detector="avg")
    try:
        span = types.SimpleNamespace(start=432_000_000, stop=438_000_000)
        src.start(span)
        assert src.start_freq == span.start and src.get_number_of_points() == (span.stop - span.start) // BIN_SIZE
        deadline = time.monotonic() + 60.0
        while src.sweep_count < 2 and time.monotonic() < deadline:
            time.sleep(0.01)
        assert src.sweep_count >= 1 and src.is_running
        thread = src.thread
        src.stop()
        assert not thread.is_alive() and not src.is_running and src.thread is None
        trace = src.get_data()
        assert np.isfinite(trace).all() and trace.size == src.frequency_grid.size
        f, cell = 433_920_000.0, src.frequency_grid[1] - src.frequency_grid[0]
        near = np.nonzero(np.abs(src.frequency_grid - f) <= 40 * cell)[0]
        assert abs(src.frequency_grid[near[np.argmax(trace[near])]] - f) <= cell
    finally:
        src.close()
