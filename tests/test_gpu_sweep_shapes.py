"""The sweep assembler on the MI355X at the shapes its first tests never launched (tdsa_sweep.hip, DESIGN.md section
4.9), against tests/sweep_contract.py: the detector across workgroup seams, at every ragged end, every frame count around
its batches, on each cause of its bin-by-bin path and with a step stride past 2^32 bytes; the stitch with more steps
than one round of its table load, at the 4096 steps of the limit, on grids one ulp either side of every bin, with
cell edges on the bins and with more points than one round of its lanes; the present set changing between reads; and
every refusal of a live handle with its text.  tests/test_sweep_host.py proves on the CPU that these inputs tell a right
kernel from the wrong ones."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sweep_contract as sc
from device_room import room_or_skip
from kernel_build import CSRC
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, SweepAssembler, _native as nat

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]        # every test under a time limit of its own


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, "tdsa_sweep.hip")).read()).group(1))


DET_BLOCK, DET_BATCH = _const("kDetBlock"), _const("kDetBatch")
STITCH_BLOCK, STITCH_MAX_BLOCKS = _const("kStitchBlock"), _const("kStitchMaxBlocks")
DET_CASES = sc.detector_cases(DET_BLOCK, DET_BATCH)
STITCH_CASES = sc.stitch_cases(STITCH_BLOCK)
ERR_ARG, ERR_STATE = -1, -3


def _same(a, b):
    """Bit for bit, any NaN equal to any NaN (and -0.0 not equal to 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)):
        return False
    num = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[num]), np.signbit(b[num])))


def _first_bad(got, want):
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    return bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]]


def _geometry(S, K, bin_hz=1000.0):
    """Centres of S abutting steps and a small grid: the detector tests do not look at the stitch."""
    centres = 100e6 + (np.arange(S) + 0.5) * K * bin_hz
    return centres, np.linspace(centres[0], centres[-1] + 1.0, 16)


def _avg_error(got, want, tag):
    """max |dB error| of an avg result against the float64 formula; the NaN positions must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------- the detector
def _check_detectors(asm, d, lead_bytes, stride, F, k0, k1, families, guard):
    """Steps [1, 1 + S) of a handle of S + 2 steps updated from the buffer in d, for every detector on the rows it is
    for (families: pairs of detector and rows [S][F][N]); steps 0 and S + 1 hold `guard` and must keep it.  The worst
    avg error."""
    S = families[0][1].shape[0]
    worst = 0.0
    for det, rows in families:
        asm.reset()
        d.put(sc.lay_out(rows, stride - F * rows.shape[2], lead_bytes)[0])
        asm.update_device(None, 1, S, d.at(lead_bytes), F, det, stride)
        T, valid = asm.steps()
        assert list(valid) == [False] + [True] * S + [False], det
        assert _same(T[0], guard[0]) and _same(T[S + 1], guard[1]), det     # the neighbours' rows are as they were
        for s in range(S):
            want = sc.detector(rows[s], k0, k1, det)
            if det != "avg":
                assert _same(T[1 + s], want), (det, s) + _first_bad(T[1 + s], want)
            else:
                err = _avg_error(T[1 + s], want, (det, s))
                worst = max(worst, err)
                assert err <= sc.AVG_BOUND_DB, (s, err)
    return worst


def _detector_case(N, k0, k1, F, pad, byte_offset, seed, special=False):
    S, K = sc.case_steps(N), k1 - k0
    if special:
        rows = sc.special_rows(S, F, N, seed)
        families = [(det, rows) for det in sc.DETECTORS]
    else:
        spiky = sc.spiky_rows(S, F, N, seed)[0]
        families = [(det, spiky) for det in ("sample", "max", "min")] + [("avg", sc.level_rows(S, F, N, seed))]
    stride = F * N + pad
    centres, grid = _geometry(S + 2, K)
    rng = np.random.default_rng(seed + 1000)
    guard_rows = (-50 + rng.standard_normal((2, N))).astype(np.float32)
    with SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm, DeviceBuffer(byte_offset + 4 * S * stride) as d:
        assert d.ptr % 16 == 0
        d.put(guard_rows)                                                    # the guards, through the sample detector
        for i, step in enumerate((0, S + 1)):
            asm.update_device(None, step, 1, d.at(4 * i * N), 1, "sample")
        guard = guard_rows[:, k0:k1]
        assert _same(asm.steps()[0][[0, S + 1]], guard)                      # steps() waits: the buffer is free again
        worst = _check_detectors(asm, d, byte_offset, stride, F, k0, k1, families, guard)
    print(f"avg detector N={N} [{k0},{k1}) F={F} pad={pad} offset={byte_offset}: worst |dB error| {worst:.3e}")
    return worst


@pytest.mark.parametrize("N,k0,k1,F,pad,byte_offset", DET_CASES)
def test_detectors_at_every_shape(N, k0, k1, F, pad, byte_offset):
    """sample / max / min bit for bit on the spiky rows, avg within the row allowance on the level rows."""
    _detector_case(N, k0, k1, F, pad, byte_offset, seed=DET_CASES.index((N, k0, k1, F, pad, byte_offset)))


@pytest.mark.parametrize("N,k0,k1,F,pad,byte_offset", [(16 * DET_BLOCK, 1, 16 * DET_BLOCK - 1, DET_BATCH + 1, 0, 0),
                                                       (8 * DET_BLOCK, 2, 8 * DET_BLOCK - 1, 2 * DET_BATCH + 1, 0, 4),
                                                       (64, 3, 62, 1, 0, 0)])
def test_detectors_on_special_values(N, k0, k1, F, pad, byte_offset):
    """A NaN stays wherever it stands, no power at all gives -300 (avg) and -inf (max, min), +-299 pass through: all
    four detectors, on the quad path and bin by bin."""
    _detector_case(N, k0, k1, F, pad, byte_offset, seed=77, special=True)


@pytest.mark.parametrize("pad", [0, 1])
def test_any_split_of_a_wide_shape_same_bits(pad):
    N, k0, k1, F, S = 16 * DET_BLOCK, 3, 16 * DET_BLOCK - 2, DET_BATCH + 2, 3
    stride = F * N + pad
    centres, grid = _geometry(S, k1 - k0)
    with SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm, DeviceBuffer(4 * S * stride) as d:
        for det in sc.DETECTORS:
            rows = sc.level_rows(S, F, N, 5) if det == "avg" else sc.spiky_rows(S, F, N, 5)[0]
            d.put(sc.lay_out(rows, pad, 0)[0])
            asm.reset()
            asm.update_device(None, 0, S, d.ptr, F, det, stride)
            whole = asm.steps()[0]
            if det != "avg":
                assert all(_same(whole[s], sc.detector(rows[s], k0, k1, det)) for s in range(S))
            asm.reset()
            for s in reversed(range(S)):
                asm.update_device(None, s, 1, d.at(4 * s * stride), F, det, stride)
            T, valid = asm.steps()
            assert valid.all() and _same(T, whole), det


@pytest.mark.parametrize("extra", [4, 5])
def test_step_stride_past_2_to_32_bytes(extra):
    """Two steps (1 << 30) + 4 floats apart on the quad path, + 5 bin by bin; only the rows used are uploaded."""
    N, k0, k1, F = 16 * DET_BLOCK, 1, 16 * DET_BLOCK - 1, 2
    stride = (1 << 30) + extra
    assert 4 * stride > 1 << 32 and sc.takes_quads(N, F, stride - F * N, 0) == (extra == 4)
    centres, grid = _geometry(2, k1 - k0)
    with room_or_skip(4 * (stride + F * N)) as d, SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm:
        for det in sc.DETECTORS:
            rows = sc.level_rows(2, F, N, 9) if det == "avg" else sc.spiky_rows(2, F, N, 9)[0]
            d.put(rows[0], 0)
            d.put(rows[1], 4 * stride)
            asm.reset()
            asm.update_device(None, 0, 2, d.ptr, F, det, stride)
            T, valid = asm.steps()
            assert valid.all()
            for s in range(2):
                want = sc.detector(rows[s], k0, k1, det)
                if det != "avg":
                    assert _same(T[s], want), (det, s) + _first_bad(T[s], want)
                else:
                    assert _avg_error(T[s], want, (det, s)) <= sc.AVG_BOUND_DB


# ---------------------------------------------------------------------------------------------------- the stitch
def _load_steps(asm, T, present, N, k0):
    """T[s] of the steps flagged in `present` into the handle, exactly: one frame per step, the sample detector, one
    call for every run of present steps."""
    S, K = T.shape
    rows = np.zeros((S, N), dtype=np.float32)
    rows[:, k0:k0 + K] = T
    edges = np.flatnonzero(np.diff(np.concatenate([[0], present.astype(np.int8), [0]])))
    with DeviceBuffer(rows.nbytes) as d:
        d.put(rows)
        asm.reset()
        for first, end in zip(edges[::2], edges[1::2]):
            asm.update_device(None, int(first), int(end - first), d.at(4 * int(first) * N), 1, "sample")
        got, valid = asm.steps()
    assert np.array_equal(valid, present)
    assert _same(got[present], T[present])
    return len(edges) // 2


@functools.lru_cache(maxsize=None)
def _stitch_inputs(name, tag, grid_tag):
    out = sc.stitch_inputs(name, tag, grid_tag, STITCH_BLOCK, STITCH_MAX_BLOCKS)
    for a in out[4:]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name,tag,grid_tag", STITCH_CASES)
def test_read_both_modes_bit_exact(name, tag, grid_tag):
    N, k0, k1, bin_hz, centres, T, present, grid = _stitch_inputs(name, tag, grid_tag)
    xp = sc.frequencies(centres[present], k0, k1, N, bin_hz)
    fp = T[present].reshape(-1).astype(np.float64)
    with SweepAssembler(N, centres, (k0, k1), bin_hz, grid) as asm:
        calls = _load_steps(asm, T, present, N, k0)
        assert name != "steps4096" or calls == 1
        for mode in ("interp", "peak"):
            got = asm.read(mode)
            want = sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, mode)
            assert _same(got, want), (mode,) + _first_bad(got, want)
            if mode == "interp":
                below, above, hit = grid < xp[0], grid > xp[-1], np.isin(grid, xp)
                assert below.any() and _same(got[below], np.full(below.sum(), fp[0]))
                assert _same(got[above], np.full(above.sum(), fp[-1]))
                if grid_tag == "ulp":                                      # a grid point on a bin takes that bin's T
                    assert hit.sum() >= min(xp.size, 8000) and above.any()
                    assert _same(got[hit], fp[np.searchsorted(xp, grid[hit])])


def test_present_set_changing_between_reads():
    """The step table follows the present set: every read against the contract of the moment."""
    N, k0, k1, bin_hz, centres, T, _, _ = _stitch_inputs("k3", "all", "ulp")
    S, K = T.shape
    T = T.copy()
    grid = sc.ulp_grid(sc.frequencies(centres, k0, k1, N, bin_hz), K, bin_hz)
    rows = np.zeros((S, N), dtype=np.float32)
    present = np.zeros(S, dtype=bool)

    with SweepAssembler(N, centres, (k0, k1), bin_hz, grid) as asm, DeviceBuffer(rows.nbytes) as d, \
            DeviceBuffer(8 * grid.size) as d_out:
        def update(steps, values=None):
            for s in steps:
                if values is not None:
                    T[s] = values
                rows[s, k0:k1] = T[s]
                d.put(rows[s], 4 * s * N)
                asm.update_device(None, s, 1, d.at(4 * s * N), 1, "sample")
                present[s] = True

        def check(to_device=False):
            for mode in ("interp", "peak"):
                want = sc.assemble(T, present, centres, k0, k1, N, bin_hz, grid, mode)
                if to_device:                                            # to a device pointer, without a host pointer
                    assert asm.read(mode, out_dev=d_out.ptr, to_host=False) is None
                    valid = asm.steps()[1]                               # waits for the handle's stream
                    got = d_out.get(grid.size, np.float64)
                else:
                    got, valid = asm.read(mode), asm.steps()[1]
                assert np.array_equal(valid, present)
                assert _same(got, want), (mode, list(np.flatnonzero(present))) + _first_bad(got, want)

        check()                                                          # nothing present: all NaN
        update([3]); check()
        update([1, 5]); check(to_device=True)
        update([3], values=np.array([7.5, np.nan, -3.25], dtype=np.float32)); check()   # same set, new rows
        asm.reset(); present[:] = False; check()
        assert np.isnan(asm.read("interp")).all() and np.isnan(asm.read("peak")).all()
        update([0]); check()


# ---------------------------------------------------------------------------------------------------- the refusals
def _err():
    return nat.lib.tdsa_last_error_string().decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_every_refusal_of_a_live_handle_with_its_text():
    lib = nat.lib
    N, k0, k1, S, F = 256, 32, 224, 5, 2
    K = k1 - k0
    centres, _ = _geometry(S, K)
    grid = np.linspace(centres[0], centres[-1], 64)
    down = np.ascontiguousarray(grid[::-1])
    no_geometry = "no geometry: call tdsa_sweep_set_geometry first"
    host = np.zeros(S * K, dtype=np.float64)
    ms = C.c_float()
    with DeviceBuffer(4 * S * F * N) as d, DeviceBuffer(8 * grid.size + 8) as d_out:
        d.put((-80 + np.random.default_rng(2).standard_normal(S * F * N)).astype(np.float32))
        # ---- a handle without geometry
        h = C.c_void_p()
        assert lib.tdsa_sweep_create(0, N, S, grid.size, C.byref(h)) == 0
        try:
            assert lib.tdsa_sweep_update_dev(h, None, 0, 1, C.c_void_p(d.ptr), F, 0, nat.SWEEP_DET_MAX) == ERR_STATE
            assert _err() == no_geometry
            assert lib.tdsa_sweep_run_dev(h, None, nat.IN_I8, C.c_void_p(d.ptr), 0, 0, 1, N, N, 1, nat.SWEEP_DET_MAX) == ERR_STATE
            assert _err() == no_geometry
            assert lib.tdsa_sweep_read(h, nat.SWEEP_INTERP, _p(host), None) == ERR_STATE and _err() == no_geometry
            assert lib.tdsa_sweep_get_steps(h, _p(host), _p(host)) == ERR_STATE and _err() == no_geometry
        finally:
            assert lib.tdsa_sweep_destroy(h) == 0
        # ---- a live handle with two steps present
        with SweepAssembler(N, centres, (k0, k1), 1000.0, grid) as asm, SpectrumEngine(N, max_frames=F) as eng, \
                SpectrumEngine(2 * N, max_frames=F) as other:
            asm.update_device(None, 1, 2, d.at(4 * F * N), F, "max")
            T0, valid0 = asm.steps()
            out0 = {m: asm.read(m) for m in ("interp", "peak")}
            assert list(valid0) == [False, True, True, False, False]
            h, rows = asm._h, C.c_void_p(d.ptr)

            def refused(rc, text, code=ERR_ARG):
                assert rc == code and _err() == text, (rc, _err(), text)

            for det in (-1, 4):
                refused(lib.tdsa_sweep_update_dev(h, None, 0, 1, rows, F, 0, det),
                        f"detector={det}: TDSA_SWEEP_DET_SAMPLE / _MAX / _MIN / _AVG")
                refused(lib.tdsa_sweep_run_dev(h, eng._h, nat.IN_I8, rows, 0, 0, 1, N, N, 1, det),
                        f"detector={det}: TDSA_SWEEP_DET_SAMPLE / _MAX / _MIN / _AVG")
            for first, n in ((-1, 1), (4, 2), (0, 6), (0, -1), (5, 1)):
                refused(lib.tdsa_sweep_update_dev(h, None, first, n, rows, F, 0, nat.SWEEP_DET_MAX),
                        f"steps [{first}, {first} + {n}) outside the handle's {S}")
            refused(lib.tdsa_sweep_run_dev(h, eng._h, nat.IN_I8, rows, 0, 3, 3, N, N, 1, nat.SWEEP_DET_MAX),
                    f"steps [3, 3 + 3) outside the handle's {S}")
            for frames in (0, -2):
                refused(lib.tdsa_sweep_update_dev(h, None, 0, 1, rows, frames, 0, nat.SWEEP_DET_MAX),
                        f"frames_per_step={frames}: at least 1")
            refused(lib.tdsa_sweep_update_dev(h, None, 0, 1, None, F, 0, nat.SWEEP_DET_MAX), "null input")
            refused(lib.tdsa_sweep_run_dev(h, eng._h, nat.IN_I8, None, 0, 0, 1, N, N, 1, nat.SWEEP_DET_MAX), "null input")
            for off in (1, 2, 3):
                refused(lib.tdsa_sweep_update_dev(h, None, 0, 1, C.c_void_p(d.ptr + off), F, 0, nat.SWEEP_DET_MAX),
                        "rows pointer must be aligned to one float")
            refused(lib.tdsa_sweep_run_dev(h, None, nat.IN_I8, rows, 0, 0, 1, N, N, 1, nat.SWEEP_DET_MAX),
                    "null plan: the rows come from one")
            refused(lib.tdsa_sweep_run_dev(h, other._h, nat.IN_I8, rows, 0, 0, 1, 2 * N, 2 * N, 1, nat.SWEEP_DET_MAX),
                    f"the plan's frames ({2 * N} points) are not the assembler's rows of {N}")
            for fmt in (nat.IN_I8 - 1, nat.IN_C64 + 1):
                refused(lib.tdsa_sweep_run_dev(h, eng._h, fmt, rows, 0, 0, 1, N, N, 1, nat.SWEEP_DET_MAX), f"in_format {fmt}")
            for mode in (-1, 2):
                refused(lib.tdsa_sweep_read(h, mode, _p(host), None), f"mode={mode}: TDSA_SWEEP_INTERP / _PEAK")
            for off in (1, 4):
                refused(lib.tdsa_sweep_read(h, nat.SWEEP_INTERP, None, C.c_void_p(d_out.ptr + off)),
                        "output pointer must be aligned to one float64")
            refused(lib.tdsa_sweep_set_chunk_bytes(h, 0), "bytes=0")
            refused(lib.tdsa_sweep_timer_end(h, None), "null elapsed_ms")
            refused(lib.tdsa_sweep_timer_end(None, C.byref(ms)), "null sweep")
            # set_geometry: refused before anything of the handle changes
            geo = lambda c=centres, b=1000.0, a=k0, e=k1, g=grid: lib.tdsa_sweep_set_geometry(h, _p(np.ascontiguousarray(c)), b, a, e, _p(g))
            for a, e in ((-1, 10), (10, 10), (20, 10), (10, N + 1)):
                refused(geo(a=a, e=e), f"kept range [{a}, {e}): 0 <= k0 < k1 <= nfft = {N}")
            bad = centres.copy()
            bad[3] = np.inf
            refused(geo(c=bad), "centre 3 is not finite")
            bad_grid = grid.copy()
            bad_grid[17] = np.nan
            refused(geo(g=bad_grid), "grid point 17 is not finite")
            for b, shown in ((0.0, "0"), (-1.5, "-1.5"), (float("inf"), "inf"), (float("nan"), "nan")):
                refused(geo(b=b), f"bin_hz={shown}: positive and finite")
            touching = centres - np.arange(S) * 1000.0                 # the first bin of a step on the last of the one before
            last = touching[0] + float(k1 - 1 - N // 2) * 1000.0
            first = touching[1] + float(k0 - N // 2) * 1000.0
            assert last == first
            refused(geo(c=touching), f"steps 0 and 1: the last kept bin of one ({last:.17g} Hz) is not below the first of the "
                    f"next ({first:.17g} Hz) - centres must ascend and kept ranges must not overlap")
            rev = centres[::-1]
            refused(geo(c=rev), f"steps 0 and 1: the last kept bin of one ({rev[0] + float(k1 - 1 - N // 2) * 1000.0:.17g} Hz) "
                    f"is not below the first of the next ({rev[1] + float(k0 - N // 2) * 1000.0:.17g} Hz) - centres must "
                    "ascend and kept ranges must not overlap")
            # after all of them: T, the flags and a read are what they were
            T1, valid1 = asm.steps()
            assert _same(T1, T0) and np.array_equal(valid1, valid0)
            for m in ("interp", "peak"):
                assert _same(asm.read(m), out0[m])
        # peak on a descending grid: its own handle, interp still reads
        with SweepAssembler(N, centres, (k0, k1), 1000.0, down) as asm:
            asm.update_device(None, 0, S, d.ptr, F, "min")
            before = asm.read("interp")
            rc = lib.tdsa_sweep_read(asm._h, nat.SWEEP_PEAK, _p(host[:grid.size]), None)
            assert rc == ERR_ARG and _err() == f"peak mode needs an ascending grid (grid[1] - grid[0] = {down[1] - down[0]:g})"
            assert _same(asm.read("interp"), before) and asm.steps()[1].all()
