"""Zero span, host side (no GPU): the numpy restatement in tests/zero_span_contract.py reproduces every trace the
reference recorded (tests/golden/zero_span.npz; live against the reference class where its tree is there), view_plan
agrees with it, the C-ABI refuses bad arguments before it touches a device, the info struct keeps its size,
tdsa_zerospan.hip compiles for gfx950 without scratch, and DataProcessor with the device path off is the host code it
was."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import zero_span_contract as zc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import ZeroSpan, view_plan  # noqa: F401  (the public names)
from topdogspectrumanalyser_amd.core.display_data_processor import DataProcessor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "zero_span.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
ERR_ARG = -1


# ---------------------------------------------------------------------------------------------------- the contract
def test_contract_reproduces_every_recorded_trace():
    rate, ticks = zc.golden_ticks(GOLDEN)
    capacity = int(2.0 * rate)
    assert capacity == 16000 and len(ticks) >= 200
    history = np.empty(0, dtype=np.float32)
    triggered = short = 0
    for i, t in enumerate(ticks):
        re, im = zc.unpack(t["raw"], "i8")
        assert np.array_equal(re, t["block"].real) and np.array_equal(im, t["block"].imag)
        history = np.concatenate([history, zc.detect(re, im, "real")])
        n_display = max(int(t["window"] * rate), 4)
        start, trig, chunk = zc.view(history, capacity, n_display, t["mode"], t["level"])
        assert chunk.dtype == np.float32 and np.array_equal(chunk, t["shown"]), (i, t["mode"], t["level"], n_display)
        plan = zc.view_plan(history.size, capacity, n_display, t["mode"])
        assert len(chunk) == plan["length"] and plan["base"] <= start <= history.size - len(chunk)
        triggered += trig
        short += plan["held"] < n_display
    assert history.size >= 11 * capacity and triggered >= len(ticks) // 4 and short >= 1


def test_level_is_compared_in_float32():
    """float32(0.7) is not below the Python float 0.7 - and a level one float64 step above a sample is that sample."""
    e = np.array([0.0, 0.7, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
    assert not (e[1:2] < 0.7)[0] and float(e[1]) < 0.7
    start, trig, _ = zc.view(e, 16, 4, "rise", 0.7)
    assert (start, trig) == (1, 1)                                  # e[0] < level <= e[1]
    start, trig, _ = zc.view(e, 16, 4, "rise", 0.5 + 1e-12)         # rounds to 0.5: e[3] >= level
    assert (start, trig) == (3, 1)
    start, trig, _ = zc.view(np.array([0, np.nan, 1, np.nan, 0, 0, 0, 0, 0, 0], dtype=np.float32), 16, 4, "rise", 0.5)
    assert trig == 0                                                # a NaN never matches


@pytest.mark.parametrize("seed", range(4))
def test_view_plan_agrees_with_the_contract(seed):
    rng = np.random.default_rng(seed)
    for _ in range(500):
        cap = int(rng.integers(4, 5000))
        total = int(rng.integers(0, 4 * cap))
        nd = int(rng.integers(1, 2 * cap))
        mode = ("free_run", "rise", "fall")[int(rng.integers(0, 3))]
        got, want = view_plan(total, cap, nd, mode), zc.view_plan(total, cap, nd, mode)
        assert got == want, (total, cap, nd, mode)
        assert got["held"] == min(total, cap) and got["base"] == total - got["held"]
        if got["search"] is not None:
            ss, se = got["search"]
            assert 0 <= ss <= se - 2 and se == got["held"] - nd and ss == max(0, se - 8 * nd)
    for bad in ((-1, 8, 4, "rise"), (8, 0, 4, "rise"), (8, 8, 0, "rise"), (8, 8, 4, "edge")):
        with pytest.raises(ValueError):
            view_plan(*bad)


def test_cells_partition_the_chunk():
    for L, n_points in ((1, 1), (5, 7), (100, 7), (16384, 16384), (40001, 1024), (1 << 28, 16384), (63, 1), (1000, 999)):
        P, b = zc.cells(L, n_points)
        assert P == min(L, n_points) and b[0] == 0 and b[-1] == L and all(b[c] < b[c + 1] for c in range(P))
    chunk = np.array([3, 1, np.nan, 2, 5, 4, 0, 7], dtype=np.float32)
    mm = zc.columns(chunk, 4)
    assert np.array_equal(mm, np.array([[1, np.nan, 4, 0], [3, np.nan, 5, 7]], dtype=np.float32), equal_nan=True)
    assert np.array_equal(zc.columns(chunk, 4, "sample"), chunk[::2], equal_nan=True)
    assert np.array_equal(zc.columns(chunk, 20, "sample"), chunk, equal_nan=True)
    st = zc.statistics(np.array([0, 1, 1, 0, 1, 0], dtype=np.float32), 0.5)
    assert (st["n_at_or_above"], st["n_rise"], st["n_fall"], st["mean"]) == (3, 2, 2, 0.5)


def test_uint8_unpack_is_the_frame_kernels():
    """(float32(u) - 127.5) * float32(1 / 127.5): csrc/tdsa_capi_internal.hpp in_format_consts."""
    u = np.arange(256, dtype=np.uint8)
    re, im = zc.unpack(np.stack([u, u[::-1]], axis=1).reshape(-1), "u8")
    want = (u.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)
    assert np.array_equal(re, want) and np.array_equal(im, want[::-1]) and re[0] == -1.0 and re[255] == 1.0


def test_origin_is_the_identity_at_zero_and_a_shift_elsewhere_on_the_golden_ticks():
    """view(origin=0) is view() on every recorded tick; the last `capacity` samples with origin = base see the same
    window, and so does the same tail declared 2^32 samples later, shifted by exactly that."""
    rate, ticks = zc.golden_ticks(GOLDEN)
    capacity = int(2.0 * rate)
    history = np.empty(0, dtype=np.float32)
    triggered = 0
    for t in ticks:
        history = np.concatenate([history, zc.detect(*zc.unpack(t["raw"], "i8"), "real")])
        n_display = max(int(t["window"] * rate), 4)
        start, trig, chunk = zc.view(history, capacity, n_display, t["mode"], t["level"])
        s0, t0, c0 = zc.view(history, capacity, n_display, t["mode"], t["level"], origin=0)
        assert (s0, t0) == (start, trig) and np.array_equal(c0, chunk) and np.array_equal(chunk, t["shown"])
        base = max(0, history.size - capacity)
        for shift in (0, 1 << 32):
            if history.size < capacity and shift:
                continue                                  # a short history is not the tail of a longer one
            s1, t1, c1 = zc.view(history[base:], capacity, n_display, t["mode"], t["level"], origin=base + shift)
            assert (s1, t1) == (start + shift, trig) and np.array_equal(c1, chunk)
        triggered += trig
    assert triggered >= 50 and history.size > 10 * capacity
    with pytest.raises(ValueError):
        zc.view(history[-10:], capacity, 4, "rise", 0.0, origin=history.size - 10)   # does not reach back to base


def test_inputs_of_the_shapes_suite_discriminate():
    """The CPU half of tests/test_gpu_zero_span_shapes.py: exact sums, crossing trains that cross at every sample, DB
    inputs whose neighbours are 0.1 dB apart, push streams that meet every head, tail and piece length."""
    # exact sums: multiples of 2^-7 below 1 - up to 2^46 of them fit 53 bits
    rng = np.random.default_rng(0)
    e = zc.crossing_train(100_000, rng)
    assert zc.sum_is_exact(e) and np.all(np.abs(e) < 1) and np.array_equal(e * 128, np.rint(e * 128))
    assert zc.crossings(e) == (50_000, 49_999) and np.all((e[:-1] < 0) != (e[1:] < 0))
    assert zc.crossings(zc.crossing_train(7, rng, first_above=True)) == (3, 3)
    shuffled = rng.permutation(e).astype(np.float64)
    assert np.sum(shuffled) == np.sum(e, dtype=np.float64) == float(np.sum(np.rint(e.astype(np.float64) * 128).astype(np.int64))) / 128
    assert not zc.sum_is_exact([0.1]) and not zc.sum_is_exact([2.0 ** -8]) and not zc.sum_is_exact([np.nan])
    assert not zc.sum_is_exact([2.0 ** 46, 2.0 ** 46 - 2.0 ** -7]) and zc.sum_is_exact([2.0 ** 45, -(2.0 ** 45) + 2.0 ** -7])
    # the view cases: a window across the physical wrap, a crossing on either side of it, length - 1 crossings inside
    for length, points in zc.VIEW_SHAPES:
        e, cap, start = zc.train_case(length, length)        # asserts all of that
        assert e.size * 127 < 2 ** 46 and cap == length + zc.PAD
        nans = zc.nan_positions(length, points)
        assert all(2 <= k < length for k in nans) and (length < 3 or nans)
    # the push streams
    for cap in zc.PUSH_CAPS:
        for fmt in ("i8", "u8", "c64", "f32r"):
            lengths, raw = zc.push_stream(fmt, cap)
            assert sorted(lengths)[:41] == list(range(41)) and {cap - 1, cap, cap + 1, 3 * cap + 5} <= set(lengths)
            re, im = zc.unpack(raw, fmt)
            assert re.size == sum(lengths) and zc.db_spacing(re, im, zc.LOG_FLOOR) >= 0.1
            assert np.all(re[1:] != re[:-1])
            G = zc.GROUP[fmt]
            pieces = zc.push_pieces(cap, lengths, G)
            assert {p[0] for p in pieces} == {0, 1, 2, 3} and {p[2] for p in pieces} == set(range(G))
            assert all(h + g * G + t == n and n <= cap for h, g, t, n in pieces)
            assert set(range(1, G + 4)) <= {p[3] for p in pieces} and 0 in lengths
            assert len(pieces) > len(lengths) - 1                 # pushes cut in two at the physical wrap
            assert max(p[1] for p in pieces) > 256 // G or cap < 256   # a body of more than one workgroup
            p = re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2 + float(np.float32(zc.LOG_FLOOR))
            assert p.min() >= 0.999e-12 and p.max() <= 32.0
            for det in ("real", "mag", "db"):
                e = zc.detect(re, im, det, zc.LOG_FLOOR, zc.OFFSET_DB)
                assert np.all(np.isfinite(e)) and np.all(e[1:] != e[:-1]), (fmt, cap, det)
    assert zc.db_spacing([1.0, 1.0], [0.0, 0.0], 0.0) == 0.0 and zc.db_spacing([1.0], [0.0], 0.0) == float("inf")
    # the extreme samples hold what the suite says they hold
    parts = zc.extreme_parts()
    assert np.isnan(parts).sum() == 3 and np.isinf(parts).sum() == 2 and np.signbit(parts[1]) and parts[1] == 0
    tiny = np.finfo(np.float32).tiny
    with np.errstate(all="ignore"):
        sq = parts * parts
    assert ((np.abs(parts) > 0) & (np.abs(parts) < tiny)).sum() >= 4 and ((sq > 0) & (sq < tiny)).any() and np.isinf(sq[np.isfinite(parts)]).any()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core")), reason="the reference tree is not here")
def test_live_differential_against_the_reference_class(tmp_path):
    """The generator run afresh against the reference's _process_zero_span_data: the same vectors as the committed ones."""
    out = str(tmp_path / "zero_span_live.npz")
    env = dict(os.environ, TDSA_REFERENCE=REF, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_zero_span.py"), out],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    live, gold = np.load(out), np.load(GOLDEN)
    assert sorted(live.files) == sorted(gold.files)
    for k in gold.files:
        assert np.array_equal(live[k], gold[k]), k


# ---------------------------------------------------------------------------------------------------- the C-ABI
def _err():
    return nat.lib.tdsa_last_error_string().decode()


def test_info_struct_layout():
    assert C.sizeof(nat.ZspanInfo) == 64          # 2 x i64, 3 x i32, 2 x f32, (pad), f64, i64, 2 x i32
    assert nat.ZspanInfo.mean.offset == 40 and nat.ZspanInfo.n_at_or_above.offset == 48
    assert nat.ZspanInfo.n_fall.offset == 60
    hdr = open(os.path.join(ROOT, "include", "tdsa_hip.h")).read()
    assert re.search(r"#define TDSA_IN_F32R 3\b", hdr) and nat.IN_F32R == 3
    for name in ("ZS_DET_REAL", "ZS_DET_MAG", "ZS_DET_DB", "ZS_FREE_RUN", "ZS_RISE", "ZS_FALL", "ZS_COL_MINMAX",
                 "ZS_COL_SAMPLE", "ZS_COL_MEAN"):
        assert int(re.search(rf"#define TDSA_{name} (\d+)", hdr).group(1)) == getattr(nat, name), name


def test_c_abi_refuses_bad_arguments_without_a_device():
    h, lib = C.c_void_p(), nat.lib
    info = nat.ZspanInfo()
    buf = (C.c_float * 64)()
    assert lib.tdsa_zspan_create(0, 3, 1024, C.byref(h)) == ERR_ARG and "capacity" in _err()
    assert lib.tdsa_zspan_create(0, (1 << 28) + 1, 1024, C.byref(h)) == ERR_ARG and "capacity" in _err()
    assert lib.tdsa_zspan_create(0, 16000, 0, C.byref(h)) == ERR_ARG and "max_host_samples" in _err()
    assert lib.tdsa_zspan_create(0, 16000, 1024, None) == ERR_ARG and "null" in _err()
    assert not h
    assert lib.tdsa_zspan_set_detector(None, 3, 0.0, 0.0) == ERR_ARG and "detector" in _err()
    assert lib.tdsa_zspan_set_detector(None, -1, 0.0, 0.0) == ERR_ARG and "detector" in _err()
    assert lib.tdsa_zspan_set_detector(None, 1, 0.0, 0.0) == ERR_ARG and "null" in _err()
    assert lib.tdsa_zspan_reset(None) == ERR_ARG and "null" in _err()
    assert lib.tdsa_zspan_push(None, 4, buf, 8) == ERR_ARG and "in_format" in _err()
    assert lib.tdsa_zspan_push(None, 3, buf, 8) == ERR_ARG and "null" in _err()
    assert lib.tdsa_zspan_push_dev(None, None, -1, buf, 8) == ERR_ARG and "in_format" in _err()
    assert lib.tdsa_zspan_push_dev(None, None, 2, buf, 8) == ERR_ARG and "null" in _err()
    assert lib.tdsa_zspan_view(None, 3, 0.0, 100, 0, 0, C.byref(info), buf, None) == ERR_ARG and "mode" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, 100, 16385, 0, C.byref(info), buf, None) == ERR_ARG and "n_points" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, 100, -1, 0, C.byref(info), buf, None) == ERR_ARG and "n_points" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, 100, 16, 3, C.byref(info), buf, None) == ERR_ARG and "col_detector" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, 0, 16, 0, C.byref(info), buf, None) == ERR_ARG and "n_display" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, (1 << 28) + 1, 16, 0, C.byref(info), buf, None) == ERR_ARG and "n_display" in _err()
    assert lib.tdsa_zspan_view(None, 1, 0.0, 100, 16, 0, C.byref(info), buf, None) == ERR_ARG and "null" in _err()
    assert lib.tdsa_zspan_timer_begin(None) == ERR_ARG and lib.tdsa_zspan_timer_end(None, None) == ERR_ARG
    assert lib.tdsa_zspan_destroy(None) == 0


def test_python_layer_refuses_bad_arguments_before_any_handle():
    for kw in (dict(detector="peak"), dict(sample_rate=0.0), dict(sample_rate=1.0), dict(sample_rate=200e6)):
        with pytest.raises(ValueError):
            ZeroSpan(**dict(dict(sample_rate=8000.0), **kw))


# ---------------------------------------------------------------------------------------------------- the kernels
def test_zero_span_kernels_are_free_of_scratch():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/tdsa_zerospan.o" in mk and re.search(r"^CAPI\s*=.*\bzspan\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_zerospan\.hpp\b", mk, re.M)
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "tdsa_zerospan.hip", "-o", os.devnull]
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
    push = [k for k in kernels if "zspan_push_kernel" in k]
    trig = [k for k in kernels if "zspan_trigger_kernel" in k]
    view = [k for k in kernels if "zspan_view_kernel" in k]
    assert len(push) == 12, sorted(kernels)       # four input formats x three detectors
    assert len(trig) == 1 and len(view) == 7      # the chunk, and three column detectors x (wave, workgroup) per cell
    for k in push + trig + view:
        assert kernels[k]["ScratchSize [bytes/lane]"] == "0", (k, kernels[k])
        assert kernels[k].get("VGPRs Spill", "0") == "0", (k, kernels[k])
        assert int(kernels[k]["VGPRs"]) <= 64, (k, kernels[k])          # eight waves per SIMD stay possible
    for k in push:
        assert kernels[k]["LDS Size [bytes/block]"] == "0", (k, kernels[k])   # pure streaming
    src = open(os.path.join(CSRC, "tdsa_zerospan.hip")).read()
    assert not re.search(r"\basm\b", src)


# ---------------------------------------------------------------------------------------------------- DataProcessor
def _feed(dp, mw, dm, src, g):
    for i, mode in enumerate(g["zs_modes"]):
        dm.zero_span_trigger_mode, dm.zero_span_trigger_level = str(mode), float(g["zs_levels"][i])
        src.block = g[f"zs_block_{i}"]
        dp._process_zero_span_data()
        want = g[f"zs_shown_{i}"]
        assert np.array_equal(mw.zero_span_widget.y, want), (i, mode)
        assert np.array_equal(mw.zero_span_widget.t, np.arange(len(want), dtype=np.float32) / float(g["zs_rate"]))


def test_data_processor_with_the_flag_off_is_the_host_path(golden_dir):
    """No device object is made and dm.zero_span_buffer stays the float32 history - both for an object built the usual
    way and for one built with __new__, which has no such attribute at all."""
    g = np.load(os.path.join(golden_dir, "gui_feeds.npz"))

    class W:
        def update_zero_span_data(self, t, y):
            self.t, self.y = np.array(t), np.array(y)

    for build in ("new", "init"):
        src = types.SimpleNamespace(sample_rate=float(g["zs_rate"]), block=None)
        src.read_samples_only = lambda s=src: s.block
        mw = types.SimpleNamespace(current_source=src, zero_span_widget=W())
        dm = types.SimpleNamespace(zero_span_buffer=None, zero_span_time_window=float(g["zs_window"]),
                                   zero_span_trigger_mode="free_run", zero_span_trigger_level=0.0)
        if build == "new":
            dp = DataProcessor.__new__(DataProcessor)
            dp.mw, dp.dm = mw, dm
            assert not hasattr(dp, "zero_span_on_device")
        else:
            dp = DataProcessor(mw, dm)                 # makes no device object until a frame needs one
            assert dp.zero_span_on_device is False and dp._zero_span is None
        _feed(dp, mw, dm, src, g)
        assert isinstance(dm.zero_span_buffer, np.ndarray) and dm.zero_span_buffer.dtype == np.float32
        assert getattr(dp, "_zero_span", None) is None
    assert DataProcessor(mw, dm, zero_span_on_device=True).zero_span_on_device is True
