"""The signal detection without a device: the numpy contract on planted rows, the key mapping
of the radix selection, record layouts, to_hz against the analytics oracle, and every argument error of the Python layer
and of the C-ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import detect_contract as dc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import detect as dt

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from oracle import analytics_oracle as ao  # noqa: E402


# ---- the contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap,min_width,want", [(0, 1, 6), (1, 1, 5), (2, 1, 4), (6, 1, 3), (2, 2, 3)])
def test_contract_counts_the_planted_runs(max_gap, min_width, want):
    row, _ = dc.planted_row()
    n = row.size
    rr, sig, m = dc.detect_row(row, 0, n - 1, dc.rank_of(0.5, n), 10.0, min_width, max_gap, 3.0, 16)
    assert int(rr["n_found"]) == want and int(rr["flags"]) == 0
    assert int(rr["n_over"]) == int(m.sum()) == 39 + 3 + 12            # the NaN bin is not over
    assert np.all(sig["start"][want:] == -1) and np.all(np.isnan(sig["peak_db"][want:]))


def test_contract_recovers_starts_and_stops():
    row, planted = dc.planted_row()
    n = row.size
    rr, sig, _ = dc.detect_row(row, 0, n - 1, dc.rank_of(0.5, n), 10.0, 1, 1, 3.0, 16)
    assert [(int(s["start"]), int(s["stop"])) for s in sig[:5]] == planted
    assert rr["floor"] == np.sort(row)[dc.rank_of(0.5, n)] and rr["thr"] == np.float32(rr["floor"] + np.float32(10.0))
    rr0, sig0, _ = dc.detect_row(row, 0, n - 1, dc.rank_of(0.5, n), 10.0, 1, 0, 3.0, 16)
    assert [(int(s["start"]), int(s["stop"])) for s in sig0[:2]] == [(200, 219), (221, 239)]      # split at the NaN
    # the search range cuts a run, and only S records are written although more runs are found
    rr2, sig2, m2 = dc.detect_row(row, 210, 505, 100, 10.0, 1, 0, 3.0, 2)
    assert int(rr2["n_found"]) == 4 and (int(sig2["start"][0]), int(sig2["stop"][1])) == (210, 239) and not m2[:210].any()


def test_contract_centroid_within_half_a_bin_of_a_symmetric_signal():
    rng = np.random.default_rng(5)
    n, c = 2048, 777
    row = (-100.0 + rng.standard_normal(n)).astype(np.float32)
    k = np.arange(-15, 16)
    row[c + k] = (-50.0 - 0.05 * k.astype(np.float64) ** 2).astype(np.float32)
    rr, sig, _ = dc.detect_row(row, 0, n - 1, dc.rank_of(0.5, n), 10.0, 3, 0, 3.0, 4)
    assert int(rr["n_found"]) == 1 and (int(sig["start"][0]), int(sig["stop"][0])) == (c - 15, c + 15)
    centroid = sig["start"][0] + sig["moment"][0] / sig["power"][0]
    assert abs(centroid - c) < 0.5 and int(sig["peak_bin"][0]) == c
    assert (int(sig["x_lo"][0]), int(sig["x_hi"][0])) == (c - 7, c + 7)       # 0.05 k^2 <= 3 dB


def test_nan_floor_flags_the_row():
    row = np.full(16, np.nan, dtype=np.float32)
    row[:4] = [1, 2, 3, 4]
    rr, sig, m = dc.detect_row(row, 0, 15, 4, 0.0)
    assert int(rr["flags"]) == dc.FLAG_NAN_FLOOR and np.isnan(rr["thr"]) and int(rr["n_found"]) == int(rr["n_over"]) == 0
    assert not m.any() and np.all(sig["start"] == -1)
    rr, _, _ = dc.detect_row(row, 0, 15, 3, 0.0)
    assert int(rr["flags"]) == 0 and rr["floor"] == 4.0


def test_key_mapping_sorts_as_numpy_does():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 4000).astype(np.float32)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32)
    neg_nan = np.array([0xFFC00001, 0xFF800001, 0x7F800001], dtype=np.uint32).view(np.float32)
    x = np.concatenate([x, special, special, neg_nan])
    k = dc.keys(x)
    order = np.argsort(k, kind="stable")
    want = np.sort(x)
    got = x[order]
    assert np.array_equal(got, want, equal_nan=True)                    # by value: +0 / -0 may swap
    nn = int(np.count_nonzero(np.isnan(x)))
    assert np.all(k[np.isnan(x)] == 0xFFFFFFFF) and np.all(np.isnan(got[-nn:])) and not np.isnan(got[:-nn]).any()
    assert np.array_equal(dc.unkey(k), x, equal_nan=True)
    assert np.all(np.diff(np.sort(k)[:-nn].astype(np.int64)) >= 0)
    for r in (0, 1, x.size // 2, x.size - nn - 1, x.size - nn, x.size - 1):
        assert np.array_equal(dc.unkey(np.sort(k)[r]), want[r], equal_nan=True)


def test_record_sizes():
    assert dc.ROW.itemsize == dt.ROW_RECORD.itemsize == 32 and dc.SIGNAL.itemsize == dt.SIGNAL_RECORD.itemsize == 40
    assert [dt.ROW_RECORD.fields[f][1] for f in ("floor", "thr", "n_found", "n_over", "flags")] == [0, 4, 8, 12, 16]
    assert [dt.SIGNAL_RECORD.fields[f][1] for f in dt.SIGNAL_RECORD.names] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert dc.ROW.descr == dt.ROW_RECORD.descr and dc.SIGNAL.descr == dt.SIGNAL_RECORD.descr
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tdsa_hip.h")).read()
    assert "tdsa_detect_row" in hdr and "tdsa_detect_signal" in hdr


def test_to_hz_agrees_with_the_band_power_oracle():
    row, _ = dc.planted_row()
    n = row.size
    rr, sig, _ = dc.detect_row(row, 0, n - 1, dc.rank_of(0.5, n), 10.0, 1, 6, 3.0, 8)
    det = dt.detections_from(rr.reshape(1), sig.reshape(1, -1))
    freq = np.linspace(90e6, 110e6, n)
    em = det.to_hz(freq, 0)
    assert em.size == det.count(0) == 3
    bw = (freq[-1] - freq[0]) / (n - 1)
    for e, s in zip(em, sig[:3]):
        a, b = int(s["start"]), int(s["stop"])
        lv = np.where(np.isnan(row), -np.inf, row).astype(np.float64)      # a NaN bin adds no power to its run
        assert abs(e["power_db"] - ao.band_power_db(freq, lv, freq[a], freq[b])) <= 1e-4
        assert abs(e["bandwidth_hz"] - (b - a + 1) * bw) <= 1e-6 * bw
        assert abs(e["xdb_bandwidth_hz"] - (int(s["x_hi"]) - int(s["x_lo"]) + 1) * bw) <= 1e-6 * bw
        assert freq[a] <= e["centre_hz"] <= freq[b] and e["peak_hz"] == freq[int(s["peak_bin"])]
    with pytest.raises(ValueError):
        det.to_hz(freq[:10], 0)


def test_quantile_rank():
    assert [dt.quantile_rank(q, 5) for q in (0.0, 0.5, 0.6, 0.9, 1.0)] == [0, 2, 2, 4, 4]
    assert dt.quantile_rank(0.5, 1) == 0 and dt.quantile_rank(0.5, 16384) == 8192 == dc.rank_of(0.5, 16384)
    for q in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            dt.quantile_rank(q, 10)


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_python_layer_raises_before_the_library_is_called(monkeypatch):
    def boom(*a):
        raise AssertionError("the library was called")
    monkeypatch.setattr(nat.lib, "tdsa_detect_create", boom, raising=False)
    for n, kw in ((0, {}), (16385, {}), (64, dict(bins=(-1, 5))), (64, dict(bins=(5, 4))), (64, dict(bins=(0, 64))),
                  (64, dict(rank=64)), (64, dict(rank=-1)), (64, dict(bins=(10, 20), rank=11)),
                  (64, dict(floor_quantile=1.5)), (64, dict(margin_db=float("nan"))), (64, dict(margin_db=float("inf"))),
                  (64, dict(min_width=0)), (64, dict(min_width=65)), (64, dict(max_gap=-1)), (64, dict(max_gap=65)),
                  (64, dict(xdb=-1.0)), (64, dict(xdb=float("nan"))), (64, dict(max_signals=0)),
                  (64, dict(max_signals=65)), (64, dict(max_host_rows=0))):
        with pytest.raises(ValueError):
            dt.SignalDetector(n, **kw)


def test_calls_are_checked_before_the_library_is_called():
    d = object.__new__(dt.SignalDetector)                 # no device: the checks need the configuration only
    d.n_bins, d.max_host_rows, d.max_signals, d.device, d._h = 64, 4, 4, 0, None
    for call in (lambda: d.process(np.zeros((2, 63), np.float32)), lambda: d.process(np.zeros((2, 2, 64), np.float32)),
                 lambda: d.process(np.zeros((5, 64), np.float32)), lambda: d.process(np.zeros((1, 64), np.complex64)),
                 lambda: d.process_device(None, 0, 1), lambda: d.process_device(None, 258, 1),
                 lambda: d.process_device(None, 256, -1)):
        with pytest.raises(ValueError):
            call()


def test_library_refuses_bad_arguments_without_touching_a_device():
    lib = nat.lib
    good = (0, 63, 32, 10.0, 1, 0, 3.0, 16)
    bad = [(-1, 63, 0, 10.0, 1, 0, 3.0, 16), (5, 4, 0, 10.0, 1, 0, 3.0, 16), (0, 16384, 0, 10.0, 1, 0, 3.0, 16),
           (0, 63, -1, 10.0, 1, 0, 3.0, 16), (0, 63, 64, 10.0, 1, 0, 3.0, 16), (10, 20, 11, 10.0, 1, 0, 3.0, 16),
           (0, 63, 32, float("nan"), 1, 0, 3.0, 16), (0, 63, 32, float("inf"), 1, 0, 3.0, 16),
           (0, 63, 32, 10.0, 0, 0, 3.0, 16), (0, 63, 32, 10.0, 16385, 0, 3.0, 16), (0, 63, 32, 10.0, 1, -1, 3.0, 16),
           (0, 63, 32, 10.0, 1, 16385, 3.0, 16), (0, 63, 32, 10.0, 1, 0, -0.5, 16), (0, 63, 32, 10.0, 1, 0, float("nan"), 16),
           (0, 63, 32, 10.0, 1, 0, float("inf"), 16), (0, 63, 32, 10.0, 1, 0, 3.0, 0), (0, 63, 32, 10.0, 1, 0, 3.0, 65)]
    for args in bad:
        assert lib.tdsa_detect_configure(None, *args) == -1, args
        assert b"null" not in lib.tdsa_last_error_string(), args        # the argument was refused, not the handle
    assert lib.tdsa_detect_configure(None, *good) == -1 and b"null" in lib.tdsa_last_error_string()
    h = C.c_void_p()
    assert lib.tdsa_detect_create(0, 64, 1, None) == -1
    for n_bins, rows in ((0, 1), (-5, 1), (16385, 1), (64, 0)):
        assert lib.tdsa_detect_create(0, n_bins, rows, C.byref(h)) == -1 and not h.value
        assert b"n_bins" in lib.tdsa_last_error_string() or b"max_host_rows" in lib.tdsa_last_error_string()
    buf = (C.c_ubyte * 256)()
    assert lib.tdsa_detect_process(None, buf, 1, buf, buf) == -1
    assert lib.tdsa_detect_process_dev(None, None, buf, 1, buf, buf) == -1
    assert lib.tdsa_detect_read_occupancy(None, buf, None, None) == -1
    assert lib.tdsa_detect_reset(None) == -1
    assert lib.tdsa_detect_timer_begin(None) == -1 and lib.tdsa_detect_timer_end(None, None) == -1
    assert lib.tdsa_detect_destroy(None) == 0
