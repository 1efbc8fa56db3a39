#!/usr/bin/env python3
"""Golden vectors for zero span from the *imported reference* (core/display_data_processor.py:261-311,
DataProcessor._process_zero_span_data): a long run of display ticks over a wrapping two-second history.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_zero_span.py [out.npz]

Writes tests/golden/zero_span.npz.  DATA only: the raw int8 IQ of every tick, its trigger mode, level and window, and
the chunk the reference handed its widget.  The blocks the reference sees are complex64 (I + jQ) / 128 of the raw
bytes, so every sample - and every shown value - is k / 128 exactly and the chunks are stored as int8 (value * 128;
the round trip is asserted).  Rate 8000 Hz, so the history holds 16000 samples.

The generator checks what the run covers from the reference's own outputs and state (dm.zero_span_buffer) alone.
"""
import os
import sys
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
for _m in ("hackrf", "rtlsdr", "sounddevice"):
    sys.modules[_m] = MagicMock()
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

from core.display_data_processor import DataProcessor  # noqa: E402

RATE = 8000.0
TICKS = 200


class ZeroSpanWidget:
    def update_zero_span_data(self, t, y):
        self.t, self.y = np.array(t), np.array(y)


def to_c64(raw):
    """complex64 (I + jQ) / 128 of interleaved int8 pairs: exact."""
    v = raw.reshape(-1, 2).astype(np.float32) / np.float32(128.0)
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "zero_span.npz")
    rng = np.random.default_rng(20250611)
    src = types.SimpleNamespace(sample_rate=RATE, block=None)
    src.read_samples_only = lambda: src.block
    mw = types.SimpleNamespace(current_source=src, zero_span_widget=ZeroSpanWidget())
    dm = types.SimpleNamespace(zero_span_buffer=None, zero_span_time_window=0.01, zero_span_trigger_mode="free_run",
                               zero_span_trigger_level=0.0)
    dp = DataProcessor.__new__(DataProcessor)
    dp.mw, dp.dm = mw, dm

    capacity = int(2.0 * RATE)
    raws, lens, modes, levels, windows, shown, shown_len = [], [], [], [], [], [], []
    t0 = 0
    n_triggered = n_no_crossing = n_short = n_rounded_level = 0
    for tick in range(TICKS):
        n = int(rng.integers(300, 1700))
        k = np.arange(t0, t0 + n)
        t0 += n
        # a pulse train (period 91, duty drifting) under slow amplitude modulation, a little noise; Q is noise alone
        on = ((k % 91) < 30 + 20 * np.sin(k / 2900.0)).astype(np.float64)
        amp = 80.0 + 35.0 * np.sin(k / 1300.0)
        i = np.clip(np.rint(on * amp + 4.0 * rng.standard_normal(n) - 20.0), -128, 127)
        q = np.clip(np.rint(3.0 * rng.standard_normal(n)), -128, 127)
        raw = np.stack([i, q], axis=1).astype(np.int8).reshape(-1)
        block = to_c64(raw)
        assert np.array_equal(block.real * 128, i) and np.array_equal(block.imag * 128, q)

        mode = ("free_run", "rise", "fall", "rise")[int(rng.integers(0, 4))]
        window = float(10.0 ** rng.uniform(-4.0, -1.0)) if rng.random() < 0.9 else float(rng.uniform(0.1, 3.0))
        pick = rng.random()
        rounded = False
        if pick < 0.35:
            level = float(block.real[int(rng.integers(0, n))])           # a sample value
        elif pick < 0.50:
            level = float(block.real[int(rng.integers(0, n))]) + 1e-12   # float64 only: rounds to that sample in float32
            rounded = True
        elif pick < 0.65:
            level = 0.7
        elif pick < 0.75:
            level = 5.0                                                  # never crossed
        else:
            level = float(rng.uniform(-0.3, 0.9))
        dm.zero_span_trigger_mode, dm.zero_span_trigger_level, dm.zero_span_time_window = mode, level, window
        src.block = block
        dp._process_zero_span_data()

        chunk, buf = mw.zero_span_widget.y, dm.zero_span_buffer
        assert chunk.dtype == np.float32 and len(buf) <= capacity
        n_display = max(int(window * RATE), 4)
        assert np.array_equal(mw.zero_span_widget.t, np.arange(len(chunk), dtype=np.float32) / RATE)
        if len(buf) < n_display:
            n_short += 1
            assert np.array_equal(chunk, buf)
        elif mode != "free_run":
            if not np.array_equal(chunk, buf[-n_display:]):
                n_triggered += 1
                if rounded:
                    lv32 = np.float32(level)
                    assert float(lv32) != level and np.any(buf == lv32)
                    n_rounded_level += 1
            elif level == 5.0:
                n_no_crossing += 1
        c8 = np.rint(chunk * 128).astype(np.int8)
        assert np.array_equal(c8.astype(np.float32) / np.float32(128.0), chunk)
        raws.append(raw)
        lens.append(n)
        modes.append(mode)
        levels.append(level)
        windows.append(window)
        shown.append(c8)
        shown_len.append(len(chunk))

    total = int(np.sum(lens))
    wraps = total / capacity
    assert wraps >= 11.0, wraps                                   # the history wraps at least 10 times
    assert n_triggered >= TICKS // 4, n_triggered
    assert n_no_crossing >= 1 and n_short >= 1 and n_rounded_level >= 1, (n_no_crossing, n_short, n_rounded_level)
    assert min(max(int(w * RATE), 4) for w in windows) == 4 and max(int(w * RATE) for w in windows) > capacity
    assert any(lv == 0.7 for lv in levels)
    np.savez_compressed(out_path, rate=np.float64(RATE), raw=np.concatenate(raws), block_len=np.array(lens, dtype=np.int64),
                        modes=np.array(modes), levels=np.array(levels, dtype=np.float64),
                        windows=np.array(windows, dtype=np.float64), shown_i8=np.concatenate(shown),
                        shown_len=np.array(shown_len, dtype=np.int64))
    print(f"wrote {os.path.basename(out_path)}: {TICKS} ticks, {total} samples ({wraps:.1f} x the history), "
          f"{n_triggered} triggered ({100.0 * n_triggered / TICKS:.0f} %), {n_no_crossing} without a crossing, "
          f"{n_short} with held < n_display, {n_rounded_level} triggered on a level rounded to a sample, "
          f"{os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
