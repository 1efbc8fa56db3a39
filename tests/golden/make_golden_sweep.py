#!/usr/bin/env python3
"""Golden vectors for the sweep stitch from the *imported reference*.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sweep.py [other output file]

Drives HackRFSweepDataSource._parse with hackrf_sweep CSV lines made from seeded float32 step traces: 12 steps of
K = 3072 kept bins of 2000 Hz (fs = 8.192e6, N = 4096, every bin frequency a whole number of hertz), one step missing
(a gap), the first step first, the others in shuffled order, the first step again to close the sweep.  Each line's low
and high edge are x_first - bin/2 and x_last + bin/2, each value is written with repr(float(v)).  Writes
tests/golden/sweep.npz: traces, centres, geometry, grid and the reference's full_power_array.  DATA only.
"""
import os
import sys
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
for _m in ("hackrf", "rtlsdr", "sounddevice"):
    sys.modules[_m] = MagicMock()
REF = os.environ.get("TDSA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

from datasources.hackrf_sweep import HackRFSweepDataSource  # noqa: E402

FS, N, KEEP = 8.192e6, 4096, 0.75
START, BIN_SIZE = 100_000_000, 5205
SLOTS, MISSING = 13, 7                   # 13 abutting step positions, the one at index 7 is never delivered


def csv_line(low: int, high: int, bin_hz: float, values) -> str:
    return ", ".join(["2024-06-11", "12:00:00", str(low), str(high), repr(float(bin_hz)), str(len(values))] +
                     [repr(float(v)) for v in values])


def main():
    rng = np.random.default_rng(20240917)
    bin_hz = 1.0 / (N * (1.0 / FS))
    K = int(KEEP * N) // 2 * 2
    k0 = N // 2 - K // 2
    step = K * bin_hz
    stop = int(START + SLOTS * step)
    slots = np.array([s for s in range(SLOTS) if s != MISSING])
    centres = START + (slots + 0.5) * step
    traces = (-90.0 + 10.0 * rng.standard_normal((len(slots), K))).astype(np.float32)
    traces[2, 100] = np.nan
    traces[5, K - 1] = np.nan
    traces[9, 0] = np.nan
    traces[3, 2000] = np.inf
    traces[10, 17] = -np.inf
    src = HackRFSweepDataSource(START, stop, BIN_SIZE)
    order = [0] + [int(i) for i in 1 + rng.permutation(len(slots) - 1)] + [0]
    for i in order:
        x_first = centres[i] + (k0 - N // 2) * bin_hz
        x_last = centres[i] + (k0 + K - 1 - N // 2) * bin_hz
        low, high = x_first - bin_hz / 2, x_last + bin_hz / 2
        assert low == int(low) and high == int(high)
        src._parse(csv_line(int(low), int(high), bin_hz, traces[i]))
    full = src.get_data()
    assert full.dtype == np.float64 and full.size == src.frequency_grid.size and not np.isnan(full).all()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sweep.npz")
    np.savez_compressed(out, traces=traces, centres=centres, grid=src.frequency_grid, full_power_array=full,
                        order=np.array(order), geometry=np.array([FS, N, k0, k0 + K, bin_hz, START, stop, BIN_SIZE]))
    print(f"wrote {out} ({os.path.getsize(out)} bytes): {len(slots)} steps, grid of {full.size}")


if __name__ == "__main__":
    main()
