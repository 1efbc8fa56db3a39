#!/usr/bin/env python3
"""A stepped sweep end to end: 80 MHz of spectrum from a 10 Msps "tuner", stitched on the GPU.

    python examples/sweep_capture.py

`capture(centre_hz, n_samples)` stands for the radio: here it synthesises what a tuner at that centre would deliver
from a handful of carriers at absolute frequencies.  IqSweepDataSource retunes it step by step, the engine turns each
block into dB rows, the assembler folds the rows of a step (avg detector) and lays the steps' kept bins onto the fixed
grid - the trace HackRFSweepDataSource.get_data() would hand to DataProcessor._process_sweep_data.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import IqSweepDataSource  # noqa: E402

FS, NFFT = 10e6, 4096
START, STOP, BIN_SIZE = 400_000_000, 480_000_000, 10_000
CARRIERS = [(403.2e6, 0.5), (433.92e6, 0.2), (446.00625e6, 0.05), (467.5e6, 0.3)]     # (Hz, amplitude)


def capture(centre_hz, n_samples):
    rng = np.random.default_rng(int(centre_hz) & 0x7FFFFFFF)
    t = np.arange(n_samples) / FS
    x = 1e-3 * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    for f, a in CARRIERS:
        if abs(f - centre_hz) < 0.45 * FS:                    # the tuner's own filter
            x = x + a * np.exp(2j * np.pi * (f - centre_hz) * t)
    return x.astype(np.complex64)


def main():
    src = IqSweepDataSource(START, STOP, BIN_SIZE, capture=capture, sample_rate=FS, nfft=NFFT, frames_per_step=8,
                            detector="avg")
    src.mode = "peak"                                         # 10 kHz cells over 2.4 kHz bins: keep the narrow carriers
    try:
        print(f"{src.centres.size} steps of {(src.kept[1] - src.kept[0]) * src.bin_hz / 1e6:.2f} MHz, "
              f"{src.get_number_of_points()} grid points of {BIN_SIZE / 1e3:.0f} kHz")
        trace = src.sweep_once()
        grid = src.frequency_grid
        floor = np.median(trace)
        print(f"noise floor {floor:.1f} dB, {src.sweep_rate:.1f} sweeps/s (synthetic captures included)")
        for i in np.argsort(trace)[::-1][:len(CARRIERS)]:
            print(f"  {grid[i] / 1e6:10.3f} MHz  {trace[i]:7.1f} dB")
    finally:
        src.close()


if __name__ == "__main__":
    main()
