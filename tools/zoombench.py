#!/usr/bin/env python3
"""Timing of the zoom front end on one C3 second: 20e6 IQ samples in HBM, one call.

  ddc    DownConverter.process_device at D = 2, 8, 64, 512, 4096 (default 34-tap-per-phase design, offset 0.1 fs),
         int8 and complex64 input; device events on the plan's stream around `reps` back-to-back calls after warm-up
  zoom   ZoomSpectrum.process_device end to end at D = 64, nfft = 4096, hop = 2048, max hold on

Floors, from the shapes: compute = n_in (4 T / D + 8) FLOPs at the 157.3 TFLOPS FP32 vector peak; memory = n_in
(2 or 8) + n_out 8 bytes at the measured 6.29 TB/s.

    python tools/zoombench.py [--out profiles/zoombench.txt] [--reps 10]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat  # noqa: E402
from topdogspectrumanalyser_amd.zoom import DownConverter, ZoomSpectrum  # noqa: E402

FS = 20e6
N_IN = 20_000_000
FP32_PEAK = 157.3e12
HBM_BPS = 6.29e12
TARGET_US = 45.0


def timed(eng, f, warm, reps):
    for _ in range(warm):
        f()
    eng.timer_begin()
    for _ in range(reps):
        f()
    return eng.timer_end() * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    raw = rng.integers(-128, 128, 2 * N_IN).astype(np.int8)
    cplx = (raw[0::2].astype(np.float32) / 128 + 1j * raw[1::2].astype(np.float32) / 128).astype(np.complex64)
    d_i8, d_c64 = DeviceBuffer.of(raw), DeviceBuffer.of(cplx)
    d_out = DeviceBuffer(8 * (N_IN // 2 + 8))
    del cplx
    say(f"one C3 second: {N_IN} IQ samples in HBM, one call; device events around {args.reps} calls after "
        f"{args.warm} warm-up calls; offset 0.1 fs; default filter (T = 34 D)")
    say(f"floors: compute n_in (4T/D + 8) FLOP at {FP32_PEAK / 1e12:.1f} TFLOPS, memory at {HBM_BPS / 1e12:.2f} TB/s; "
        f"target <= {TARGET_US:.0f} us for D in 8, 64, 512")
    say(f"{'D':>5s} {'input':>5s} {'us':>9s} {'GFLOP':>7s} {'TFLOPS':>7s} {'%peak':>6s} {'cmp floor us':>12s} "
        f"{'mem floor us':>12s} {'GS/s':>7s}")
    try:
        with SpectrumEngine(1024) as eng:
            for D in (2, 8, 64, 512, 4096):
                with DownConverter(D, FS, 0.1 * FS) as ddc:
                    T = ddc.taps.size
                    for name, fmt, ptr, bps in (("i8", nat.IN_I8, d_i8, 2), ("c64", nat.IN_C64, d_c64, 8)):
                        us = timed(eng, lambda: ddc.process_device(eng, fmt, ptr.ptr, N_IN, d_out.ptr),
                                   args.warm, args.reps)
                        flop = N_IN * (4.0 * T / D + 8)
                        n_out = N_IN // D
                        say(f"{D:5d} {name:>5s} {us:9.1f} {flop / 1e9:7.2f} {flop / us / 1e6:7.1f} "
                            f"{100 * flop / us / 1e6 / (FP32_PEAK / 1e12):5.1f}% {flop / FP32_PEAK * 1e6:12.1f} "
                            f"{(N_IN * bps + n_out * 8) / HBM_BPS * 1e6:12.1f} {N_IN / us / 1e3:7.2f}")
        D, N, hop = 64, 4096, 2048
        with ZoomSpectrum(FS, D, N, offset_hz=0.1 * FS, hop=hop) as z:
            z.engine.configure(hold_max=True)
            frames = z.frames_completed_by(N_IN) + 4
            d_rows = DeviceBuffer(4 * frames * N)
            try:
                us = timed(z.engine, lambda: z.process_device(nat.IN_I8, d_i8.ptr, N_IN, d_rows.ptr),
                           args.warm, args.reps)
            finally:
                d_rows.close()
            say(f"ZoomSpectrum end to end, D = {D}, nfft = {N}, hop = {hop}, max hold, int8: {us:.1f} us per C3 second "
                f"({frames - 4} frames, rbw {FS / D / N:.1f} Hz)")
    finally:
        for p in (d_i8, d_c64, d_out):
            p.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
