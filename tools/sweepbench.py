#!/usr/bin/env python3
"""Timing of the sweep assembler on one panoramic sweep: 0 .. 6 GHz at fs = 20e6, N = 8192,
keep 0.75 (400 steps), 16 frames per step at hop N, int8 IQ resident in HBM, grids of 6000 and 600 000 points.

  (a) tdsa_process_dev_batch alone, rows to HBM: what the library could do before the assembler existed
  (b) SweepAssembler.run_device + read, per detector and stitch mode: device time (events on the plan's stream around
      run_device, on the handle's stream around read) and host wall clock of the whole sweep including the wait
  (c) the detector kernel alone (update_device on rows already there) and the stitch kernel alone (read to a device
      buffer), with the bytes they read
  (d) a device-to-device copy of the bytes the detector reads, in the same run
  (e) for scale, the way without the assembler: rows back to the host, the numpy contract applied to them
  and run_device under different bounds of its row scratch (are a chunk's rows still cached when the detector reads
  them?).

Device times are HIP events around `reps` back-to-back calls after `warm` warm-up calls.

    python tools/sweepbench.py [--out profiles/sweepbench.txt] [--reps 10]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (DeviceBuffer, SpectrumEngine, SweepAssembler, _native as nat,  # noqa: E402
                                        plan_steps)
from topdogspectrumanalyser_amd.sweep import frequency_grid  # noqa: E402
from topdogspectrumanalyser_amd.zoom import zoom_window  # noqa: E402

START, STOP, FS, N, KEEP, F = 0.0, 6e9, 20e6, 8192, 0.75, 16
GRIDS = ((6000, 1_000_000), (600_000, 10_000))          # points, bin_size
DETECTORS = ("sample", "max", "min", "avg")


def timed(h, f, warm, reps):
    """us per call, events on the stream of h: an engine's plan or an assembler.  The assembler's timer_end first puts
    its stream behind a launch that went on a plan's stream; everything timed on an assembler here is a read, which
    runs on the assembler's own stream, so that wait never applies and the figures mean what they did before the timer
    had it."""
    for _ in range(warm):
        f()
    h.timer_begin()
    for _ in range(reps):
        f()
    return h.timer_end() * 1e3 / reps


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

    centres, (k0, k1), bin_hz = plan_steps(START, STOP, FS, N, KEEP)
    S, K = centres.size, k1 - k0
    n_per = F * N
    rng = np.random.default_rng(1)
    raw = rng.integers(-128, 128, (S, 2 * n_per)).astype(np.int8)
    row_bytes, det_bytes = 4 * S * F * N, 4 * S * F * K
    d_iq, d_rows, d_copy = DeviceBuffer(raw.nbytes), DeviceBuffer(row_bytes), DeviceBuffer(det_bytes)
    d_iq.put(raw)
    say(f"sweep {START / 1e9:.0f} .. {STOP / 1e9:.0f} GHz: fs {FS / 1e6:.0f} MHz, N {N}, kept bins [{k0}, {k1}) of {bin_hz:.3f} Hz, "
        f"{S} steps x {F} frames at hop {N}, int8 IQ in HBM ({raw.nbytes / 1e6:.1f} MB), rows {row_bytes / 1e6:.1f} MB, "
        f"kept part of the rows {det_bytes / 1e6:.1f} MB")
    say(f"device events around {args.reps} calls after {args.warm} warm-up calls")
    try:
        with SpectrumEngine(N, max_frames=F) as eng:
            eng.set_window(zoom_window(N))
            eng.configure(db_mode="mag", log_floor=1e-12, dc_alpha=-1.0)

            def batch():
                eng.process_device_batch(nat.IN_I8, d_iq.ptr, 2 * n_per, S, n_per, N, F, d_rows.ptr)

            us_a = timed(eng, batch, args.warm, args.reps)
            say(f"(a) tdsa_process_dev_batch, rows alone: {us_a:9.1f} us")
            us_d = timed(eng, lambda: nat.check(nat.lib.tdsa_plan_copy(eng._h, d_copy.ptr, d_rows.ptr, det_bytes, 0)),
                              args.warm, args.reps)
            say(f"(d) device-to-device copy of {det_bytes / 1e6:.1f} MB: {us_d:9.1f} us "
                f"({det_bytes / us_d / 1e3:.0f} GB/s read, as much written)")
            for n_grid, bin_size in GRIDS:
                grid = frequency_grid(START, STOP, bin_size)
                assert grid.size == n_grid
                d_out = DeviceBuffer(8 * n_grid)
                try:
                    with SweepAssembler(N, centres, (k0, k1), bin_hz, grid) as asm:
                        say(f"--- grid of {n_grid} points ({bin_size / 1e3:.0f} kHz cells, {bin_size / bin_hz:.1f} bins each)")
                        batch()
                        for det in DETECTORS:
                            us = timed(eng, lambda: asm.update_device(eng, 0, S, d_rows.ptr, F, det),
                                            args.warm, args.reps)
                            rd = 4 * S * K if det == "sample" else det_bytes
                            say(f"(c) detector {det:>6s} alone: {us:9.1f} us, reads {rd / 1e6:7.1f} MB, {rd / us / 1e3:6.0f} GB/s"
                                + (f"   [aim: <= copy (d) {us_d:.1f} us: {'met' if us <= us_d else 'MISSED'}]"
                                   if det != "sample" else ""))
                        eng.synchronize()
                        for mode in ("interp", "peak"):
                            us = timed(asm, lambda: asm.read(mode, out_dev=d_out.ptr, to_host=False),
                                             args.warm, args.reps)
                            rd = 8 * n_grid + 4 * S * K
                            say(f"(c) stitch {mode:>6s} alone: {us:9.1f} us, reads <= {rd / 1e6:6.1f} MB "
                                f"(grid + T), writes {8 * n_grid / 1e6:.2f} MB, {(rd + 8 * n_grid) / us / 1e3:6.0f} GB/s")
                        for det in DETECTORS:
                            def run():
                                asm.run_device(eng, nat.IN_I8, d_iq.ptr, 2 * n_per, 0, S, n_per, N, F, det)
                            us_run = timed(eng, run, args.warm, args.reps)
                            for mode in ("interp", "peak"):
                                us_read = timed(asm, lambda: asm.read(mode, out_dev=d_out.ptr, to_host=False),
                                                      1, args.reps)
                                run()
                                asm.read(mode)
                                t0 = time.perf_counter()
                                for _ in range(args.reps):
                                    run()
                                    asm.read(mode)
                                wall = (time.perf_counter() - t0) * 1e6 / args.reps
                                say(f"(b) run_dev {det:>6s} + read {mode:>6s}: device {us_run:9.1f} + {us_read:7.1f} us "
                                    f"(rows alone (a) {us_a:.1f}), host wall clock per sweep {wall:9.1f} us")
                        if n_grid == GRIDS[0][0]:
                            for mib in (8, 16, 32, 64, 128, 256):
                                asm.set_chunk_bytes(mib << 20)
                                us = timed(eng, lambda: asm.run_device(eng, nat.IN_I8, d_iq.ptr, 2 * n_per, 0, S,
                                                                            n_per, N, F, "avg"), args.warm, args.reps)
                                steps = max(1, min(S, (mib << 20) // (4 * F * N)))
                                say(f"    run_dev avg, row scratch bound {mib:4d} MiB ({steps:3d} steps per chunk): {us:9.1f} us")
                            asm.set_chunk_bytes(256 << 20)
                finally:
                    d_out.close()
            # (e) without the assembler: rows to the host, numpy
            import sweep_contract as sc
            batch()
            rows = np.empty((S, F, N), dtype=np.float32)
            t0 = time.perf_counter()
            batch()
            nat.check(nat.lib.tdsa_plan_copy(eng._h, rows.ctypes.data_as(C.c_void_p), d_rows.ptr, rows.nbytes, 1))
            t1 = time.perf_counter()
            T = np.stack([sc.detector(rows[s], k0, k1, "avg") for s in range(S)])
            t2 = time.perf_counter()
            grid = frequency_grid(START, STOP, GRIDS[1][1])
            sc.assemble(T, np.ones(S, bool), centres, k0, k1, N, bin_hz, grid)
            t3 = time.perf_counter()
            say(f"(e) today's way: rows + read-back of {rows.nbytes / 1e6:.1f} MB {1e3 * (t1 - t0):.1f} ms, numpy avg detector "
                f"{1e3 * (t2 - t1):.1f} ms, np.interp onto {grid.size} points {1e3 * (t3 - t2):.1f} ms")
    finally:
        for p in (d_iq, d_rows, d_copy):
            p.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    main()
