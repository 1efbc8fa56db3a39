#!/usr/bin/env python3
"""Timing of the analog demodulator on one C3 second: 20e6 int8 IQ samples through
Channelizer(128, os=2), which leaves 128 channels of 312 500 complex64 samples (312.5 kHz) in HBM; then FM at R = 6 with
the default audio filter (34 taps per phase) and 75 us de-emphasis, and AM at the same shape with carrier removal.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  fm, am   one Demodulator.process_device call over all 128 channels of the second, next to its memory floor: 8 bytes in
           and 4 / R bytes out per channel sample at the copy rate
  split    the FM step again under `rocprofv3 --kernel-trace --stats`: the audio, post and history kernels separately
  numpy    for scale: the same three stages in float32 numpy on one host core, on 8 of the 128 channels, times 16

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per figure: warm-up calls, then the median of `--reps` (at least 20) single
calls, each between device events on the engine's stream the work is launched on.

    python tools/demodbench.py [--out profiles/demodbench.txt] [--reps 20] [--steps copy,fm]
"""
import csv
import functools
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

FS = 20e6
N_SEC = 20_000_000
M, OS, R = 128, 2, 6
TAU = 75e-6


def capture(n):
    """Noise: an FM carrier per channel would cost minutes of host time, and the kernels' work does not depend on the data."""
    rng = np.random.default_rng(4)
    return rng.integers(-128, 128, 2 * n).astype(np.int8)


def step_demod(args, mode):
    from topdogspectrumanalyser_amd import Channelizer, Demodulator, DeviceBuffer, SpectrumEngine, _native as nat
    D = M // OS
    n = N_SEC // D * D
    ny = n // D
    iq = capture(n)
    d_in = DeviceBuffer(iq.nbytes)
    d_in.put(iq)
    d_y = DeviceBuffer(8 * M * ny)
    kw = dict(deemphasis=TAU) if mode == "fm" else dict(remove_carrier=True)
    with SpectrumEngine(64) as eng, Channelizer(M, FS, OS) as bank, \
            Demodulator(mode, FS / D, R, M, max_host_samples=M, **kw) as dm:
        bank.process_device(eng, nat.IN_I8, d_in.ptr, n, d_y.ptr, ny)
        na = ny // R                             # a whole number of outputs per call: every call does the same work
        d_a = DeviceBuffer(4 * M * na)

        def call():
            dm.process_device(eng, d_y.ptr, na * R, ny, d_a.ptr, na)

        us, lo, hi = median_us(eng, call, args.warm, args.reps)
        eng.synchronize()
        taps = dm.taps.size
    ny = na * R
    floor = M * ny * (8 + 4.0 / R) / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    for p in (d_in, d_y, d_a):
        p.close()
    return dict(text=[
        f"{mode} R={R}: {M} channels x {ny} samples at {FS / D / 1e3:.1f} kHz, {taps // R} taps per phase, one-pole section on: "
        f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {floor:8.1f} us (8 bytes in, 4 / {R} out per channel sample at "
        f"the copy rate) = {100 * floor / us:5.1f}% of the time"])


def step_split(args):
    prof = shutil.which("rocprofv3")
    if not prof:
        return dict(text=["split: rocprofv3 not found; the kernels were not timed separately"])
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--step", "fm", "--reps", str(args.reps), "--warm", str(args.warm)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [row for row in csv.DictReader(f) if "demod_" in row.get("Name", "")]
        if r.returncode != 0 or not rows:
            return dict(text=[f"split: no kernel statistics (exit status {r.returncode}); the kernels were not timed separately"])
    text = []
    for row in sorted(rows, key=lambda q: q["Name"].split("demod_")[-1]):
        name = re.search(r"demod_\w+(<\d+>)?", row["Name"]).group(0)
        text.append(f"split fm R={R}: {name}: {int(row['Calls'])} calls, average {float(row['AverageNs']) / 1e3:9.1f} us "
                    f"(min {float(row['MinNs']) / 1e3:.1f}, max {float(row['MaxNs']) / 1e3:.1f}), under the profiler")
    return dict(text=text)


def step_numpy(args):
    from topdogspectrumanalyser_amd.demod import deemphasis_pole, design_audio_filter
    D, part = M // OS, 8
    ny = N_SEC // D
    rng = np.random.default_rng(5)
    y = (rng.standard_normal((part, ny)) + 1j * rng.standard_normal((part, ny))).astype(np.complex64)
    g = design_audio_filter(R)
    c = np.float32(deemphasis_pole(TAU, FS / D / R))
    t0 = time.perf_counter()
    for row in y:
        p = row[1:] * np.conj(row[:-1])
        d = np.arctan2(p.imag, p.real) * np.float32(1 / np.pi)
        a = np.convolve(d, g)[:d.size:R].astype(np.float32)
        out = np.empty_like(a)
        acc = np.float32(0)
        for m in range(a.size):                  # the recursion, as a host program would write it without scipy
            acc = c * acc + (np.float32(1) - c) * a[m]
            out[m] = acc
    dt = time.perf_counter() - t0
    return dict(text=[f"numpy fm R={R}: {part} of the {M} channels on one host core {dt:.2f} s; times {M // part} = "
                      f"{dt * M / part:.1f} s for the second"])


def header(args):
    return (f"analog demodulator on one C3 second through Channelizer({M}, os={OS}): {M} channels at {FS * OS / M / 1e3:.1f} kHz "
            f"in HBM; every device figure is the median of {args.reps} single calls after warm-up calls, between device events on "
            f"the stream the work runs on")


STEPS = dict(copy=step_copy, fm=functools.partial(step_demod, mode="fm"), am=functools.partial(step_demod, mode="am"),
             split=step_split, numpy=step_numpy)

if __name__ == "__main__":
    main(__file__, STEPS, header)
