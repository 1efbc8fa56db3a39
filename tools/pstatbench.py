#!/usr/bin/env python3
"""Timing of the power statistics.

  copy      the box's device-to-device copy rate (1 GiB, torch), which the memory floors are stated against
  int8      a C3 second, 20e6 interleaved int8 samples of noise in HBM, PowerStats.process_device, next to its memory
            floor: the bytes read at the copy rate
  constant  the same length as a constant envelope: every sample in ONE bin and ONE octave, against the noise time
  c64       the same length as complex64 noise
  streams   256 channelizer streams of a C3 second: [256][78125] complex64, stride 78125 + 3, one call
  scale     for scale, on the int8 samples of `int8`: Constellation's density pass (no table: rms and the 128 x 128
            histogram), and the numpy contract (tests/pstat_contract.py) on one core

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  Per device figure:
warm-up calls, then the median of `--reps` (at least 20) single calls, each between device events on the handle's
stream.  process_device does not wait, so a figure is the device time of the pass alone.  No time is fixed in advance:
each figure stands next to its memory floor.

    python tools/pstatbench.py [--out profiles/pstatbench.txt] [--reps 20] [--steps int8,constant]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 20_000_000                    # a C3 second
STREAMS, PER_STREAM, GAP = 256, N // 256, 3
STEPS = ["copy", "int8", "constant", "c64", "streams", "scale"]
LIMIT_S = 240


def median_us(h, f, warm, reps):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        h.timer_begin()
        f()
        t.append(h.timer_end() * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def noise_i8(n=N):
    rng = np.random.default_rng(7)
    return np.clip(np.rint(rng.standard_normal(2 * n, dtype=np.float32) * 24.0), -128, 127).astype(np.int8)


def noise_c64(shape):
    rng = np.random.default_rng(8)
    x = np.empty(shape, dtype=np.complex64)
    x.real = rng.standard_normal(shape, dtype=np.float32) * 0.1
    x.imag = rng.standard_normal(shape, dtype=np.float32) * 0.1
    return x


def step_copy(args):
    import torch
    x = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    x.fill_(1.0)
    for _ in range(3):
        y.copy_(x)
    t = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y.copy_(x)
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e-3)
    moved = 2 * x.numel() * 4
    return dict(copy_bps=moved / float(np.median(t)), text=[
        f"copy: 1 GiB device to device, median of {args.reps}: {moved / np.median(t) / 1e12:.2f} TB/s read + written"])


def _figure(args, us, lo, hi, nbytes):
    fl = nbytes / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    return (f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {fl:7.1f} us ({nbytes / 1e6:.0f} MB read at the copy rate) = "
            f"{100 * fl / us:5.1f}% of the time")


def _run(args, data, n, fmt, streams=1, stride=None):
    """(median us, min, max, the statistics of one call) of process_device over `data` in HBM."""
    from topdogspectrumanalyser_amd import DeviceBuffer, PowerStats
    with DeviceBuffer.of(data) as d, PowerStats(streams, max_host_samples=streams) as p:
        f = lambda: p.process_device(None, d.ptr, n, stride, fmt)
        us, lo, hi = median_us(p, f, args.warm, args.reps)
        p.reset()
        f()
        return us, lo, hi, p.read()


def _table(s, stream=0):
    lv = s.level_db([0.1, 0.01, 0.001, 0.0001], stream)
    return f"PAPR {s.papr_db[stream]:.2f} dB; 10 % / 1 % / 0.1 % / 0.01 % at " + " / ".join(f"{v:.2f}" for v in lv) + " dB"


def step_int8(args):
    from topdogspectrumanalyser_amd import _native as nat
    us, lo, hi, s = _run(args, noise_i8(), N, nat.IN_I8)
    return dict(noise_us=us, text=[f"int8: {N} int8 samples of noise, one stream: {_figure(args, us, lo, hi, 2 * N)}",
                                   f"      {_table(s)}; {int(np.count_nonzero(s.hist[0]))} bins and "
                                   f"{int(np.count_nonzero(s.msum[0]))} octaves hold samples"])


def step_constant(args):
    from topdogspectrumanalyser_amd import _native as nat
    x = np.tile(np.array([48, -64], dtype=np.int8), N)
    us, lo, hi, s = _run(args, x, N, nat.IN_I8)
    ratio = us / args.noise_us if args.noise_us else float("nan")
    return dict(text=[f"constant: {N} int8 samples of one value (a constant envelope), one stream: {_figure(args, us, lo, hi, 2 * N)}",
                      f"      {ratio:.2f} x the noise time; PAPR {s.papr_db[0]:.2f} dB, {int(np.count_nonzero(s.hist[0]))} bin and "
                      f"{int(np.count_nonzero(s.msum[0]))} octave hold samples"])


def step_c64(args):
    from topdogspectrumanalyser_amd import _native as nat
    us, lo, hi, s = _run(args, noise_c64(N), N, nat.IN_C64)
    return dict(text=[f"c64: {N} complex64 samples of noise, one stream: {_figure(args, us, lo, hi, 8 * N)}", f"      {_table(s)}"])


def step_streams(args):
    from topdogspectrumanalyser_amd import _native as nat
    stride = PER_STREAM + GAP
    x = noise_c64((STREAMS, stride))
    x[:, PER_STREAM:] = np.nan
    us, lo, hi, s = _run(args, x, PER_STREAM, nat.IN_C64, STREAMS, stride)
    assert int(s.n_nan.sum()) == 0 and (s.n_total == PER_STREAM).all()
    papr = s.papr_db
    return dict(text=[f"streams: {STREAMS} streams of {PER_STREAM} complex64 samples (stride {stride}: every other stream by elements), "
                      f"one call: {_figure(args, us, lo, hi, 8 * STREAMS * PER_STREAM)}",
                      f"      PAPR over the streams {papr.min():.2f} .. {papr.max():.2f} dB"])


def step_scale(args):
    import pstat_contract as pc
    from topdogspectrumanalyser_amd import Constellation, DeviceBuffer, _native as nat
    x = noise_i8()
    with DeviceBuffer.of(x) as d, Constellation(max_host_samples=1, modulation="none") as c, \
            DeviceBuffer(4 * c.bins * c.bins) as counts:
        f = lambda: c.process_segments(None, d.ptr, nat.IN_I8, N, N, 1, counts.ptr)
        for _ in range(args.warm):
            f()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f()                                     # returns with rms and EVM in host memory
            t.append((time.perf_counter() - t0) * 1e6)
    t0 = time.perf_counter()
    pc.State().accumulate(x, pc.I8)
    cpu = time.perf_counter() - t0
    return dict(text=[
        f"scale: on the samples of `int8`, Constellation.process_segments (no table: rms and the {c.bins} x {c.bins} density "
        f"histogram, one segment), wall time of the call: {np.median(t):9.1f} us (min {np.min(t):.1f}, max {np.max(t):.1f}); the numpy "
        f"contract on one core: {cpu * 1e3:.0f} ms"])


def run_step(args):
    return dict(copy=step_copy, int8=step_int8, constant=step_constant, c64=step_c64, streams=step_streams,
                scale=step_scale)[args.step](args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--steps", default=",".join(STEPS), help="the steps to run, in the order above")
    ap.add_argument("--copy-bps", dest="copy_bps", type=float, default=0.0)
    ap.add_argument("--noise-us", dest="noise_us", type=float, default=0.0)
    args = ap.parse_args()
    args.reps = max(args.reps, 20)
    if args.step:
        print("RESULT " + json.dumps(run_step(args)), flush=True)
        return
    lines = [f"power statistics (tdsa_pstat_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
             f"between device events on the handle's stream; the state stays on the device"]
    print(lines[0], flush=True)
    copy_bps, noise_us, failed = 0.0, 0.0, False
    for step in [st for st in STEPS if st in args.steps.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warm", str(args.warm),
               "--copy-bps", repr(copy_bps), "--noise-us", repr(noise_us)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"{step}: no result within {LIMIT_S} s; stopping")
            print(lines[-1], flush=True)
            failed = True
            break
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            lines.append(f"{step}: exit status {r.returncode}; stopping\n{r.stderr[-1500:]}")
            print(lines[-1], flush=True)
            failed = True
            break
        res = json.loads(res[-1][7:])
        copy_bps = res.get("copy_bps", copy_bps)
        noise_us = res.get("noise_us", noise_us)
        for ln in res["text"]:
            print(ln, flush=True)
            lines.append(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
