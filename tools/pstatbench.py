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

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream.  process_device does not wait, so a figure is the
device time of the pass alone.  No time is fixed in advance: each figure stands next to its memory floor.

    python tools/pstatbench.py [--out profiles/pstatbench.txt] [--reps 20] [--steps int8,constant]
"""
import os
import sys
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 20_000_000                    # a C3 second
STREAMS, PER_STREAM, GAP = 256, N // 256, 3


def noise_i8(n=N):
    rng = np.random.default_rng(7)
    return np.clip(np.rint(rng.standard_normal(2 * n, dtype=np.float32) * 24.0), -128, 127).astype(np.int8)


def noise_c64(shape):
    rng = np.random.default_rng(8)
    x = np.empty(shape, dtype=np.complex64)
    x.real = rng.standard_normal(shape, dtype=np.float32) * 0.1
    x.imag = rng.standard_normal(shape, dtype=np.float32) * 0.1
    return x


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


def header(args):
    return (f"power statistics (tdsa_pstat_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream; the state stays on the device")


STEPS = dict(copy=step_copy, int8=step_int8, constant=step_constant, c64=step_c64, streams=step_streams, scale=step_scale)

if __name__ == "__main__":
    main(__file__, STEPS, header, carry=("noise_us",))
