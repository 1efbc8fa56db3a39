#!/usr/bin/env python3
"""Timing of the pulse analysis.

  copy      the box's device-to-device copy rate (1 GiB, torch), which the memory floors are stated against
  int8      a C3 second, 20e6 interleaved int8 samples in HBM: noise with a pulse train of 10 % duty (2000 pulses of
            1000 samples), PulseAnalyzer.process_device, next to its memory floor - the bytes read at the copy rate -
            and next to PowerStats.process_device on the same buffer
  c64       the same train as complex64
  dense     the pathological stream: every other sample on, 10e6 pulses of one sample (capacity 4096: the rest is counted)
  streams   256 channelizer streams of a C3 second: [256][78125] complex64, stride 78125 + 3, each with its own train

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream.  process_device does not wait, so a figure is the
device time of the passes alone.  The three kernels' shares are timed the same way with the other two masked out
(tdsa_pulse_debug_limits); they read what the last whole call left.  No time is fixed in advance: each figure stands
next to its memory floor and the power statistics' time.

    python tools/pulsebench.py [--out profiles/pulsebench.txt] [--reps 20] [--steps int8,dense]
"""
import os
import sys

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N = 20_000_000                    # a C3 second
PERIOD, WIDTH = 10_000, 1_000
STREAMS, PER_STREAM, GAP = 256, N // 256, 3
ON, OFF = 0.2, 0.05


def train_c64(shape, period=PERIOD, width=WIDTH):
    """Noise of power 0.005 with a carrier of power 0.5 at 0.05 cycles per sample switched on for `width` of every
    `period` samples; each row starts its train somewhere else."""
    rng = np.random.default_rng(8)
    x = np.empty(shape, dtype=np.complex64)
    x.real = rng.standard_normal(shape, dtype=np.float32) * 0.05
    x.imag = rng.standard_normal(shape, dtype=np.float32) * 0.05
    n = np.arange(shape[-1])
    rows = x.reshape(-1, shape[-1])
    for r in range(rows.shape[0]):
        gate = (n + 37 * r) % period < width
        rows[r, gate] += (0.7071 * np.exp(2j * np.pi * 0.05 * n[gate])).astype(np.complex64)
    return x


def train_i8(n=N):
    x = train_c64((n,))
    out = np.empty(2 * n, dtype=np.int8)
    out[0::2] = np.clip(np.rint(x.real * 128.0), -128, 127)
    out[1::2] = np.clip(np.rint(x.imag * 128.0), -128, 127)
    return out


def _figure(args, us, lo, hi, nbytes):
    fl = nbytes / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    return (f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {fl:7.1f} us ({nbytes / 1e6:.0f} MB read at the copy rate) = "
            f"{100 * fl / us:5.1f}% of the time")


def _run(args, data, n, fmt, streams=1, stride=None, capacity=4096):
    """The figures of process_device over `data` in HBM, the train of stream 0 and of the last stream after one call,
    and the power statistics' time on the same buffer."""
    from topdogspectrumanalyser_amd import DeviceBuffer, PowerStats, PulseAnalyzer
    with DeviceBuffer.of(data) as d, PulseAnalyzer(streams, capacity, max_host_samples=streams) as p, \
            PowerStats(streams, max_host_samples=streams) as ps:
        p.configure(ON, OFF)
        f = lambda: p.process_device(None, d.ptr, n, stride, fmt)
        whole = median_us(p, f, args.warm, args.reps)
        shares = []
        for k in range(3):
            p._debug_limits(passes=1 << k)
            shares.append(median_us(p, f, args.warm, args.reps)[0])
        p._debug_limits()
        p.reset()
        f()
        first, last = p.read(0), p.read(streams - 1)
        stat = median_us(ps, lambda: ps.process_device(None, d.ptr, n, stride, fmt), args.warm, args.reps)
        return whole, shares, first, last, stat


def _lines(args, head, nbytes, res):
    whole, shares, t, _, stat = res
    out = [f"{head}: {_figure(args, *whole, nbytes)}",
           f"      tile pass {shares[0]:.1f} us, stitch {shares[1]:.1f} us, emit {shares[2]:.1f} us, each launched alone; "
           f"PowerStats.process_device on the same buffer {stat[0]:.1f} us: the pulse analysis takes {whole[0] / stat[0]:.2f} x that"]
    if len(t) > 1:
        out.append(f"      stream 0: {t.n_pulses} pulses ({len(t)} stored, {t.n_lost} lost, {t.n_short} short), median width "
                   f"{np.median(t.width):.0f}, median PRI {np.median(t.pri()):.0f} samples, duty {100 * t.duty_cycle:.2f} %, median "
                   f"in-pulse frequency {np.nanmedian(t.freq):+.5f} cycles per sample, median mean power {np.median(t.mean_power):.3f}")
    return out


def step_int8(args):
    from topdogspectrumanalyser_amd import _native as nat
    res = _run(args, train_i8(), N, nat.IN_I8)
    assert res[2].n_pulses == N // PERIOD, res[2].n_pulses
    return dict(text=_lines(args, f"int8: {N} int8 samples, noise with a pulse train of {100 * WIDTH // PERIOD} % duty, one stream", 2 * N, res))


def step_c64(args):
    from topdogspectrumanalyser_amd import _native as nat
    res = _run(args, train_c64((N,)), N, nat.IN_C64)
    assert res[2].n_pulses == N // PERIOD, res[2].n_pulses
    return dict(text=_lines(args, f"c64: the same train as {N} complex64 samples", 8 * N, res))


def step_dense(args):
    from topdogspectrumanalyser_amd import _native as nat
    x = np.tile(np.array([90, 0, 0, 0], dtype=np.int8), N // 2)
    res = _run(args, x, N, nat.IN_I8)
    assert res[2].n_pulses == N // 2 and res[2].n_lost == N // 2 - 4096
    return dict(text=_lines(args, f"dense: {N} int8 samples, every other one on ({N // 2} pulses of one sample, capacity 4096)", 2 * N, res))


def step_streams(args):
    from topdogspectrumanalyser_amd import _native as nat
    stride = PER_STREAM + GAP
    x = train_c64((STREAMS, stride), 5000, 500)
    x[:, PER_STREAM:] = complex(3.0, 3.0)                 # the gaps would show as pulses
    res = _run(args, x, PER_STREAM, nat.IN_C64, STREAMS, stride, 64)
    assert res[2].n_total == PER_STREAM and 14 <= res[3].n_pulses <= 16
    return dict(text=_lines(args, f"streams: {STREAMS} streams of {PER_STREAM} complex64 samples (stride {stride}: every other stream by "
                                  f"elements), a train of 10 % duty each, one call", 8 * STREAMS * PER_STREAM, res))


def header(args):
    return (f"pulse analysis (tdsa_pulse_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream; the records stay on the device.  on_level {ON}, off_level {OFF}, min_width 1")


STEPS = dict(copy=step_copy, int8=step_int8, c64=step_c64, dense=step_dense, streams=step_streams)

if __name__ == "__main__":
    main(__file__, STEPS, header)
