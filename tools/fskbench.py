#!/usr/bin/env python3
"""Timing of the FSK analysis.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floors are stated against
  tick     one GUI tick: 16 384 complex64 samples at 4 samples per symbol as one segment (K = 4093), 2 levels,
           FskAnalyzer.process_device with the samples, the levels and the indices in HBM; SymbolSync (qpsk) on the same
           samples beside it
  second   a C3-shaped second: 1e7 complex64 samples in HBM analysed as 2441 segments of 4096 in one call, next to its
           memory floor - 8 bytes read per sample, 4 K + K bytes written per segment at the copy rate - and to SymbolSync
           on the same shape
  freq     the same second as float32 that is a frequency already: 4 bytes read per sample
  numpy    for scale: the float64 contract (tests/fsk_contract.py) on the tick's segment on one host core

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream; a call ends when the segments' records are in host
memory, so the figure includes that copy and wait.

    python tools/fskbench.py [--out profiles/fskbench.txt] [--reps 20] [--steps copy,tick]
"""
import os
import sys
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SPS = 4
TICK = 16384
N_SEC = 10_000_000
SEG = 4096


def frequency(n, sps):
    """A 2-level frequency stream in half turns per sample, rectangular pulses at h = 0.5, plus noise: cheap to make at
    1e7 samples, and the kernel's work does not depend on the data."""
    rng = np.random.default_rng(4)
    f = np.repeat((2.0 * rng.integers(0, 2, n // sps + 1) - 1.0) * (0.5 / sps), sps)[:n]
    return f + 0.004 + 1e-3 * rng.standard_normal(n)


def signal(n, sps):
    return np.exp(1j * np.pi * np.cumsum(frequency(n, sps))).astype(np.complex64)


def _symsync_us(args, d_x, seg, n_seg):
    """SymbolSync's time on the same samples and the same segments."""
    from topdogspectrumanalyser_amd import DeviceBuffer, SymbolSync
    with SymbolSync(SPS, "qpsk") as s:
        K = s.symbols_per_segment(seg)
        with DeviceBuffer(8 * K * n_seg) as d_s:
            return median_us(s, lambda: s.process_device(None, d_x.ptr, seg, seg, n_seg, d_s.ptr, K), args.warm, args.reps)[0]


def step_tick(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, FskAnalyzer
    x = signal(TICK, SPS)
    with FskAnalyzer(SPS, 2) as a, DeviceBuffer(x.nbytes) as d_x:
        K = a.symbols_per_segment(TICK)
        d_x.put(x)
        with DeviceBuffer(4 * K) as d_v, DeviceBuffer(K) as d_i:
            us, lo, hi = median_us(a, lambda: a.process_device(None, d_x.ptr, TICK, TICK, 1, d_v.ptr, K, d_i.ptr), args.warm, args.reps)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            a.process(x, TICK)
        host_us = (time.perf_counter() - t0) / args.reps * 1e6
        sym_us = _symsync_us(args, d_x, TICK, 1)
    return dict(text=[
        f"tick: {TICK} samples at {SPS} samples per symbol, one segment, K = {K}, 2 levels, B = L = {a.boxcar}: {us:8.1f} us "
        f"(min {lo:.1f}, max {hi:.1f}) in device memory; from and to host memory (FskAnalyzer.process, wall clock, mean of "
        f"{args.reps}) {host_us:8.1f} us; SymbolSync (qpsk) on the same samples {sym_us:8.1f} us"])


def _second(args, kind):
    from topdogspectrumanalyser_amd import DeviceBuffer, FskAnalyzer
    n_seg = N_SEC // SEG
    x = signal(N_SEC, SPS) if kind == "iq" else frequency(N_SEC, SPS).astype(np.float32)
    unit = x.itemsize
    with FskAnalyzer(SPS, 2, input=kind) as a, DeviceBuffer(x.nbytes) as d_x:
        K = a.symbols_per_segment(SEG)
        d_x.put(x)
        with DeviceBuffer(4 * K * n_seg) as d_v, DeviceBuffer(K * n_seg) as d_i:
            call = lambda: a.process_device(None, d_x.ptr, SEG, SEG, n_seg, d_v.ptr, K, d_i.ptr)      # noqa: E731
            us, lo, hi = median_us(a, call, args.warm, args.reps)
            r = call()
        sym = f"; SymbolSync (qpsk) on the same shape {_symsync_us(args, d_x, SEG, n_seg):9.1f} us" if kind == "iq" else ""
    floor = (float(unit) * n_seg * SEG + 5.0 * K * n_seg) / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    return dict(text=[
        f"{'second' if kind == 'iq' else 'freq'}: {N_SEC} {x.dtype} samples in HBM, {n_seg} segments of {SEG}, K = {K}: {us:9.1f} us "
        f"(min {lo:.1f}, max {hi:.1f}); memory floor {floor:8.1f} us ({unit} bytes read per sample, 4 K + K written per segment "
        f"at the copy rate) = {100 * floor / us:5.1f}% of the time; median timing quality {np.median(r.timing_quality):.3f}, "
        f"median FSK error {np.median(r.fsk_error):.4f}, {int(np.count_nonzero(r.flags))} segments flagged{sym}"])


def step_second(args):
    return _second(args, "iq")


def step_freq(args):
    return _second(args, "freq")


def step_numpy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fsk_contract as fc
    x = signal(TICK, SPS).astype(np.complex128)
    fc.analyse(x, SPS, 2)
    t0 = time.perf_counter()
    for _ in range(5):
        fc.analyse(x, SPS, 2)
    dt = (time.perf_counter() - t0) / 5
    return dict(text=[f"numpy: the contract on the tick's segment on one host core: {dt * 1e3:.1f} ms"])


def header(args):
    return (f"FSK analysis (tdsa_fsk_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream, records read back included")


STEPS = dict(copy=step_copy, tick=step_tick, second=step_second, freq=step_freq, numpy=step_numpy)

if __name__ == "__main__":
    main(__file__, STEPS, header)
