#!/usr/bin/env python3
"""Timing of the symbol recovery.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  tick     one GUI tick: 16 384 complex64 samples at 4 samples per symbol as one segment (K = 4094, a 8192-point carrier
           transform), qpsk, SymbolSync.process_device with the samples and the symbols in HBM
  second   a C3-shaped second: 20e6 complex64 samples through DownConverter(D = 2, root-raised-cosine taps) leave 10e6 in
           HBM; analysed as 2441 segments of 4096 (K = 1022 each) in one call, next to its memory floor: 8 bytes read
           per sample and 8 K bytes written per segment at the copy rate
  numpy    for scale: the float64 contract (tests/symsync_contract.py) on the tick's segment on one host core

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream; a call ends when the segments' records are in host
memory, so the figure includes that copy and wait.

    python tools/symsyncbench.py [--out profiles/symsyncbench.txt] [--reps 20] [--steps copy,tick]
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
N_SEC = 20_000_000
D = 2
SEG = 4096


def signal(n, sps):
    """A qpsk stream through a rectangular pulse with a carrier, plus noise: cheap to make at 20e6 samples, and the
    kernel's work does not depend on the data."""
    rng = np.random.default_rng(4)
    sym = ((2 * rng.integers(0, 2, n // sps + 1) - 1) + 1j * (2 * rng.integers(0, 2, n // sps + 1) - 1)) / np.sqrt(2.0)
    x = np.repeat(sym, sps)[:n] * np.exp(1j * 0.002 * np.arange(n))
    x += 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def step_tick(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, SymbolSync
    x = signal(TICK, SPS)
    with SymbolSync(SPS, "qpsk") as s:
        K = s.symbols_per_segment(TICK)
        d_x, d_s = DeviceBuffer(x.nbytes), DeviceBuffer(8 * K)
        d_x.put(x)
        us, lo, hi = median_us(s, lambda: s.process_device(None, d_x.ptr, TICK, TICK, 1, d_s.ptr, K), args.warm, args.reps)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            s.process(x, TICK)
        host_us = (time.perf_counter() - t0) / args.reps * 1e6
        for p in (d_x, d_s):
            p.close()
    return dict(text=[
        f"tick: {TICK} samples at {SPS} samples per symbol, one segment, K = {K}, qpsk: {us:8.1f} us (min {lo:.1f}, max {hi:.1f}) "
        f"in device memory; from and to host memory (SymbolSync.process, wall clock, mean of {args.reps}) {host_us:8.1f} us"])


def step_second(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, DownConverter, SpectrumEngine, SymbolSync, _native as nat
    from topdogspectrumanalyser_amd.symbols import rrc_taps
    x = signal(N_SEC, SPS * D)
    ny = N_SEC // D
    n_seg = ny // SEG
    d_x, d_y = DeviceBuffer(x.nbytes), DeviceBuffer(8 * (ny + 8))
    d_x.put(x)
    with SpectrumEngine(64) as eng, DownConverter(D, 20e6, taps=rrc_taps(SPS * D, 0.35, 4)) as ddc, SymbolSync(SPS, "qpsk") as s:
        K = s.symbols_per_segment(SEG)
        d_s = DeviceBuffer(8 * K * n_seg)
        assert ddc.process_device(eng, nat.IN_C64, d_x.ptr, N_SEC, d_y.ptr) == ny
        eng.synchronize()
        us, lo, hi = median_us(s, lambda: s.process_device(None, d_y.ptr, SEG, SEG, n_seg, d_s.ptr, K), args.warm, args.reps)
        r = s.process_device(None, d_y.ptr, SEG, SEG, n_seg, d_s.ptr, K)
    floor = (8.0 * n_seg * SEG + 8.0 * K * n_seg) / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    for p in (d_x, d_y, d_s):
        p.close()
    return dict(text=[
        f"second: {N_SEC} samples through DownConverter(D = {D}, RRC) -> {ny} in HBM, {n_seg} segments of {SEG}, K = {K}: "
        f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {floor:8.1f} us (8 bytes read per sample, 8 K written per "
        f"segment at the copy rate) = {100 * floor / us:5.1f}% of the time; median timing quality {np.median(r.timing_quality):.3f}, "
        f"median lock {np.median(r.lock):.0f}, {int(np.count_nonzero(r.flags))} segments flagged"])


def step_numpy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import symsync_contract as sc
    x = signal(TICK, SPS).astype(np.complex128)
    ref = sc.reference_phase(sc.points("qpsk"), 4)
    sc.recover(x, SPS, 4, ref)
    t0 = time.perf_counter()
    for _ in range(5):
        sc.recover(x, SPS, 4, ref)
    dt = (time.perf_counter() - t0) / 5
    return dict(text=[f"numpy: the float64 contract on the tick's segment on one host core: {dt * 1e3:.1f} ms"])


def header(args):
    return (f"symbol recovery (tdsa_symsync_*): every device figure is the median of {args.reps} single calls after warm-up "
            f"calls, between device events on the handle's stream, records read back included")


STEPS = dict(copy=step_copy, tick=step_tick, second=step_second, numpy=step_numpy)

if __name__ == "__main__":
    main(__file__, STEPS, header)
