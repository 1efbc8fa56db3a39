#!/usr/bin/env python3
"""Timing of the modulation quality stage.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  tick     one GUI tick: the K = 4094 symbols SymbolSync makes of 16 384 samples at 4 samples per symbol, one row in HBM,
           16qam, ModQuality.process_device with indices and no error vectors; SymbolSync (16qam) on those samples beside it
  second   a C3-shaped second: 2441 rows of K = 1022 symbols (1e7 samples in segments of 4096) in one call, next to its
           memory floor - 8 bytes read and 1 byte written per symbol at the copy rate - and to SymbolSync on the same shape
  numpy    for scale: the contract (tests/modq_contract.py) on the tick's row on one host core

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream.  Both stages' calls end when their records are in host
memory.

    python tools/modqbench.py [--out profiles/modqbench.txt] [--reps 20] [--steps copy,tick]
"""
import os
import sys
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SPS = 4
MOD = "16qam"
TICK = 16384
N_SEC = 10_000_000
SEG = 4096


def symbols(n, mod=MOD):
    """n random points of the table through a gain, the small turn a carrier recovery leaves and an offset, with a little noise."""
    from topdogspectrumanalyser_amd.analytics import constellation_points
    rng = np.random.default_rng(4)
    t = np.asarray(constellation_points(mod), dtype=np.float64)
    i = rng.integers(0, t.shape[0], n)
    y = 0.85 * np.exp(0.02j) * (t[i, 0] + 1j * t[i, 1]) + (0.02 - 0.01j) + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return y.astype(np.complex64)


def _sync_us(args, seg, n_seg):
    """SymbolSync's time on the samples that give the same rows, measured here."""
    from topdogspectrumanalyser_amd import DeviceBuffer, SymbolSync
    x = np.repeat(symbols(n_seg * seg // SPS + 1), SPS)[:n_seg * seg]
    with SymbolSync(SPS, MOD) as s, DeviceBuffer.of(x) as d_x:
        K = s.symbols_per_segment(seg)
        with DeviceBuffer(8 * K * n_seg) as d_s:
            return K, median_us(s, lambda: s.process_device(None, d_x.ptr, seg, seg, n_seg, d_s.ptr, K), args.warm, args.reps)[0]


def _rows(args, seg, n_seg):
    """(K, median, min, max, the last call's result, SymbolSync's median) of n_seg rows of the K symbols a segment gives."""
    from topdogspectrumanalyser_amd import DeviceBuffer, ModQuality
    K, sync_us = _sync_us(args, seg, n_seg)
    y = symbols(K * n_seg)
    with ModQuality(MOD) as m, DeviceBuffer.of(y) as d_y, DeviceBuffer(K * n_seg) as d_i:
        last = []
        us, lo, hi = median_us(m, lambda: last.append(m.process_device(None, d_y.ptr, K, K, n_seg, d_i.ptr, K)), args.warm, args.reps)
    return K, us, lo, hi, last[-1], sync_us


def step_tick(args):
    from topdogspectrumanalyser_amd import ModQuality
    K, us, lo, hi, r, sync_us = _rows(args, TICK, 1)
    y = symbols(K)
    with ModQuality(MOD) as m:
        t0 = time.perf_counter()
        for _ in range(args.reps):
            m.process(y)
        host_us = (time.perf_counter() - t0) / args.reps * 1e6
    return dict(text=[
        f"tick: one row of K = {K} symbols ({TICK} samples at {SPS} samples per symbol), {MOD}: {us:8.1f} us (min {lo:.1f}, max {hi:.1f}) "
        f"in device memory, evm_rms {float(r.evm_rms[0]):.4f}, changed {int(r.changed[0])}; from host memory (ModQuality.process, wall "
        f"clock, mean of {args.reps}) {host_us:8.1f} us; SymbolSync ({MOD}) on the samples {sync_us:8.1f} us: this stage takes "
        f"{us / sync_us:.2f} of it"])


def step_second(args):
    n_seg = N_SEC // SEG
    K, us, lo, hi, r, sync_us = _rows(args, SEG, n_seg)
    assert not r.flags.any()
    mem = 9.0 * n_seg * K / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    return dict(text=[
        f"second: {n_seg} rows of K = {K} symbols ({N_SEC} samples in segments of {SEG}), {MOD}, {n_seg * K} symbols: {us:9.1f} us "
        f"(min {lo:.1f}, max {hi:.1f}), {n_seg * K / us:.0f} symbols per us; memory floor {mem:7.1f} us (8 bytes read and 1 byte "
        f"written per symbol at the copy rate) = {100 * mem / us:5.1f}% of the time; SymbolSync ({MOD}) on the same shape "
        f"{sync_us:9.1f} us: this stage takes {us / sync_us:.2f} of it"])


def step_numpy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modq_contract as mc
    K = ((TICK - 4) << 32) // (SPS << 32) - 1
    y, tab = symbols(K), mc.table(MOD)
    mc.analyse(y, tab)
    t0 = time.perf_counter()
    for _ in range(3):
        mc.analyse(y, tab)
    dt = (time.perf_counter() - t0) / 3
    return dict(text=[f"numpy: the contract on the tick's row on one host core: {dt * 1e3:.1f} ms"])


def header(args):
    return (f"Modulation quality (tdsa_modq_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream")


STEPS = dict(copy=step_copy, tick=step_tick, second=step_second, numpy=step_numpy)

if __name__ == "__main__":
    main(__file__, STEPS, header)
