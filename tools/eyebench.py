#!/usr/bin/env python3
"""Timing of the eye diagrams.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floors are stated against
  tick     one GUI tick: 16 384 complex64 samples at 4 samples per symbol as one segment (K = 4094), 32 points per symbol,
           128 rows, I and Q eyes on a fixed clock, EyeDiagram.process_device with the samples in HBM and no traces;
           SymbolSync (qpsk) on the same samples beside it
  second   a C3-shaped second: 1e7 complex64 samples in HBM folded as 2441 segments of 4096 in one call, next to its
           memory floor - 8 bytes read per sample at the copy rate, plus the merge's atomics, counted - to its FP32 issue
           floor for the 8 points a sample gives, and to SymbolSync on the same shape
  fm       the same second through the discriminator and the boxcar into one eye, next to FskAnalyzer on the same shape
  numpy    for scale: the float64 contract (tests/eye_contract.py) on the tick's segment on one host core

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream.  An eye call does not wait for its kernel and hands
nothing back; the producers' calls end when their records are in host memory.

    python tools/eyebench.py [--out profiles/eyebench.txt] [--reps 20] [--steps copy,tick]
"""
import os
import sys
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SPS = 4
POINTS, ROWS = 32, 128
TICK = 16384
N_SEC = 10_000_000
SEG = 4096
# FP32 instructions of one point, counted from tdsa_symsync_math.hpp and tdsa_eye.hip: mu 2 (convert, scale), the
# coefficients 15 (three sums, twelve products), the interpolation 4 per part, the rotation 13 (angle 2, series 4, the two
# parts 3 each, the table's entry aside), the product 4, a row 2 per eye
FP32_PER_POINT = {"iq": 2 + 15 + 8 + 13 + 4 + 4, "fm": 2 + 15 + 4 + 2}
LANES_PER_S = 256 * 128 * 2.4e9          # 256 CUs x 4 SIMD-32 at 2.4 GHz: FP32 instructions per lane the device issues


def signal(n, sps):
    """Unit-power QPSK-like samples with a rectangular pulse and a little noise: cheap to make at 1e7 samples, and the
    kernel's work does not depend on the data (a clean signal's hot bins are the slow case of its LDS adds)."""
    rng = np.random.default_rng(4)
    sym = ((2.0 * rng.integers(0, 2, n // sps + 1) - 1.0) + 1j * (2.0 * rng.integers(0, 2, n // sps + 1) - 1.0)) / np.sqrt(2.0)
    x = np.repeat(sym, sps)[:n] + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def fm_signal(n, sps):
    rng = np.random.default_rng(4)
    f = np.repeat((2.0 * rng.integers(0, 2, n // sps + 1) - 1.0) * (0.5 / sps), sps)[:n] + 0.004 + 1e-3 * rng.standard_normal(n)
    return np.exp(1j * np.pi * np.cumsum(f)).astype(np.complex64)


def _producer_us(args, kind, d_x, seg, n_seg):
    """SymbolSync's (iq) or FskAnalyzer's (fm) time on the same samples and the same segments, measured here."""
    from topdogspectrumanalyser_amd import DeviceBuffer, FskAnalyzer, SymbolSync
    with (SymbolSync(SPS, "qpsk") if kind == "iq" else FskAnalyzer(SPS, 2)) as s:
        K = s.symbols_per_segment(seg)
        with DeviceBuffer(8 * K * n_seg) as d_s:
            return median_us(s, lambda: s.process_device(None, d_x.ptr, seg, seg, n_seg, d_s.ptr, K), args.warm, args.reps)[0]


def _eye(kind):
    from topdogspectrumanalyser_amd import EyeDiagram
    rng = (-1.5, 1.5) if kind == "iq" else (-0.3, 0.3)
    return EyeDiagram(SPS, kind, points=POINTS, rows=ROWS, v_range=rng, max_segments=N_SEC // SEG)


def step_tick(args):
    from topdogspectrumanalyser_amd import DeviceBuffer
    x = signal(TICK, SPS)
    with _eye("iq") as e, DeviceBuffer(x.nbytes) as d_x:
        K = e.symbols_per_segment(TICK)
        d_x.put(x)
        ck = e.clocks(delta=2.0)
        us, lo, hi = median_us(e, lambda: e.process_device(None, d_x.ptr, TICK, TICK, 1, ck), args.warm, args.reps)
        img = e.read()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            e.process(x, TICK, ck)
        host_us = (time.perf_counter() - t0) / args.reps * 1e6
        sym_us = _producer_us(args, "iq", d_x, TICK, 1)
    return dict(text=[
        f"tick: {TICK} samples at {SPS} samples per symbol, one segment, K = {K}, {POINTS} points x {ROWS} rows, I and Q: {us:8.1f} us "
        f"(min {lo:.1f}, max {hi:.1f}) in device memory, {int(img.n_points[0]) // (args.warm + args.reps)} points per eye and call; "
        f"from host memory (EyeDiagram.process, wall clock, mean of {args.reps}) {host_us:8.1f} us; SymbolSync (qpsk) on the same "
        f"samples {sym_us:8.1f} us: the eye takes {us / sym_us:.2f} of it"])


def _second(args, kind):
    from topdogspectrumanalyser_amd import DeviceBuffer
    n_seg = N_SEC // SEG
    x = signal(N_SEC, SPS) if kind == "iq" else fm_signal(N_SEC, SPS)
    with _eye(kind) as e, DeviceBuffer(x.nbytes) as d_x:
        K = e.symbols_per_segment(SEG)
        d_x.put(x)
        ck = e.clocks(delta=2.0, n_seg=n_seg)
        us, lo, hi = median_us(e, lambda: e.process_device(None, d_x.ptr, SEG, SEG, n_seg, ck), args.warm, args.reps)
        img = e.read()
        prod_us = _producer_us(args, kind, d_x, SEG, n_seg)
    calls = args.warm + args.reps
    points = e.eyes * n_seg * (K - 2) * POINTS
    assert int(img.n_points.sum()) == points * calls and img.segments == n_seg * calls
    mem = 8.0 * n_seg * SEG / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    fp32 = n_seg * (K - 2) * POINTS * FP32_PER_POINT[kind] / LANES_PER_S * 1e6
    inside = int(np.count_nonzero(img.counts))
    who = "SymbolSync (qpsk)" if kind == "iq" else "FskAnalyzer (2 levels)"
    return dict(text=[
        f"{'second' if kind == 'iq' else 'fm'}: {N_SEC} complex64 samples in HBM, {n_seg} segments of {SEG}, K = {K}, {POINTS} points x {ROWS} "
        f"rows, {e.eyes} eye(s), {points} points: {us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {mem:7.1f} us (8 bytes read "
        f"per sample at the copy rate) = {100 * mem / us:5.1f}% of the time, the merge adds at most {inside} 8-byte atomics per "
        f"workgroup (the bins in use); FP32 issue floor {fp32:7.1f} us ({FP32_PER_POINT[kind]} instructions per point, "
        f"{POINTS // SPS} points per sample and eye pair) = {100 * fp32 / us:5.1f}%; {who} on the same shape {prod_us:9.1f} us: the eye "
        f"takes {us / prod_us:.2f} of it"])


def step_second(args):
    return _second(args, "iq")


def step_fm(args):
    return _second(args, "fm")


def step_numpy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eye_contract as ec
    x = signal(TICK, SPS).astype(np.complex128)
    step = ec.step_of(SPS)

    def once():
        tr = ec.traces(x, ec.IQ, 1, step, POINTS, (2 << 32, 0, 0)).astype(np.complex64)
        return ec.bin_traces(tr, -1.5, 1.5, ROWS)
    once()
    t0 = time.perf_counter()
    for _ in range(3):
        once()
    dt = (time.perf_counter() - t0) / 3
    return dict(text=[f"numpy: the contract on the tick's segment on one host core: {dt * 1e3:.1f} ms"])


def header(args):
    return (f"Eye diagrams (tdsa_eye_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream")


STEPS = dict(copy=step_copy, tick=step_tick, second=step_second, fm=step_fm, numpy=step_numpy)

if __name__ == "__main__":
    main(__file__, STEPS, header)
