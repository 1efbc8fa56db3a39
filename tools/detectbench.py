#!/usr/bin/env python3
"""Timing of the signal detection.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  second   a C3-shaped second: 2440 rows of 16384 bins in HBM, noise with emissions over about 3 % of the bins,
           SignalDetector.process_device (median floor, 10 dB margin, max_gap 2, min_width 3, 16 records per row), next
           to its memory floor: 4 bytes read per bin at the copy rate
  worst    the same shape with every other bin above the threshold: 8192 runs per row, 64 records per row
  scale    tdsa_rows_marker_peaks and tdsa_rows_stats on the rows of `second`, for scale (their code is not touched by
           the detector), between events on the plan's stream

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream; a call ends when the records are in host memory, so the
figure includes that copy and wait.  No time is fixed in advance: each figure stands next to its memory floor.

    python tools/detectbench.py [--out profiles/detectbench.txt] [--reps 20] [--steps copy,second]
"""
import os
import sys

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_ROWS, N_BINS = 2440, 16384


def capture(kind):
    """[N_ROWS][N_BINS] float32 dB rows: noise around -100 dB; "second": twelve emissions of 24 .. 56 bins whose level
    and edges move a little from row to row (about 3 % of the bins); "worst": every odd bin 60 dB up."""
    rng = np.random.default_rng(6)
    rows = (-100.0 + 2.0 * rng.standard_normal((N_ROWS, N_BINS), dtype=np.float32)).astype(np.float32)
    if kind == "worst":
        rows[:, 1::2] += np.float32(60.0)
        return rows
    centres = rng.integers(200, N_BINS - 200, 12)
    widths = rng.integers(24, 57, 12)
    for c, w in zip(centres, widths):
        jit = rng.integers(-2, 3, N_ROWS)
        for r in range(N_ROWS):
            a = int(c - w // 2 + jit[r])
            rows[r, a:a + w] += np.float32(40.0)
    return rows


def floor_us(copy_bps):
    return 4.0 * N_ROWS * N_BINS / copy_bps * 1e6 if copy_bps else float("nan")


def _detect(args, kind, **kw):
    from topdogspectrumanalyser_amd import DeviceBuffer, SignalDetector
    rows = capture(kind)
    d_rows = DeviceBuffer(rows.nbytes)
    d_rows.put(rows)
    with SignalDetector(N_BINS, max_host_rows=1, **kw) as d:
        us, lo, hi = median_us(d, lambda: d.process_device(None, d_rows.ptr, N_ROWS), args.warm, args.reps)
        r = d.process_device(None, d_rows.ptr, N_ROWS)
    d_rows.close()
    fl = floor_us(args.copy_bps)
    return r, (f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {fl:7.1f} us (4 bytes read per bin at the copy "
               f"rate) = {100 * fl / us:5.1f}% of the time")


def step_second(args):
    r, fig = _detect(args, "second", margin_db=10.0, max_gap=2, min_width=3, max_signals=16)
    occ = float(np.mean(r.n_over)) / N_BINS
    return dict(text=[
        f"second: {N_ROWS} rows of {N_BINS} bins in HBM, {100 * occ:.1f}% of the bins above the threshold, median "
        f"{int(np.median(r.n_found))} emissions per row (max_gap 2, min_width 3, 16 records): {fig}"])


def step_worst(args):
    r, fig = _detect(args, "worst", floor_quantile=0.25, margin_db=30.0, max_gap=0, min_width=1, max_signals=64)
    return dict(text=[
        f"worst: the same shape, every other bin above the threshold, median {int(np.median(r.n_found))} runs per row, "
        f"64 records: {fig}"])


def step_scale(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, analytics as an
    rows = capture("second")
    d_rows = DeviceBuffer(rows.nbytes)
    d_rows.put(rows)
    freq = np.linspace(90e6, 110e6, N_BINS)
    with SpectrumEngine(64) as eng:
        mk = median_us(eng, lambda: an.rows_marker_peaks(eng, d_rows.ptr, N_ROWS, N_BINS), args.warm, args.reps)
        st = median_us(eng, lambda: an.rows_stats(eng, d_rows.ptr, N_ROWS, N_BINS, freq, (95e6, 105e6)), args.warm, args.reps)
    d_rows.close()
    fl = floor_us(args.copy_bps)
    return dict(text=[
        f"scale: on the rows of `second`, tdsa_rows_marker_peaks (reference defaults) {mk[0]:9.1f} us (min {mk[1]:.1f}, max "
        f"{mk[2]:.1f}); tdsa_rows_stats (peak, argmax, a band of half the row) {st[0]:9.1f} us (min {st[1]:.1f}, max {st[2]:.1f}); "
        f"the same memory floor, {fl:7.1f} us"])


def header(args):
    return (f"signal detection (tdsa_detect_*): every device figure is the median of {args.reps} single calls after warm-up "
            f"calls, between device events on the handle's stream, records read back included")


STEPS = dict(copy=step_copy, second=step_second, worst=step_worst, scale=step_scale)

if __name__ == "__main__":
    main(__file__, STEPS, header)
