#!/usr/bin/env python3
"""Timing of the channel measurements.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  second   a C3-shaped second: 2440 rows of 16384 bins in HBM, noise with one wide emission and its skirts,
           ChannelMeasure.process_device with a main channel and four adjacent channels, the occupied bandwidth of the
           whole row at 0.99, the 26 dB width and a limit line relative to the main channel's peak, next to its memory
           floor: 4 bytes read per bin at the copy rate
  parts    the same rows with less to do, to see what each part costs: one channel and no limit line; sixteen channels
           of the whole row
  scale    tdsa_detect (SignalDetector.process_device, detectbench's `second` parameters) and tdsa_rows_stats on the rows
           of `second`, for scale (their code is not touched by the measurements)

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream; a call ends when the records are in host memory, so the
figure includes that copy and wait.  No time is fixed in advance: each figure stands next to its memory floor.

    python tools/measbench.py [--out profiles/measbench.txt] [--reps 20] [--steps copy,second]
"""
import os
import sys

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_ROWS, N_BINS = 2440, 16384
FREQ = np.linspace(90e6, 110e6, N_BINS)
CENTRE, BANDWIDTH, SPACING = 100e6, 1.5e6, 2e6


def capture():
    """[N_ROWS][N_BINS] float32 dB rows: noise around -100 dB, a 1.5 MHz emission at -40 dB whose level moves a little
    from row to row, skirts that fall 30 dB per channel spacing on either side."""
    rng = np.random.default_rng(6)
    rows = (-100.0 + 2.0 * rng.standard_normal((N_ROWS, N_BINS), dtype=np.float32)).astype(np.float32)
    off = np.abs(FREQ - CENTRE)
    shape = np.where(off <= 0.5 * BANDWIDTH, 0.0, -30.0 * (off - 0.5 * BANDWIDTH) / SPACING - 25.0).astype(np.float32)
    level = (-40.0 + 0.5 * rng.standard_normal(N_ROWS)).astype(np.float32)
    return np.maximum(rows, level[:, None] + shape[None, :])


def floor_us(copy_bps):
    return 4.0 * N_ROWS * N_BINS / copy_bps * 1e6 if copy_bps else float("nan")


def _figure(args, us, lo, hi):
    fl = floor_us(args.copy_bps)
    return (f"{us:9.1f} us (min {lo:.1f}, max {hi:.1f}); memory floor {fl:7.1f} us (4 bytes read per bin at the copy rate) = "
            f"{100 * fl / us:5.1f}% of the time")


def _measure(args, d_rows, channels, **kw):
    from topdogspectrumanalyser_amd import ChannelMeasure
    with ChannelMeasure(N_BINS, channels, max_host_rows=1, **kw) as m:
        us, lo, hi = median_us(m, lambda: m.process_device(None, d_rows.ptr, N_ROWS), args.warm, args.reps)
        r = m.process_device(None, d_rows.ptr, N_ROWS)
    return r, _figure(args, us, lo, hi)


def _plan_and_line():
    from topdogspectrumanalyser_amd import channel_plan, limit_line
    plan = channel_plan(FREQ, CENTRE, BANDWIDTH, SPACING, n_adjacent=2)
    line = limit_line(FREQ, [(-5e6, -45.0), (-1e6, -15.0), (-0.76e6, 3.0), (0.76e6, 3.0), (1e6, -15.0), (5e6, -45.0)], CENTRE)
    return plan, line


def step_second(args):
    from topdogspectrumanalyser_amd import DeviceBuffer
    plan, line = _plan_and_line()
    with DeviceBuffer.of(capture()) as d_rows:
        r, fig = _measure(args, d_rows, plan, fraction=0.99, xdb=26.0, limit=line, limit_relative=True)
    bw = (FREQ[-1] - FREQ[0]) / (N_BINS - 1)
    acpr = np.median(r.acpr_db(), axis=0)
    width = float(np.median(r.x_hi - r.x_lo)) * bw
    return dict(text=[
        f"second: {N_ROWS} rows of {N_BINS} bins in HBM, main + 4 adjacent channels of {plan[0][1] - plan[0][0] + 1} bins, OBW at "
        f"0.99, 26 dB width, a relative limit line over {int(np.count_nonzero(~np.isnan(line)))} bins: {fig}",
        f"        median ACPR {', '.join(f'{a:.1f}' for a in acpr[1:])} dB, median occupied bandwidth {width / 1e6:.3f} MHz, "
        f"{int(np.count_nonzero(r.mask_failed))} rows above the line"])


def step_parts(args):
    from topdogspectrumanalyser_amd import DeviceBuffer
    plan, _ = _plan_and_line()
    with DeviceBuffer.of(capture()) as d_rows:
        _, one = _measure(args, d_rows, plan[:1], fraction=0.99, xdb=26.0)
        _, wide = _measure(args, d_rows, [(0, N_BINS - 1)] * 16, fraction=0.99, xdb=26.0)
    return dict(text=[f"parts: one channel, no limit line: {one}",
                      f"parts: sixteen channels of the whole row, no limit line: {wide}"])


def step_scale(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, SignalDetector, SpectrumEngine, analytics as an
    with DeviceBuffer.of(capture()) as d_rows:
        with SignalDetector(N_BINS, max_host_rows=1, margin_db=10.0, max_gap=2, min_width=3, max_signals=16) as d:
            dt = median_us(d, lambda: d.process_device(None, d_rows.ptr, N_ROWS), args.warm, args.reps)
        with SpectrumEngine(64) as eng:
            st = median_us(eng, lambda: an.rows_stats(eng, d_rows.ptr, N_ROWS, N_BINS, FREQ, (95e6, 105e6)), args.warm, args.reps)
    fl = floor_us(args.copy_bps)
    return dict(text=[
        f"scale: on the rows of `second`, tdsa_detect (median floor, 10 dB margin, 16 records) {dt[0]:9.1f} us (min {dt[1]:.1f}, max "
        f"{dt[2]:.1f}); tdsa_rows_stats (peak, argmax, a band of half the row) {st[0]:9.1f} us (min {st[1]:.1f}, max {st[2]:.1f}); "
        f"the same memory floor, {fl:7.1f} us"])


def header(args):
    return (f"channel measurements (tdsa_meas_*): every device figure is the median of {args.reps} single calls after warm-up "
            f"calls, between device events on the handle's stream, records read back included")


STEPS = dict(copy=step_copy, second=step_second, parts=step_parts, scale=step_scale)

if __name__ == "__main__":
    main(__file__, STEPS, header)
