#!/usr/bin/env python3
"""Timing of the signal detection.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  second   a C3-shaped second: 2440 rows of 16384 bins in HBM, noise with emissions over about 3 % of the bins,
           SignalDetector.process_device (median floor, 10 dB margin, max_gap 2, min_width 3, 16 records per row), next
           to its memory floor: 4 bytes read per bin at the copy rate
  worst    the same shape with every other bin above the threshold: 8192 runs per row, 64 records per row
  scale    tdsa_rows_marker_peaks and tdsa_rows_stats on the rows of `second`, for scale (their code is not touched by
           the detector), between events on the plan's stream

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  Per device figure:
warm-up calls, then the median of `--reps` (at least 20) single calls, each between device events on the handle's
stream; a call ends when the records are in host memory, so the figure includes that copy and wait.  No time is fixed in
advance: each figure stands next to its memory floor.

    python tools/detectbench.py [--out profiles/detectbench.txt] [--reps 20]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_ROWS, N_BINS = 2440, 16384
STEPS = ["copy", "second", "worst", "scale"]
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


def run_step(args):
    return dict(copy=step_copy, second=step_second, worst=step_worst, scale=step_scale)[args.step](args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--copy-bps", dest="copy_bps", type=float, default=0.0)
    args = ap.parse_args()
    args.reps = max(args.reps, 20)
    if args.step:
        print("RESULT " + json.dumps(run_step(args)), flush=True)
        return
    lines = [f"signal detection (tdsa_detect_*): every device figure is the median of {args.reps} single calls after warm-up "
             f"calls, between device events on the handle's stream, records read back included"]
    print(lines[0], flush=True)
    copy_bps = 0.0
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warm", str(args.warm),
               "--copy-bps", repr(copy_bps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"{step}: no result within {LIMIT_S} s; stopping")
            print(lines[-1], flush=True)
            break
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            lines.append(f"{step}: exit status {r.returncode}; stopping\n{r.stderr[-1500:]}")
            print(lines[-1], flush=True)
            break
        res = json.loads(res[-1][7:])
        copy_bps = res.get("copy_bps", copy_bps)
        for ln in res["text"]:
            print(ln, flush=True)
            lines.append(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
