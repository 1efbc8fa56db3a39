#!/usr/bin/env python3
"""Timing of the 3-D history views at n = 16384 bins, rows resident in HBM.

  copy     the box's device-to-device copy rate (1 GiB, torch), which the view passes are stated against
  push     256 dB rows already in HBM into the ring in one call, per row
  ribbon   30 rows -> vertices and colours; lines: 300 lines -> z and colour index / RGBA; surface: 100 rows -> z and
           colours.  Each at full width and at columns=1024, into device memory (the pass alone) and into host
           memory (with the read-back), with the bytes each moves and the bytes that cross to the host
  host     the numpy restatement of the same tick (tests/history_contract.py) on the host's CPU, for scale

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per step: warm-up calls, then the median of `--reps` (at least 20) single
calls, each between device events on the handle's stream.

    python tools/historybench.py [--out profiles/historybench.txt] [--reps 20] [--steps copy,ribbon]
"""
import functools
import os
import sys
import time

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 16384
PUSH_ROWS = 256
LIMIT_S = {"copy": 120, "push": 120, "ribbon": 180, "lines": 240, "surface": 180, "host": 300}


def rows_db(rng, n_rows):
    return rng.normal(-80.0, 12.0, size=(n_rows, N)).astype(np.float32)


def fill(h, rng, n_rows):
    from topdogspectrumanalyser_amd import DeviceBuffer
    with DeviceBuffer.of(rows_db(rng, n_rows)) as d:
        h.push_rows(None, d.ptr, n_rows)
        h.lines(0, 1) if h.kind == "heights" else h.surface(columns=1)


def step_push(args):
    from topdogspectrumanalyser_amd import DeviceBuffer, TraceHistory
    rng = np.random.default_rng(1)
    rows = rows_db(rng, PUSH_ROWS)
    d = DeviceBuffer(rows.nbytes)
    d.put(rows)
    text = []
    for kind, depth in (("heights", 300), ("levels", 100)):
        with TraceHistory(depth, N, kind) as h:
            us, lo, hi = median_us(h, lambda: h.push_rows(None, d.ptr, PUSH_ROWS), args.warm, args.reps)
            one = median_us(h, lambda: h.push_rows(None, d.ptr, 1), args.warm, args.reps)[0]
            moved = PUSH_ROWS * N * 8
            text.append(f"push {kind:8s}: {PUSH_ROWS} rows in one call {us:9.1f} us (min {lo:.1f}, max {hi:.1f}) = "
                        f"{us / PUSH_ROWS:7.3f} us per row, {moved / us / 1e6:7.3f} TB/s = "
                        f"{100 * moved / us * 1e6 / args.copy_bps:5.1f}% of the copy rate; one row per call {one:7.1f} us")
    d.close()
    return dict(text=text)


def view_step(args, name):
    from topdogspectrumanalyser_amd import DeviceBuffer, TraceHistory
    rng = np.random.default_rng(2)
    x = np.linspace(-10, 10, N, dtype=np.float32)
    kind, depth = ("levels", 100) if name == "surface" else ("heights", 30 if name == "ribbon" else 300)
    text = []
    with TraceHistory(depth, N, kind) as h:
        fill(h, rng, depth + 5)
        variants = [("index",), ("rgba",)] if name == "lines" else [()]
        for var in variants:
            for cols in (None, 1024):
                n = cols or N
                R = min(depth, 30) if name == "ribbon" else depth
                per = {"ribbon": (24, 32), "surface": (4, 12), "lines": (4, 16 if var == ("rgba",) else 1)}[name]
                out_bytes = R * n * (per[0] + per[1])
                read_bytes = R * N * 4 + (R * n * 12 if cols else 0)       # the rows; reduced: values + bins written, values read
                d0, d1 = DeviceBuffer(R * n * per[0]), DeviceBuffer(R * n * per[1])
                dest = dict(primary=d0.ptr, colours=d1.ptr)
                if name == "ribbon":
                    on_dev, on_host = (lambda: h.ribbon(x, cols, device_out=dest)), (lambda: h.ribbon(x, cols))
                elif name == "lines":
                    on_dev = lambda: h.lines(0, None, var[0], cols, device_out=dest)      # noqa: E731
                    on_host = lambda: h.lines(0, None, var[0], cols)                      # noqa: E731
                else:
                    on_dev, on_host = (lambda: h.surface(cols, device_out=dest)), (lambda: h.surface(cols))
                us_d = median_us(h, on_dev, args.warm, args.reps)
                us_h = median_us(h, on_host, args.warm, args.reps)
                walls = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    on_host()
                    walls.append((time.perf_counter() - t0) * 1e6)
                moved = out_bytes + read_bytes
                d2h = out_bytes + (R * n * 4 if cols else 0) + (2 * n * 4 if name == "lines" else 0)
                text.append(f"{name:7s} {'/'.join(var) or '-':5s} columns={str(cols):5s}: device destination {us_d[0]:9.1f} us "
                            f"(min {us_d[1]:.1f}, max {us_d[2]:.1f}), {moved / 1e6:8.2f} MB moved = {moved / us_d[0] / 1e6:6.3f} TB/s = "
                            f"{100 * moved / us_d[0] * 1e6 / args.copy_bps:5.1f}% of the copy rate; host destination "
                            f"{us_h[0]:9.1f} us on the stream, {np.median(walls):9.1f} us wall, {d2h / 1e6:8.2f} MB to the host")
                d0.close()
                d1.close()
    return dict(text=text)


def step_host(args):
    import history_contract as hc
    rng = np.random.default_rng(3)
    x = np.linspace(-10, 10, N, dtype=np.float32)
    text = []
    for name, depth, kind in (("ribbon", 30, "heights"), ("lines", 300, "heights"), ("surface", 100, "levels")):
        m = hc.HistoryModel(depth, N, kind)
        rows = rows_db(rng, 8)
        t = []
        for r in rows:
            t0 = time.perf_counter()
            m.push(r)
            v = m.ribbon(x) if name == "ribbon" else m.lines() if name == "lines" else m.surface()
            t.append((time.perf_counter() - t0) * 1e3)
        del v
        text.append(f"host numpy tick {name:7s} (push + full-width view, {depth} rows x {N} bins): median {np.median(t[1:]):8.2f} ms")
    return dict(text=text)


def header(args):
    return (f"3-D history views at n = {N} bins; every figure is the median of {args.reps} single calls after {args.warm} "
            "warm-up calls, between device events on the handle's stream unless it says wall")


STEPS = dict(copy=step_copy, push=step_push,
             **{name: functools.partial(view_step, name=name) for name in ("ribbon", "lines", "surface")}, host=step_host)

if __name__ == "__main__":
    main(__file__, STEPS, header, LIMIT_S)
