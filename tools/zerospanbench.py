#!/usr/bin/env python3
"""Timing of zero span at 20 Msps: a two-second detector ring of 40 M float32 in HBM.

  push   one C3 second (20e6 samples already in HBM, one call) into the ring, int8 and complex64 input, per detector;
         device events on the handle's stream around `reps` calls after warm-up.  Floor: the bytes of the shapes
         (2 or 8 in, 4 out per sample) at the measured 6.29 TB/s.
  view   trigger search (rise) plus trace over a full ring at windows of 10 ms, 100 ms and 1 s, as 2048 MINMAX
         columns and as the raw chunk; device events around `reps` views (they include the read-back), and the host
         wall time of one view.  Next to each: the bytes it must read (4 per searched pair, 4 per shown sample).
  tick   one GUI tick - a host block of 400 000 complex64 samples pushed, a 10 ms rise-triggered raw view - as host
         wall time ending in the view's synchronise, against DataProcessor._process_zero_span_data's host path on the
         same blocks with the two-second history full; the two alternate in one process.

    python tools/zerospanbench.py [--out profiles/zerospanbench.txt] [--reps 10] [--pairs 12]
"""
import argparse
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import DataProcessor, DeviceBuffer, ZeroSpan, _native as nat  # noqa: E402

FS = 20e6
N_IN = 20_000_000
TICK = 400_000
HBM_BPS = 6.29e12


def timed(zs, f, warm, reps):
    for _ in range(warm):
        f()
    zs.timer_begin()
    for _ in range(reps):
        f()
    return zs.timer_end() * 1e3 / reps


def pulse_train(rng, n, t0=0):
    """int8 IQ: a 1 kHz pulse train of 30 % duty under noise (I), noise (Q)."""
    k = np.arange(t0, t0 + n)
    i = np.where((k % 20_000) < 6_000, 70, -30) + rng.integers(-6, 7, n)
    q = rng.integers(-6, 7, n)
    return np.stack([i, q], axis=1).astype(np.int8).reshape(-1)


def to_c64(raw):
    v = raw.reshape(-1, 2).astype(np.float32) / np.float32(128.0)
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def spread(x):
    x = np.asarray(x)
    return f"median {np.median(x):9.3f} ms, min {x.min():9.3f}, max {x.max():9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=12)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    raw = pulse_train(rng, 2 * N_IN)                       # two seconds: fills the ring
    d_i8, d_c64 = DeviceBuffer(raw.nbytes // 2), DeviceBuffer(8 * N_IN)
    try:
        d_i8.put(raw[:raw.size // 2])
        cplx = to_c64(raw[:2 * N_IN])
        d_c64.put(cplx)
        del cplx
        say(f"zero span at {FS / 1e6:.0f} Msps: ring of {int(2 * FS)} float32 in HBM; device events around {args.reps} "
            f"calls after {args.warm} warm-up calls; memory floors at {HBM_BPS / 1e12:.2f} TB/s")
        say("")
        say(f"push of one C3 second ({N_IN} samples in HBM, one call)")
        say(f"{'input':>5s} {'detector':>8s} {'us':>9s} {'floor us':>9s} {'% of floor':>10s} {'GB/s':>8s}")
        for det in ("real", "mag", "db"):
            with ZeroSpan(FS, detector=det) as zs:
                for name, fmt, ptr, bps in (("i8", nat.IN_I8, d_i8, 2), ("c64", nat.IN_C64, d_c64, 8)):
                    us = timed(zs, lambda: zs.push_device(None, fmt, ptr.ptr, N_IN), args.warm, args.reps)
                    nbytes = N_IN * (bps + 4)
                    floor = nbytes / HBM_BPS * 1e6
                    say(f"{name:>5s} {det:>8s} {us:9.1f} {floor:9.1f} {100 * floor / us:9.1f}% {nbytes / us / 1e3:8.0f}")
        say("")
        say("view over a full ring: rise trigger at 0.15, then the trace (device events include the read-back)")
        say(f"{'window':>7s} {'output':>12s} {'device us':>10s} {'wall us':>9s} {'searched':>10s} {'shown':>9s} "
            f"{'MB read':>8s} {'floor us':>9s} {'to host B':>10s} {'triggered':>9s}")
        with ZeroSpan(FS) as zs:
            zs.push_device(None, nat.IN_I8, d_i8.ptr, N_IN)
            zs.push(raw[2 * N_IN:])
            for window in (0.01, 0.1, 1.0):
                nd = int(window * FS)
                plan_se = zs.capacity - nd
                pairs = max(0, plan_se - 1 - max(0, plan_se - 8 * nd))
                for what, points in (("2048 minmax", 2048), ("raw chunk", None)):
                    f = lambda: zs.view(mode="rise", level=0.15, window_s=window, points=points)   # noqa: E731
                    us = timed(zs, f, args.warm, args.reps)
                    walls = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        v = f()
                        walls.append((time.perf_counter() - t0) * 1e6)
                    nbytes = 4 * (pairs + nd)
                    back = 16432 + (4 * nd if points is None else 8 * points)
                    say(f"{window:7.2f} {what:>12s} {us:10.1f} {np.median(walls):9.1f} {pairs:10d} {nd:9d} "
                        f"{nbytes / 1e6:8.1f} {nbytes / HBM_BPS * 1e6:9.1f} {back:10d} {int(v.triggered):9d}")
        say("")
        # ---- one GUI tick, device ring against the host history ------------------------------------------------
        blocks = [to_c64(raw[2 * a:2 * (a + TICK)]) for a in range(0, 2 * N_IN, TICK)]

        class Widget:
            def update_zero_span_data(self, t, y):
                self.t, self.y = t, y

        def gui(**kw):
            src = types.SimpleNamespace(sample_rate=FS, block=None)
            src.read_samples_only = lambda: src.block
            mw = types.SimpleNamespace(current_source=src, zero_span_widget=Widget())
            dm = types.SimpleNamespace(zero_span_buffer=None, zero_span_time_window=0.01, zero_span_trigger_mode="rise",
                                       zero_span_trigger_level=0.15)
            return src, mw, DataProcessor(mw, dm, **kw)

        src_d, mw_d, on_dev = gui(zero_span_on_device=True)
        src_h, mw_h, on_host = gui()
        for b in blocks:                                   # two seconds: both histories are full
            src_d.block = src_h.block = b
            on_dev._process_zero_span_data()
            on_host._process_zero_span_data()
        t_dev, t_host = [], []
        for k in range(args.pairs):
            b = blocks[k % len(blocks)]
            src_d.block = src_h.block = b
            t0 = time.perf_counter()
            on_dev._process_zero_span_data()
            t1 = time.perf_counter()
            on_host._process_zero_span_data()
            t2 = time.perf_counter()
            t_dev.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
            assert np.array_equal(mw_d.zero_span_widget.y, mw_h.zero_span_widget.y)
        nd = int(0.01 * FS)
        say(f"one GUI tick: {TICK} complex64 samples in, rise-triggered 10 ms view ({nd} points) out, history full; "
            f"{args.pairs} alternating pairs, host wall time; the two paths gave the same chunk every time")
        say(f"  device ring : {spread(t_dev)}; {8 * TICK} bytes to the device, {16432 + 4 * nd} bytes to the host")
        say(f"  host history: {spread(t_host)}; nothing crosses PCIe; {4 * int(2 * FS)} bytes of history rebuilt per tick")
        say(f"  ratio of the medians: {np.median(t_host) / np.median(t_dev):.1f} x")
    finally:
        for p in (d_i8, d_c64):
            p.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
