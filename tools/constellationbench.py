#!/usr/bin/env python3
"""Timing of the device constellation analysis.

  per tick   wall time of Constellation.process on 16 384 complex64 samples from the host (density mode: rms, EVM,
             128 x 128 histogram read back), per modulation; median of 300 calls after 30 warm-up calls
  capture    a C3-sized int8 capture resident in HBM (20 M samples as 1220 ticks of 16 384): process_segments with
             per-segment histograms in HBM; samples/s and the fraction of the HBM floor (the input is read twice:
             4 B per int8 sample at 8 TB/s)
  histogram  the same capture with every sample in one bin (hot) against samples spread over the plane (spread)

    python tools/constellationbench.py [--out profiles/constellationbench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import Constellation, DeviceBuffer, _native as nat  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak, as bench.py
MODS = ("bpsk", "qpsk", "8psk", "16qam", "64qam", "ofdm")


def median_call(f, warm=30, reps=300):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    with Constellation(max_host_samples=1 << 17) as c:
        say("per tick: 16384 complex64 samples from the host, density mode (rms, EVM, 128x128 counts read back)")
        tick = ((rng.standard_normal(16384) + 1j * rng.standard_normal(16384)) * 0.1 +
                rng.choice([-0.3, 0.3], 16384) + 1j * rng.choice([-0.3, 0.3], 16384)).astype(np.complex64)
        for mod in MODS:
            c.set_modulation(mod)
            med, p90 = median_call(lambda: c.process(tick))
            say(f"  {mod:6s} median {med * 1e6:7.1f} us   p90 {p90 * 1e6:7.1f} us")

        seg, n_seg = 16384, 1220
        ns = seg * n_seg
        cases = {
            "spread": rng.integers(-128, 128, 2 * ns).astype(np.int8),
            "qpsk-like": np.clip(np.round(rng.standard_normal(2 * ns) * 6 + 40 * rng.choice([-1, 1], 2 * ns)), -128,
                                 127).astype(np.int8),
            "hot": np.tile(np.array([40, -40], np.int8), ns),
        }
        d_in = DeviceBuffer(2 * ns)
        d_cnt = DeviceBuffer(n_seg * 128 * 128 * 4)
        try:
            say(f"capture: {ns} int8 samples in HBM as {n_seg} segments of {seg}; floor = 4 B/sample at "
                f"{HBM_PEAK_GBS:.0f} GB/s = {4 * ns / (HBM_PEAK_GBS * 1e9) * 1e6:.1f} us")
            for name, raw in cases.items():
                d_in.put(raw)
                for mod in ("qpsk", "64qam", "8psk"):
                    c.set_modulation(mod)
                    for hist in (True, False):
                        cnt = d_cnt.ptr if hist else None
                        med, _ = median_call(lambda: c.process_segments(None, d_in.ptr, nat.IN_I8, seg, seg, n_seg,
                                                                         cnt), warm=3, reps=15)
                        rate = ns / med
                        frac = 4 * ns / med / (HBM_PEAK_GBS * 1e9)
                        say(f"  {name:9s} {mod:6s} hist={'on ' if hist else 'off'} {med * 1e3:7.3f} ms  "
                            f"{rate / 1e9:6.2f} G samples/s  {frac * 100:5.1f} % of the HBM floor")
        finally:
            d_in.close()
            d_cnt.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
