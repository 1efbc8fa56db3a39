#!/usr/bin/env python3
"""3-D history views of a capture without pulling its rows to the host.

    python examples/history_capture.py

An int8 IQ capture shaped like the C3 workload (N = 16384, 50 % overlap) becomes dB rows on the GPU; the rows go
straight from the engine's device buffer into two trace histories (`push_rows`, on the engine's stream), and what comes
back is what the ribbon and the line-stack displays draw, reduced to 1024 screen columns: 30 ribbon meshes and a
300-line stack, 2.6 MB instead of the 19.7 MB of rows a host-side history of 300 lines would have to hold.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import SpectrumEngine, TraceHistory  # noqa: E402
from topdogspectrumanalyser_amd.utils.synthetic import synth_iq_int8  # noqa: E402

FS, FC, NFFT, HOP = 20e6, 2.45e9, 16384, 8192
SAMPLES = 4_000_000
COLUMNS = 1024


def main():
    frames = (SAMPLES - NFFT) // HOP + 1
    freq = np.fft.fftshift(np.fft.fftfreq(NFFT, 1 / FS)) + FC
    window = np.hanning(NFFT).astype(np.float32)
    window /= np.sqrt(np.mean(window ** 2))
    x = (-10.0 + (freq.astype(np.float32) - float(freq[0])) / (float(freq[-1]) - float(freq[0])) * 20.0)   # the ribbon's x
    iq = synth_iq_int8(SAMPLES, NFFT, seed=21)
    with SpectrumEngine(NFFT, max_frames=frames) as eng, TraceHistory(30, NFFT) as ribbon, \
            TraceHistory(300, NFFT) as stack:
        eng.set_window(window)
        eng.configure(db_mode="mag", log_floor=1e-12, dc_alpha=1.0)
        for h in (ribbon, stack):
            h.set_amplitude(0.0, 120.0)
        t0 = time.perf_counter()
        with eng.pipe(SAMPLES, n_slots=1, rows="device") as pipe:
            pipe.acquire()[: iq.size] = iq
            pipe.submit(SAMPLES, HOP, frames)
            rows_dev, nf = pipe.collect_device()             # the rows stay on the GPU
            ribbon.push_rows(eng, rows_dev, nf)
            stack.push_rows(eng, rows_dev, nf)
            r = ribbon.ribbon(x, columns=COLUMNS)
            s = stack.lines(columns=COLUMNS)
        dt = time.perf_counter() - t0
    back = sum(a.nbytes for a in (r["verts"], r["colours"], r["bins"], s["z"], s["index"], s["bins"], s["hold"]))
    li, lz = s["live_peak"]
    print(f"{nf} frames of {NFFT} bins in {dt * 1e3:.1f} ms; {back / 1e6:.2f} MB came back "
          f"({nf * NFFT * 4 / 1e6:.1f} MB of rows stayed on the device)")
    print(f"ribbon: verts {r['verts'].shape}, colours {r['colours'].shape}, faces {TraceHistory.ribbon_faces(COLUMNS).shape}")
    print(f"line stack: z {s['z'].shape}, colour index {s['index'].shape} into a palette {TraceHistory.line_palette().shape}; "
          f"live peak z = {lz:.2f} at {freq[li] / 1e6:.3f} MHz, hold peak z = {s['hold_peak'][1]:.2f} at "
          f"{freq[s['hold_peak'][0]] / 1e6:.3f} MHz")


if __name__ == "__main__":
    main()
