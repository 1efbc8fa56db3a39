#!/usr/bin/env python3
"""Which emissions a second of a band holds, without the rows leaving the device.

    python examples/detect_capture.py

One synthetic second at 20 Msps (int8 IQ): noise, two steady carriers with some width, a narrow one that is on for a
third of the time and a wide burst.  SpectrumEngine turns it into 2440 rows of 16384 bins (50 % overlap) that stay in
HBM; SignalDetector reads them in place, on the engine's stream, and returns a few records per row.  Printed: the
emissions of the last row, and the ten bins that were occupied most often with the share of the rows they were in.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import DeviceBuffer, SignalDetector, SpectrumEngine, _native as nat  # noqa: E402

FS, CENTRE, NFFT, HOP = 20e6, 100e6, 16384, 8192
FRAMES, CHUNK = 2440, 244                                            # ten calls of 244 frames


def chunk_iq(c, rng):
    """Frames [c CHUNK, (c + 1) CHUNK) of the second: (HOP (CHUNK - 1) + NFFT) samples as interleaved int8."""
    n = HOP * (CHUNK - 1) + NFFT
    t = (np.arange(n, dtype=np.float64) + c * CHUNK * HOP) / FS
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f0, dev, amp in ((-6.2e6, 40e3, 0.25), (2.5e6, 90e3, 0.12)):  # steady, frequency modulated: some bandwidth
        x += amp * np.exp(2j * np.pi * (f0 * t + dev / 2e3 * np.sin(2 * np.pi * 1e3 * t)))
    if c % 3 == 0:
        x += 0.08 * np.exp(2j * np.pi * 7.75e6 * t)                 # on for a third of the time
    if c == 9:
        x += 0.1 * np.exp(2j * np.pi * (-1.0e6 * t + 150e3 / 1e3 * np.sin(2 * np.pi * 1e3 * t)))   # a burst at the end
    iq = np.empty(2 * n, dtype=np.int8)
    iq[0::2] = np.clip(np.round(x.real * 127), -128, 127)
    iq[1::2] = np.clip(np.round(x.imag * 127), -128, 127)
    return iq


def main():
    rng = np.random.default_rng(1)
    freq = CENTRE + np.fft.fftshift(np.fft.fftfreq(NFFT, 1 / FS))
    with SpectrumEngine(NFFT, max_frames=CHUNK) as eng, \
            SignalDetector(NFFT, margin_db=12.0, max_gap=4, min_width=3, max_signals=8, bins=(8, NFFT - 9)) as det:
        eng.set_window(np.hanning(NFFT).astype(np.float32))
        eng.configure(db_mode="mag", log_floor=1e-12)
        with DeviceBuffer(4 * FRAMES * NFFT) as d_rows, DeviceBuffer(2 * (HOP * (CHUNK - 1) + NFFT)) as d_iq:
            for c in range(FRAMES // CHUNK):
                iq = chunk_iq(c, rng)
                eng.synchronize()                                     # the previous chunk has left d_iq
                d_iq.put(iq)
                eng.process_device(nat.IN_I8, d_iq.ptr, iq.size // 2, HOP, CHUNK,
                                   d_rows.at(4 * c * CHUNK * NFFT, 4 * CHUNK * NFFT))
            r = det.process_device(eng, d_rows.ptr, FRAMES)           # behind the last chunk, on the same stream
            counts, seen, flagged = det.occupancy()
    print(f"{FRAMES} rows of {NFFT} bins ({FS / 1e6:g} Msps around {CENTRE / 1e6:g} MHz): median noise floor "
          f"{np.median(r.floor):.1f} dB, {seen} rows seen, {flagged} flagged")
    print(f"last row: floor {r.floor[-1]:.1f} dB, threshold {r.thr[-1]:.1f} dB, {r.n_found[-1]} emissions")
    print("  centre MHz   width kHz   3 dB kHz   power dB   peak dB")
    for e in r.to_hz(freq, -1):
        print(f"{e['centre_hz'] / 1e6:12.4f} {e['bandwidth_hz'] / 1e3:11.1f} {e['xdb_bandwidth_hz'] / 1e3:10.1f} "
              f"{e['power_db']:10.1f} {e['peak_db']:9.1f}")
    print("most occupied bins:")
    for b in np.argsort(-counts.astype(np.int64), kind="stable")[:10]:
        print(f"  {freq[b] / 1e6:10.4f} MHz   {100.0 * counts[b] / max(seen - flagged, 1):5.1f}% of the rows")


if __name__ == "__main__":
    main()
