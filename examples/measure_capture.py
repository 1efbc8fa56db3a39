#!/usr/bin/env python3
"""Channel power, ACPR, occupied bandwidth and a mask verdict for every row of a second, without the rows leaving the
device.

    python examples/measure_capture.py

One synthetic second at 20 Msps (int8 IQ): noise, a wide frequency-modulated carrier and a weak neighbour one channel
up.  SpectrumEngine turns it into 2440 rows of 16384 bins (50 % overlap) that stay in HBM.  SignalDetector reads the
first rows and finds the strongest emission; its centre and width become the channel plan - the main channel and two
adjacent channels on either side - and an emission mask relative to the main channel's peak.  ChannelMeasure then reads
all rows in place, on the engine's stream, and returns 80 + 5 x 24 bytes per row.  Printed: the plan, the median channel
powers and ACPR, the occupied bandwidth and 26 dB width, and how many rows broke the mask and where the worst bin lay.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (ChannelMeasure, DeviceBuffer, SignalDetector, SpectrumEngine,  # noqa: E402
                                        channels_from_emission, limit_line, _native as nat)

FS, CENTRE, NFFT, HOP = 20e6, 100e6, 16384, 8192
FRAMES, CHUNK = 2440, 244                                            # ten calls of 244 frames


def chunk_iq(c, rng):
    """Frames [c CHUNK, (c + 1) CHUNK) of the second: (HOP (CHUNK - 1) + NFFT) samples as interleaved int8."""
    n = HOP * (CHUNK - 1) + NFFT
    t = (np.arange(n, dtype=np.float64) + c * CHUNK * HOP) / FS
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += 0.3 * np.exp(1j * (2 * np.pi * 2.5e6 * t + 150e3 / 2e3 * np.sin(2 * np.pi * 2e3 * t)))   # FM, 150 kHz deviation
    x += 0.003 * np.exp(2j * np.pi * (2.5e6 + 0.5e6) * t)            # a weak neighbour: in the first upper channel
    if c >= 8:
        x += 0.05 * np.exp(2j * np.pi * (2.5e6 - 1.0e6) * t)         # a spur two channels down, in the last fifth
    iq = np.empty(2 * n, dtype=np.int8)
    iq[0::2] = np.clip(np.round(x.real * 127), -128, 127)
    iq[1::2] = np.clip(np.round(x.imag * 127), -128, 127)
    return iq


def main():
    rng = np.random.default_rng(1)
    freq = CENTRE + np.fft.fftshift(np.fft.fftfreq(NFFT, 1 / FS))
    bin_width = FS / NFFT
    with SpectrumEngine(NFFT, max_frames=CHUNK) as eng, \
            SignalDetector(NFFT, margin_db=15.0, max_gap=8, min_width=8, max_signals=8, bins=(8, NFFT - 9)) as det:
        eng.set_window(np.hanning(NFFT).astype(np.float32))
        eng.configure(db_mode="mag", log_floor=1e-12)
        with DeviceBuffer(4 * FRAMES * NFFT) as d_rows, DeviceBuffer(2 * (HOP * (CHUNK - 1) + NFFT)) as d_iq:
            for c in range(FRAMES // CHUNK):
                iq = chunk_iq(c, rng)
                eng.synchronize()                                     # the previous chunk has left d_iq
                d_iq.put(iq)
                eng.process_device(nat.IN_I8, d_iq.ptr, iq.size // 2, HOP, CHUNK,
                                   d_rows.at(4 * c * CHUNK * NFFT, 4 * CHUNK * NFFT))
            found = det.process_device(eng, d_rows.ptr, 16).to_hz(freq, -1)   # the plan comes from the detector's records
            em = found[np.argmax(found["power_db"])]
            spacing = 0.5e6
            plan = channels_from_emission(em, freq, spacing_hz=spacing, n_adjacent=2, bandwidth_hz=0.4e6)
            mask = limit_line(freq, [(-2e6, -20.0), (-0.3e6, -10.0), (-0.2e6, 3.0), (0.2e6, 3.0), (0.3e6, -10.0), (2e6, -20.0)],
                              centre_hz=float(em["centre_hz"]))
            span = (plan[1][0], plan[2][1])                            # OBW and 26 dB width: over the main and first adjacent channels
            with ChannelMeasure(NFFT, plan, obw=span, fraction=0.99, xdb=26.0, limit=mask, limit_relative=True) as meas:
                r = meas.process_device(eng, d_rows.ptr, FRAMES)      # behind the last chunk, on the same stream
                seen, failed = meas.totals()
    print(f"{FRAMES} rows of {NFFT} bins ({FS / 1e6:g} Msps around {CENTRE / 1e6:g} MHz); the detector's strongest emission: "
          f"{em['centre_hz'] / 1e6:.4f} MHz, {em['bandwidth_hz'] / 1e3:.1f} kHz wide, {em['power_db']:.1f} dB")
    names = ["main", "lower 1", "upper 1", "lower 2", "upper 2"]
    power, acpr = np.median(r.channel_power_db(bin_width), axis=0), np.median(r.acpr_db(), axis=0)
    print("  channel        bins        MHz   power dB   ACPR dB")
    for name, (lo, hi), p, a in zip(names, plan, power, acpr):
        print(f"  {name:8s} {lo:6d}..{hi:<6d} {0.5 * (freq[lo] + freq[hi]) / 1e6:9.4f} {p:10.1f} {a:9.1f}")
    width, centre = zip(*(r.obw_hz(freq, k) for k in range(len(r))))
    x26 = np.array([r.xdb_hz(freq, k)[0] for k in range(len(r))])
    print(f"occupied bandwidth (99 %): median {np.median(width) / 1e3:.1f} kHz around {np.median(centre) / 1e6:.4f} MHz; "
          f"26 dB width: median {np.median(x26) / 1e3:.1f} kHz")
    print(f"mask: {failed} of {seen} rows above the line; the first at row {int(np.argmax(r.mask_failed)) if failed else -1}")
    if failed:
        k = int(np.argmax(np.where(r.mask_failed, r.worst_margin, -np.inf)))
        print(f"  worst: row {k}, {r.worst_margin[k]:.1f} dB over at {freq[r.worst_bin[k]] / 1e6:.4f} MHz "
              f"({int(r.n_fail[k])} bins, {freq[r.first_fail[k]] / 1e6:.4f} .. {freq[r.last_fail[k]] / 1e6:.4f} MHz)")


if __name__ == "__main__":
    main()
