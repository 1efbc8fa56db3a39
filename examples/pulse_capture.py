#!/usr/bin/env python3
"""Pulse descriptors of a radar-like train, without the samples leaving the device.

    python examples/pulse_capture.py

One synthetic second at 20 Msps (int8 IQ, made and uploaded in chunks): noise and a pulsed carrier 3.0 MHz above the
centre, 40 us on every 500 us, with a small offset of 12.5 kHz from the nominal carrier.  A DownConverter tunes onto
the nominal carrier and decimates by 8 on an engine's stream; a PulseAnalyzer behind it, on the same stream, keeps one
record per pulse in HBM - the chunks cut pulses wherever they like, an open pulse waits in the handle for the next
chunk.  read() brings the records back; printed: the number of pulses, PRI and PRF, width, duty cycle, the power in
the pulse and the carrier inside it, which is the offset the nominal tuning left.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (DeviceBuffer, DownConverter, PulseAnalyzer, SpectrumEngine, levels_from_db,  # noqa: E402
                                        _native as nat)

FS, SECOND, CHUNK = 20e6, 20_000_000, 2_000_000 + 1234                # a chunk length that is no multiple of anything
CARRIER, OFFSET, D = 3.0e6, 12.5e3, 8
PRI_S, WIDTH_S = 500e-6, 40e-6


def chunk_of(start, n, rng):
    """Samples start .. start + n - 1 of the second, interleaved int8."""
    t = (np.arange(n, dtype=np.float64) + start) / FS
    gate = np.mod(t, PRI_S) < WIDTH_S
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.6 * gate * np.exp(2j * np.pi * (CARRIER + OFFSET) * t)
    iq = np.empty(2 * n, dtype=np.int8)
    iq[0::2] = np.clip(np.round(x.real * 127.0), -128, 127)
    iq[1::2] = np.clip(np.round(x.imag * 127.0), -128, 127)
    return iq


def main():
    rng = np.random.default_rng(5)
    fs_out = FS / D
    on, off = levels_from_db(-12.0, 6.0)                              # the carrier's power is about -4.5 dB; the noise far below
    with SpectrumEngine(64) as eng, DownConverter(D, FS, CARRIER) as ddc, PulseAnalyzer(1, 4096) as pa, \
            DeviceBuffer(2 * CHUNK) as d_iq, DeviceBuffer(8 * (CHUNK // D + 2)) as d_bb:
        pa.configure(on, off, min_width=4)
        start = 0
        while start < SECOND:
            n = min(CHUNK, SECOND - start)
            iq = chunk_of(start, n, rng)
            pa.read_summaries()                                       # the previous chunk has left both buffers
            d_iq.put(iq)
            n_out = ddc.process_device(eng, nat.IN_I8, d_iq.ptr, n, d_bb.ptr)
            pa.process_device(eng, d_bb.ptr, n_out)                   # behind the down-converter, on the engine's stream
            start += n
        t = pa.read(0)
    toa_s, width_s = t.to_seconds(fs_out)
    print(f"one second at {FS / 1e6:g} Msps, tuned to {CARRIER / 1e6:g} MHz, decimated by {D} to {fs_out / 1e6:g} Msps: "
          f"on at {10 * np.log10(on):.1f} dB, off at {10 * np.log10(off):.1f} dB")
    print(f"  {t.n_pulses} pulses ({len(t)} stored, {t.n_lost} lost, {t.n_short} shorter than 4 samples dropped), "
          f"open at the end: {t.open_pulse}")
    print(f"  PRI    median {np.median(t.pri()) / fs_out * 1e6:8.2f} us   (made: {PRI_S * 1e6:g} us), PRF {np.median(t.prf(fs_out)):.1f} Hz")
    print(f"  width  median {np.median(width_s) * 1e6:8.2f} us   (made: {WIDTH_S * 1e6:g} us), first pulse at {toa_s[0] * 1e6:.2f} us")
    print(f"  duty   {100 * t.duty_cycle:8.3f} %        (made: {100 * WIDTH_S / PRI_S:g} %)")
    print(f"  power  median {10 * np.log10(np.median(t.mean_power)):8.2f} dB mean, {10 * np.log10(np.median(t.peak_power)):.2f} dB peak")
    print(f"  carrier inside the pulses: median {np.median(t.freq) * fs_out / 1e3:+8.3f} kHz from the tuning "
          f"(made: {OFFSET / 1e3:+g} kHz), spread {np.std(t.freq) * fs_out:.1f} Hz")


if __name__ == "__main__":
    main()
