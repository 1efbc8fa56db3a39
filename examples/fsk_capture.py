#!/usr/bin/env python3
"""FSK analysis of a GFSK burst, without the samples leaving the device.

    python examples/fsk_capture.py [2 | 4]

A complex64 capture at 16 Msps holds a 1 Msym/s GFSK carrier (BT 0.5, modulation index 0.5 for two levels as in Bluetooth
LE, 0.33 for four), 21 kHz off tune, with noise 30 dB down.  The down-converter (decimation 2) leaves 8 samples per
symbol in HBM; FskAnalyzer finds the symbol clock of every 4096-sample segment and leaves one level and one decision
per symbol next to them.  Per segment the deviation, the carrier offset, the FSK error and a record come back to the
host; the decisions of the first segment are read back to print its first bits.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import DeviceBuffer, DownConverter, FskAnalyzer, SpectrumEngine, _native as nat  # noqa: E402

FS, SYMBOL_RATE, D = 16e6, 1e6, 2
SPS_IN = int(FS / SYMBOL_RATE)
SPS = SPS_IN // D
OFFSET_HZ, SNR_DB, BT = 21e3, 30.0, 0.5
SEG, N_SEG = 4096, 4


def capture(levels, h, n_sym):
    """Random symbols through a Gaussian filter (BT) as a frequency, integrated to a phase."""
    rng = np.random.default_rng(7)
    sent = rng.integers(0, levels, n_sym)
    f = np.repeat(2.0 * sent - (levels - 1), SPS_IN) * (h / 2 / SPS_IN)             # cycles per sample
    sigma = math.sqrt(math.log(2.0)) / (2.0 * math.pi * BT) * SPS_IN
    t = np.arange(-4 * SPS_IN, 4 * SPS_IN + 1)
    gauss = np.exp(-0.5 * (t / sigma) ** 2)
    f = np.convolve(f, gauss / gauss.sum(), mode="same") + OFFSET_HZ / FS
    x = np.exp(2j * np.pi * np.cumsum(f))
    s = 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0)
    x += s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64), sent


def main():
    levels = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    h = 0.5 if levels == 2 else 0.33
    x, sent = capture(levels, h, (SEG * N_SEG * D) // SPS_IN + 64)
    with SpectrumEngine(64) as eng, DownConverter(D, FS) as ddc, FskAnalyzer(SPS, levels) as fsk:
        K = fsk.symbols_per_segment(SEG)
        ny = (x.size + D - 1) // D
        skip = 8 * ddc.first_full_output                             # past the decimator's fill, 8-byte samples
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * ny) as d_y, DeviceBuffer(4 * K * N_SEG) as d_v, \
                DeviceBuffer(K * N_SEG) as d_i:
            ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            r = fsk.process_device(eng, d_y.at(skip, 8 * SEG * N_SEG), SEG, SEG, N_SEG, d_v.ptr, K, d_i.ptr)   # behind it, on the same stream
            r.indices = d_i.get((N_SEG, K), np.uint8)
    fs = FS / D
    print(f"{levels}-GFSK, BT {BT}, h = {h}, {SYMBOL_RATE / 1e6:g} Msym/s at {FS / 1e6:g} Msps, {OFFSET_HZ / 1e3:g} kHz off tune, noise "
          f"{SNR_DB:g} dB down: {N_SEG} segments of {SEG} samples at {SPS} samples per symbol, {K} symbols each")
    print(f"nominal outer deviation {h * (levels - 1) / 2 * SYMBOL_RATE / 1e3:.1f} kHz; the fit averages over the Gaussian filter's "
          f"intersymbol interference and reads about 0.91 of it")
    print("segment   timing (samples)   quality   deviation kHz   offset kHz   mod index   FSK error   peak error")
    dev, off = r.deviation_hz(fs), r.offset_hz(fs)
    for g in range(N_SEG):
        print(f"{g:7d} {r.delta[g]:18.4f} {r.timing_quality[g]:9.3f} {dev[g] / 1e3:15.2f} {off[g] / 1e3:12.2f} {r.mod_index[g]:11.4f} "
              f"{r.fsk_error[g]:11.4f} {r.peak_error[g]:12.4f}" + ("   <- flagged" if r.flags[g] else ""))
    bits = r.bits("gray")[0][:32]
    print("first bits of segment 0 (Gray):", "".join(map(str, bits)))


if __name__ == "__main__":
    main()
