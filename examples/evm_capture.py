#!/usr/bin/env python3
"""EVM of a digitally modulated capture, without the samples leaving the device.

    python examples/evm_capture.py [qpsk | bpsk | 8psk | 16qam | 64qam]

A complex64 capture at 8 Msps holds a 1 Msym/s carrier, root-raised-cosine shaped (excess bandwidth 0.35), 1.3 kHz off
tune, at an arbitrary symbol phase, with noise 35 dB down.  The down-converter is the matched filter (RRC taps,
decimation 2), which leaves 4 samples per symbol in HBM; SymbolSync finds the symbol clock and the carrier of every
4096-sample segment and leaves one sample per symbol, derotated, next to them; Constellation reads those in place.  All
three run on one engine stream; per segment three numbers and an EVM come back to the host.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (Constellation, DeviceBuffer, DownConverter, SpectrumEngine, SymbolSync,  # noqa: E402
                                        _native as nat)
from topdogspectrumanalyser_amd.analytics import constellation_points  # noqa: E402
from topdogspectrumanalyser_amd.symbols import rrc_taps  # noqa: E402

FS, SYMBOL_RATE, D = 8e6, 1e6, 2
SPS_IN = int(FS / SYMBOL_RATE)
SPS = SPS_IN // D
OFFSET_HZ, SNR_DB, ALPHA = 1300.0, 35.0, 0.35
SEG, N_SEG = 4096, 8
SPAN = 6                       # symbols to either side: 97 taps, within the down-converter's 64 per phase


def capture(mod, n_sym):
    rng = np.random.default_rng(7)
    pts = constellation_points(mod).astype(np.float64)
    pts = pts[:, 0] + 1j * pts[:, 1]
    up = np.zeros(n_sym * SPS_IN, dtype=np.complex128)
    up[3::SPS_IN] = pts[rng.integers(0, pts.size, n_sym)]           # the symbol instants: 3 samples into each period
    x = np.convolve(up, rrc_taps(SPS_IN, ALPHA, SPAN).astype(np.float64) * np.sqrt(SPS_IN))
    x *= np.exp(1j * (2 * np.pi * OFFSET_HZ / FS * np.arange(x.size) + 0.4))
    s = 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0)                    # the shaped symbols have unit power per sample
    x += s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)


def main():
    mod = sys.argv[1] if len(sys.argv) > 1 else "qpsk"
    x = capture(mod, (SEG * N_SEG * D) // SPS_IN + 64)
    taps = rrc_taps(SPS_IN, ALPHA, SPAN)
    with SpectrumEngine(64) as eng, DownConverter(D, FS, taps=taps) as ddc, SymbolSync(SPS, mod) as sync, \
            Constellation(modulation=mod) as cst:
        K = sync.symbols_per_segment(SEG)
        ny = (x.size + D - 1) // D
        skip = 8 * ddc.first_full_output                             # past the matched filter's fill, 8-byte samples
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * ny) as d_y, DeviceBuffer(8 * K * N_SEG) as d_s:
            ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            r = sync.process_device(eng, d_y.at(skip, 8 * SEG * N_SEG), SEG, SEG, N_SEG, d_s.ptr, K)   # behind it, on the same stream
            _, evm = cst.process_segments(eng, d_s.ptr, nat.IN_C64, K, K, N_SEG)            # K symbols per segment, in place
    print(f"{mod}, {SYMBOL_RATE / 1e6:g} Msym/s at {FS / 1e6:g} Msps, {OFFSET_HZ:g} Hz off tune, noise {SNR_DB:g} dB down: "
          f"{N_SEG} segments of {SEG} samples at {SPS} samples per symbol, {K} symbols each")
    print("segment   timing (samples)   quality   carrier Hz    phase rad     lock   EVM rms")
    hz = r.freq_hz(SYMBOL_RATE)
    for g in range(N_SEG):
        print(f"{g:7d} {r.delta[g]:18.4f} {r.timing_quality[g]:9.3f} {hz[g]:12.1f} {r.phase[g]:12.4f} {r.lock[g]:8.0f} {evm[g]:9.4f}"
              + ("   <- not finite" if r.flags[g] else ""))


if __name__ == "__main__":
    main()
