#!/usr/bin/env python3
"""The error summary of a 16QAM burst, without the samples leaving the device.

    python examples/modq_capture.py

A complex64 capture at 16 Msps holds a 1 Msym/s 16QAM carrier, root-raised-cosine shaped, 3 kHz off tune, through an
amplifier with a gain, a turn, an IQ offset and an IQ imbalance.  The down-converter (decimation 2) is the matched
filter and leaves 8 samples per symbol in HBM, SymbolSync recovers timing and carrier of every 8192-sample segment, and
ModQuality reads its symbols in place: two rounds of decision and least-squares fit, then the error of every symbol
against its point.  All of it runs on the engine's stream; what comes back are the records.  Printed per segment: gain,
phase, IQ offset, EVM, MER, magnitude and phase error, rho, the decisions that moved between the rounds - and, from the
indices, the IQ imbalance and the first bits.  The bits carry the four-fold rotation the carrier recovery leaves open;
a quarter turn of it swaps I and Q, and with them the sign of the two imbalance figures.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (DeviceBuffer, DownConverter, ModQuality, SpectrumEngine, SymbolSync, rrc_taps,  # noqa: E402
                                        _native as nat)
from topdogspectrumanalyser_amd.analytics import constellation_points  # noqa: E402
from topdogspectrumanalyser_amd.modquality import result_from  # noqa: E402

FS, SYMBOL_RATE, D = 16e6, 1e6, 2
SPS_IN = int(FS / SYMBOL_RATE)
SPS = SPS_IN // D
SEG, N_SEG = 8192, 4
SNR_DB, ALPHA, SPAN = 35.0, 0.5, 3                   # 97 taps: the down-converter takes 64 per phase
MOD = "16qam"
Q_GAIN_DB, Q_SKEW_DEG, OFFSET = -0.3, 1.5, 0.01 - 0.02j


def burst(rng, n_sym):
    pts = np.asarray(constellation_points(MOD), dtype=np.float64)
    i = rng.integers(0, pts.shape[0], n_sym)
    up = np.zeros(n_sym * SPS_IN, dtype=np.complex128)
    up[::SPS_IN] = pts[i, 0] + 1j * pts[i, 1]
    x = np.convolve(up, rrc_taps(SPS_IN, ALPHA, SPAN).astype(np.float64))       # unit energy: unit symbols behind the matched filter
    x = x.real + 10.0 ** (Q_GAIN_DB / 20.0) * np.exp(1j * math.radians(Q_SKEW_DEG)) * 1j * x.imag + OFFSET
    x = 0.6 * x * np.exp(2j * np.pi * 3e3 / FS * np.arange(x.size) + 0.4j)
    s = 0.6 * 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0)
    return (x + s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))).astype(np.complex64)


def main():
    rng = np.random.default_rng(7)
    x = burst(rng, (SEG * N_SEG * D) // SPS_IN + 64)
    with SpectrumEngine(64) as eng, DownConverter(D, FS, taps=rrc_taps(SPS_IN, ALPHA, SPAN)) as ddc, \
            SymbolSync(SPS, MOD) as sync, ModQuality(MOD) as modq:
        K = sync.symbols_per_segment(SEG)
        ny = (x.size + D - 1) // D
        skip = 8 * ddc.first_full_output                             # past the filter's fill, 8-byte samples
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * ny) as d_y, DeviceBuffer(8 * K * N_SEG) as d_s, \
                DeviceBuffer(K * N_SEG) as d_i, DeviceBuffer(8 * K * N_SEG) as d_e:
            ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            s = sync.process_device(eng, d_y.at(skip, 8 * SEG * N_SEG), SEG, SEG, N_SEG, d_s.ptr, K)   # behind it, on the same stream
            r = modq.process_device(eng, d_s.ptr, K, K, N_SEG, d_i.ptr, K, d_e.ptr)             # and this stage behind both
            idx = d_i.get((N_SEG, K), np.uint8)
            err = d_e.get((N_SEG, K), np.complex64)
    r = result_from(r.records, idx, err, K, modq.table, MOD)          # the same figures, now with the indices beside them
    gdb, qdeg = r.iq_imbalance()
    print(f"{MOD}, root-raised cosine {ALPHA}, {N_SEG} segments of {SEG} samples at {SPS} samples per symbol, K = {K}; "
          f"carrier {np.median(s.freq_hz(SYMBOL_RATE)):.0f} Hz off")
    for g in range(N_SEG):
        print(f"  segment {g}: gain {r.gain[g]:.4f}, phase {math.degrees(r.phase[g]):+.2f} deg, IQ offset {r.iq_offset_db[g]:.1f} dB, "
              f"EVM {100 * r.evm_rms[g]:.2f} % rms / {100 * r.evm_peak[g]:.2f} % peak, MER {r.mer_db[g]:.1f} dB, magnitude error "
              f"{100 * r.mag_error_rms[g]:.2f} %, phase error {r.phase_error_rms_deg[g]:.2f} deg, rho {r.rho[g]:.5f}, "
              f"{int(r.changed[g])} decisions moved, IQ imbalance {gdb[g]:+.2f} dB / {qdeg[g]:+.2f} deg")
    print(f"  the error vector of segment 0 over time: rms {np.sqrt(np.mean(np.abs(err[0]) ** 2)):.4f} of the unit-rms table; "
          f"first bits {''.join(map(str, r.bits('gray')[0, :32]))}")
    assert not r.flags.any() and np.all(r.evm_rms < 0.1), "the constellation did not lock"


if __name__ == "__main__":
    main()
