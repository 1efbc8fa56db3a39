#!/usr/bin/env python3
"""Where the bursts of a capture start, how far off tune each is, and its EVM - without the samples leaving the device.

    python examples/sync_capture.py

A complex64 capture at 8 Msps, 50 ms of noise with six QPSK bursts of 1 Msym/s in it: a Zadoff-Chu preamble of 31 symbols,
then 300 random symbols, root-raised-cosine shaped, each burst at a random even offset (so that it starts on an output
sample of the decimation by 2) and a few kHz off the nominal carrier.  The capture goes through a DownConverter - the
matched filter, tuned to the nominal carrier - on an engine's stream in chunks that cut bursts and preambles anywhere;
behind it, on the same stream, a Correlator searches the decimated stream for the core of the preamble as the matched
filter delivers it.  Its matches say where the bursts start and, from the phase between the preamble's two halves, how far
off tune each is; a segment of payload behind every match goes to SymbolSync and its symbols to Constellation.
Printed per burst: the planted and the found start in input samples, the planted and the found carrier offset, the
metric, the SNR estimate and the EVM.  The starts must agree exactly, the offsets within 300 Hz.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (Constellation, Correlator, DeviceBuffer, DownConverter, SpectrumEngine, SymbolSync,  # noqa: E402
                                        from_symbols, rrc_taps, zadoff_chu, _native as nat)

FS, SYMBOL_RATE, D, TUNE_HZ = 8e6, 1e6, 2, 1.5e6
SPS_IN = int(FS / SYMBOL_RATE)
SPS = SPS_IN // D
ALPHA, SPAN, SNR_DB = 0.35, 6, 25.0
N_PRE, N_PAY, N_BURSTS = 31, 300, 6
N, CHUNK = 400_000, 37_777                     # 50 ms; a chunk length that is no multiple of anything
SEG = 1024                                     # payload samples per burst handed to SymbolSync: 256 symbols
TOLERANCE_HZ = 300.0


def capture(rng):
    """(x, starts, offsets): the capture, where each burst's first symbol enters the shaping filter, its offset in Hz."""
    qpsk = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    pre = zadoff_chu(N_PRE, 3).astype(np.complex128)
    taps = rrc_taps(SPS_IN, ALPHA, SPAN).astype(np.float64) * np.sqrt(SPS_IN)
    s = 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0)
    x = s * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    slot = N // N_BURSTS
    starts = [b * slot + 2 * int(rng.integers(500, (slot - 4000) // 2)) for b in range(N_BURSTS)]
    offsets = rng.uniform(-8e3, 8e3, N_BURSTS)
    t = np.arange(N) / FS
    for s0, off in zip(starts, offsets):
        up = np.zeros((N_PRE + N_PAY) * SPS_IN, dtype=np.complex128)
        up[::SPS_IN] = np.concatenate([pre, qpsk[rng.integers(0, 4, N_PAY)]])
        burst = np.convolve(up, taps)
        seg = slice(s0, s0 + burst.size)
        x[seg] += burst * np.exp(2j * np.pi * (TUNE_HZ + off) * t[seg] + 1j * rng.uniform(0, 2 * np.pi))
    return x.astype(np.complex64), starts, offsets


def main():
    rng = np.random.default_rng(11)
    x, starts, offsets = capture(rng)
    taps = rrc_taps(SPS_IN, ALPHA, SPAN)
    # the preamble as the decimated stream carries it: SPS samples per symbol, shaped by both root-raised cosines; of
    # that its core, from the first symbol's peak to the last one's: there the envelope is level, which is what the
    # carrier estimate from the two halves assumes, and no payload symbol reaches far into it
    rrc = rrc_taps(SPS, ALPHA, SPAN).astype(np.float64)
    raised = np.convolve(rrc, rrc)
    reach = (raised.size - 1) // 2
    reference = from_symbols(zadoff_chu(N_PRE, 3), SPS, raised)[reach:reach + N_PRE * SPS].copy()
    ny = N // D + 1
    with SpectrumEngine(64) as eng, DownConverter(D, FS, TUNE_HZ, taps=taps) as ddc, Correlator(reference, capacity=64) as cor, \
            SymbolSync(SPS, "qpsk") as sync, Constellation(modulation="qpsk") as cst, \
            DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * ny) as d_y:
        cor.configure(0.5)
        done = 0
        for k in range(0, N, CHUNK):
            n = min(CHUNK, N - k)
            got = ddc.process_device(eng, nat.IN_C64, d_x.ptr + 8 * k, n, d_y.ptr + 8 * done)
            cor.process_device(eng, d_y.ptr + 8 * done, got)        # behind it on the engine's stream: nobody waits
            done += got
        cor.flush()
        found = cor.read(0)
        K = sync.symbols_per_segment(SEG)
        # a match is the peak of the first preamble symbol: the payload begins the preamble and a few symbols behind it
        first = [int(i) + (N_PRE + 4) * SPS for i in found.index]
        with DeviceBuffer(8 * K * max(1, len(found))) as d_s:
            for b, m0 in enumerate(first):
                sync.process_device(eng, d_y.at(8 * m0, 8 * SEG), SEG, SEG, 1, d_s.ptr + 8 * K * b, K)
            evm = cst.process_segments(eng, d_s.ptr, nat.IN_C64, K, K, len(found))[1] if len(found) else []
    print(f"{N_BURSTS} QPSK bursts of {N_PRE} + {N_PAY} symbols at {SYMBOL_RATE / 1e6:g} Msym/s in {N} samples at {FS / 1e6:g} Msps, noise {SNR_DB:g} dB "
          f"down; reference of {reference.size} samples at {SPS} per symbol, {found.n_windows} windows searched in chunks of {CHUNK}")
    print("burst   planted start   found start   planted Hz    found Hz   metric   snr dB   EVM rms")
    hz = found.freq * FS / D
    for b in range(len(found)):
        at = (int(found.index[b]) - reach) * D            # the first symbol entered the shaping filter a reach earlier
        print(f"{b:5d} {starts[b] if b < len(starts) else -1:15d} {at:13d} {offsets[b] if b < len(starts) else 0:12.1f} {hz[b]:11.1f} "
              f"{found.metric[b]:8.4f} {found.snr_db[b]:8.1f} {evm[b]:9.4f}")
    assert [(int(i) - reach) * D for i in found.index] == starts, "a burst was not found where it was planted"
    assert np.abs(hz - offsets).max() <= TOLERANCE_HZ, "a carrier offset is off by more than the tolerance"
    print(f"all {N_BURSTS} starts exact, carrier offsets within {np.abs(hz - offsets).max():.0f} Hz (tolerance {TOLERANCE_HZ:g} Hz)")


if __name__ == "__main__":
    main()
