#!/usr/bin/env python3
"""CCDF and PAPR of a second of IQ, and of every channel of a channelizer at once, without the samples leaving the
device.

    python examples/ccdf_capture.py

Three synthetic seconds at 20 Msps (int8 IQ, made and uploaded in chunks): complex noise, a CW, and QPSK shaped with a
root-raised-cosine filter.  PowerStats reads each chunk in place and keeps integer state in HBM; read() brings a few
KiB back.  Printed per signal: the PAPR and the levels over the mean that the power exceeds 10 %, 1 %, 0.1 % and 0.01 %
of the time - for the noise next to exp(-x), the curve of complex Gaussian noise.  Then one second of noise with a
strong carrier in one channel goes through a 256-channel Channelizer on an engine's stream, and ONE PowerStats call
behind it, on the same stream, gives the table for all 256 channels: the carrier's channel stands out by its low PAPR.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (Channelizer, DeviceBuffer, PowerStats, SpectrumEngine, gaussian_ccdf,  # noqa: E402
                                        rrc_taps, _native as nat)

FS, SECOND, CHUNK = 20e6, 20_000_000, 2_000_000
PROBS = (0.1, 0.01, 0.001, 0.0001)
SPS = 4                                                               # samples per QPSK symbol


def to_int8(x, scale):
    iq = np.empty(2 * x.size, dtype=np.int8)
    iq[0::2] = np.clip(np.round(x.real * scale), -128, 127)
    iq[1::2] = np.clip(np.round(x.imag * scale), -128, 127)
    return iq


def chunk_of(kind, c, rng):
    """Chunk c of a second of `kind`, interleaved int8."""
    n = CHUNK
    if kind == "noise":
        return to_int8(rng.standard_normal(n) + 1j * rng.standard_normal(n), 20.0)
    if kind == "cw":
        t = np.arange(n, dtype=np.float64) + c * n
        return to_int8(np.exp(2j * np.pi * 0.0123 * t), 100.0)
    if kind == "qpsk":                                                # every chunk a burst of its own: the filter's edges are cut off
        taps = rrc_taps(SPS, 0.35, 8).astype(np.float64)
        sym = (rng.integers(0, 2, n // SPS + 16) * 2 - 1) + 1j * (rng.integers(0, 2, n // SPS + 16) * 2 - 1)
        up = np.zeros(sym.size * SPS, dtype=np.complex128)
        up[::SPS] = sym
        y = np.convolve(up, taps, mode="same")[8 * SPS:8 * SPS + n]
        return to_int8(y, 60.0 / np.sqrt(2.0) * np.sqrt(SPS))
    t = np.arange(n, dtype=np.float64) + c * n                        # "band": noise and a carrier at 2.5 MHz
    return to_int8(0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.5 * np.exp(2j * np.pi * 2.5e6 / FS * t), 127.0)


def row(name, s, k=0):
    lv = s.level_db(PROBS, k)
    return f"  {name:10s} {s.papr_db[k]:8.2f} " + " ".join(f"{v:9.2f}" for v in lv)


def main():
    rng = np.random.default_rng(2)
    print(f"one second at {FS / 1e6:g} Msps, int8 IQ: PAPR, and the level over the mean exceeded with probability")
    print("  signal      PAPR dB " + " ".join(f"{100 * q:8g}%" for q in PROBS))
    with PowerStats(1) as ps, DeviceBuffer(2 * CHUNK) as d_iq:
        for kind in ("noise", "cw", "qpsk"):
            ps.reset()
            for c in range(SECOND // CHUNK):
                iq = chunk_of(kind, c, rng)
                ps.read()                                             # the previous chunk has left d_iq
                d_iq.put(iq)
                ps.process_device(None, d_iq.ptr, CHUNK, in_format=nat.IN_I8)
            s = ps.read()
            print(row(kind, s))
            if kind == "noise":
                ref = 10 * np.log10(-np.log(PROBS))
                print(f"  {'exp(-x)':10s} {'':8s} " + " ".join(f"{v:9.2f}" for v in ref)
                      + f"   (ccdf at 6 dB: {s.ccdf(6.0):.5f}, reference {gaussian_ccdf(6.0):.5f})")

    M = 256
    with SpectrumEngine(64) as eng, Channelizer(M, FS) as ch, PowerStats(M) as ps, DeviceBuffer(2 * CHUNK) as d_iq:
        per_chunk = CHUNK // M + 1
        with DeviceBuffer(8 * M * per_chunk) as d_ch:
            for c in range(SECOND // CHUNK):
                iq = chunk_of("band", c, rng)
                ps.read()                                             # both buffers are free again
                d_iq.put(iq)
                n_out = ch.process_device(eng, nat.IN_I8, d_iq.ptr, CHUNK, d_ch.ptr, per_chunk)
                ps.process_device(eng, d_ch.ptr, n_out, per_chunk)    # behind the channelizer, on the engine's stream
            s = ps.read()
    papr = s.papr_db
    k = int(np.argmin(papr))
    centres = ch.channel_centres()
    print(f"{M} channels of {FS / M / 1e3:.3f} kHz, {int(s.n_total[0])} samples each, one call per chunk for all of them:")
    print(f"  PAPR {np.median(papr):.2f} dB in the median channel; the lowest, {papr[k]:.2f} dB, in channel {k} at "
          f"{centres[k] / 1e6:+.4f} MHz (the carrier is at +2.5000 MHz)")
    print(row(f"ch {k}", s, k))
    print(row("ch 0", s, 0))


if __name__ == "__main__":
    main()
