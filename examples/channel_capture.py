#!/usr/bin/env python3
"""Every channel of a capture at once: a stitched high-resolution row, and one channel's envelope in zero span.

    python examples/channel_capture.py

An int8 IQ capture at 20 Msps goes through the 64-channel polyphase bank (oversampled by 2) in one pass.  ChannelSpectra
turns every channel's stream into 1024-point spectra in one frame-kernel launch and stitches the central half of each
into one 32768-bin row of the whole capture at RBW 610 Hz.  The same capture through a plain Channelizer leaves 64
complex64 streams in HBM; one of them - the channel a pulsed carrier sits in - goes straight into a ZeroSpan ring, on the
same stream, without touching the host.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (Channelizer, ChannelSpectra, DeviceBuffer, SpectrumEngine, ZeroSpan,  # noqa: E402
                                        _native as nat)

FS, FC = 20e6, 2.45e9
M, OS, NFFT, FRAMES = 64, 2, 1024, 4
D = M // OS
SAMPLES = FRAMES * D * NFFT
F_CW, F_PULSED = 3.3e6, -5.47e6            # a steady carrier and one keyed at 20 kHz


def capture():
    rng = np.random.default_rng(3)
    t = np.arange(SAMPLES) / FS
    keyed = (np.floor(t * 40e3) % 2 == 0)
    x = 0.3 * np.exp(2j * np.pi * F_CW * t) + 0.2 * keyed * np.exp(2j * np.pi * F_PULSED * t)
    x += 0.01 * (rng.standard_normal(SAMPLES) + 1j * rng.standard_normal(SAMPLES))
    iq = np.empty(2 * SAMPLES, np.int8)
    iq[0::2] = np.clip(np.round(x.real * 127), -128, 127)
    iq[1::2] = np.clip(np.round(x.imag * 127), -128, 127)
    return iq


def main():
    iq = capture()
    with ChannelSpectra(FS, M, NFFT, oversample=OS, max_frames=FRAMES) as cs:
        rows = cs.process(iq)                                            # [M][FRAMES][NFFT] dB
        idx = cs.stitch_index()
        axis = cs.freq_bins(FC).reshape(-1)[idx]
        row = rows[:, -1, :].reshape(-1)[idx]                            # the last frame: past the filter's fill
        print(f"{SAMPLES} samples -> {M} channels x {FRAMES} frames of {NFFT} bins; stitched row: {row.size} bins, "
              f"RBW {cs.rbw:.1f} Hz, {axis[0] / 1e6:.4f} .. {axis[-1] / 1e6:.4f} MHz")
        for k in np.argsort(row)[-2:][::-1]:
            print(f"  peak {row[k]:7.2f} dB at {axis[k] / 1e6:.4f} MHz")

    with Channelizer(M, FS, OS) as bank, SpectrumEngine(64) as eng, \
            ZeroSpan(bank.output_rate, detector="mag", buffer_s=0.01) as zs:
        c = int(np.argmin(np.abs(bank.channel_centres() - F_PULSED)))
        n_out = bank.outputs_completed_by(SAMPLES)
        with DeviceBuffer.of(iq) as d_in, DeviceBuffer(8 * M * n_out) as d_y:
            bank.process_device(eng, nat.IN_I8, d_in.ptr, SAMPLES, d_y.ptr, n_out)
            zs.push_device(eng, nat.IN_C64, d_y.at(8 * c * n_out, 8 * n_out), n_out)     # channel c's run, behind the bank
            v = zs.view("rise", level=0.05, points=64, n_display=n_out // 2)
            print(f"channel {c} (centre {bank.channel_centres(FC)[c] / 1e6:.4f} MHz, {bank.output_rate / 1e3:.1f} kHz wide): "
                  f"{v.total} envelope samples in the ring, triggered={v.triggered}, min {v.min:.3f}, max {v.max:.3f}, "
                  f"{v.n_rise} rising edges in the window")
            eng.synchronize()


if __name__ == "__main__":
    main()
