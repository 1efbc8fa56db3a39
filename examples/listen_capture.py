#!/usr/bin/env python3
"""Listen to one channel of a capture, and read the deviation of all of them.

    python examples/listen_capture.py [out.wav]

A complex64 capture at 1.536 Msps holds a broadcast-style FM carrier (a 1 kHz tone, +-50 kHz deviation) in channel 3 of
16 and a weaker one (400 Hz, +-20 kHz) in channel 12.  The 16-channel polyphase bank (oversampled by 2) leaves 16 streams
of 192 kHz in HBM; the demodulator takes all of them from there on the same stream - discriminator, audio filter and
decimation by 4 to 48 kHz, 75 us de-emphasis - and only the audio and five numbers per channel come back to the host.
One channel is written as a 16-bit WAV; the table lists carrier offset and deviation per channel.
"""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import Channelizer, Demodulator, DeviceBuffer, SpectrumEngine, _native as nat  # noqa: E402

FS, M, OS, R = 1.536e6, 16, 2, 4
D = M // OS
SECONDS = 0.5
LISTEN = 3
STATIONS = {3: (1000.0, 50e3, 0.4), 12: (400.0, 20e3, 0.1)}       # channel: (tone Hz, deviation Hz, amplitude)


def capture():
    n = int(SECONDS * FS) // (D * R) * (D * R)
    t = np.arange(n) / FS
    rng = np.random.default_rng(3)
    x = 2e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    centres = np.fft.fftfreq(M, 1.0 / FS)
    for c, (tone, dev, amp) in STATIONS.items():
        x += amp * np.exp(1j * (2 * np.pi * centres[c] * t + dev / tone * np.sin(2 * np.pi * tone * t)))
    return x.astype(np.complex64)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "listen_capture.wav"
    x = capture()
    n = x.size
    with SpectrumEngine(64) as eng, Channelizer(M, FS, OS) as bank, \
            Demodulator("fm", bank.output_rate, R, M, deemphasis=75e-6, max_host_samples=M) as dm:
        ny = bank.outputs_completed_by(n)
        na = dm.outputs_completed_by(ny)
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * M * ny) as d_y, DeviceBuffer(4 * M * na) as d_a:
            bank.process_device(eng, nat.IN_C64, d_x.ptr, n, d_y.ptr, ny)
            dm.process_device(eng, d_y.ptr, ny, ny, d_a.ptr, na)          # behind the bank, on the same stream
            meas = dm.measure()                                           # waits for both
            audio = d_a.get(na, np.float32, 4 * LISTEN * na)
        rate = dm.audio_rate
        skip = dm.first_full_output + bank.first_full_output // R + 1

    audio = audio[skip:]
    pcm = np.clip(np.round(audio / max(float(np.abs(audio).max()), 1e-12) * 0.8 * 32767), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(round(rate)))
        w.writeframes(pcm.tobytes())
    print(f"{n} samples at {FS / 1e6:.3f} Msps -> {M} channels at {FS / D / 1e3:.0f} kHz -> audio at {rate / 1e3:.0f} kHz; "
          f"channel {LISTEN}: {pcm.size} samples written to {path}")
    print("channel   centre kHz   offset Hz   peak+ Hz   peak- Hz     rms Hz   (over the whole capture, the filters' fill included)")
    centres = bank.channel_centres()
    for c in range(M):
        print(f"{c:7d} {centres[c] / 1e3:12.1f} {meas.offset_hz[c]:11.1f} {meas.peak_plus_hz[c]:10.1f} "
              f"{meas.peak_minus_hz[c]:10.1f} {meas.rms_hz[c]:10.1f}" + ("   <- carrier" if c in STATIONS else ""))


if __name__ == "__main__":
    main()
