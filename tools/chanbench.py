#!/usr/bin/env python3
"""Timing of the polyphase channelizer on one C3 second: 20e6 int8 IQ samples resident in HBM,
the default prototype (zoom.design_decimator(M), 34 taps per branch).

  copy     the box's device-to-device copy rate (1 GiB, torch), which the memory floor is stated against
  bank     M in {8, 64, 256} x os in {1, 2}: one Channelizer.process_device call over the whole second, next to its
           memory floor (2 bytes in and 8 os bytes out per input sample at the copy rate) and next to M passes of
           zoom.DownConverter at the same decimation, one per channel, measured in the same process.  The down-converter
           takes at most 64 D taps, so at os = 2 its passes run 32 taps per branch (64 per phase of D) and the line says so
  spectra  ChannelSpectra end to end at M = 64, os = 2, nfft = 1024: the bank and all 64 x 610 frames in one launch
  diff     the largest |difference| between channel 5 and the DownConverter tuned to 5 fs / M, on the same block

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per figure: warm-up calls, then the median of `--reps` (at least 20) single
calls, each between device events on the engine's stream the work is launched on.

    python tools/chanbench.py [--out profiles/chanbench.txt] [--reps 20] [--steps copy,bank_64_2]
"""
import functools
import os
import sys

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

FS = 20e6
N_SEC = 20_000_000
SHAPES = [(M, os_) for M in (8, 64, 256) for os_ in (1, 2)]


def capture(n):
    from topdogspectrumanalyser_amd import DeviceBuffer
    rng = np.random.default_rng(4)
    iq = rng.integers(-128, 128, 2 * n).astype(np.int8)
    return iq, DeviceBuffer.of(iq)


def step_bank(args, M, os_):
    from topdogspectrumanalyser_amd import Channelizer, DeviceBuffer, DownConverter, SpectrumEngine, _native as nat
    from topdogspectrumanalyser_amd.zoom import design_decimator
    D = M // os_
    n = N_SEC // D * D
    n_out = n // D
    _, d_in = capture(n)
    d_out = DeviceBuffer(8 * M * n_out)
    with SpectrumEngine(64) as eng, Channelizer(M, FS, os_) as bank:
        us, lo, hi = median_us(eng, lambda: bank.process_device(eng, nat.IN_I8, d_in.ptr, n, d_out.ptr, n_out),
                               args.warm, args.reps)
        floor = n * (2 + 8 * os_) / args.copy_bps * 1e6
        taps = bank.taps if bank.taps.size <= 64 * D else design_decimator(M, 32)
        with DownConverter(D, FS, 0.0, taps=taps) as ddc:
            def passes():
                for c in range(M):
                    nat.check(nat.lib.tdsa_ddc_set_nco(ddc._h, (c << 32) // M))
                    ddc.process_device(eng, nat.IN_I8, d_in.ptr, n, d_out.at(8 * c * n_out))
            us_d = median_us(eng, passes, 1, args.reps)
    for p in (d_in, d_out):
        p.close()
    return dict(text=[
        f"bank M={M:3d} os={os_}: {n} samples, {bank.taps.size // M} taps per branch: {us:9.1f} us (min {lo:.1f}, max {hi:.1f}); "
        f"memory floor {floor:8.1f} us ({2 + 8 * os_} bytes per sample at the copy rate) = {100 * floor / us:5.1f}% of the time; "
        f"{M} DownConverter passes at D={D}, {taps.size // M} taps per branch: {us_d[0]:10.1f} us "
        f"({us_d[0] / M:7.1f} us per pass) = {us_d[0] / us:6.1f} x the bank"])


def step_spectra(args):
    from topdogspectrumanalyser_amd import ChannelSpectra, DeviceBuffer, _native as nat
    M, os_, nfft = 64, 2, 1024
    F = N_SEC // (M // os_ * nfft)
    n = F * (M // os_) * nfft
    _, d_in = capture(n)
    d_rows = DeviceBuffer(4 * M * F * nfft)
    with ChannelSpectra(FS, M, nfft, oversample=os_, max_frames=F) as cs:
        us, lo, hi = median_us(cs.engine, lambda: cs.process_device(nat.IN_I8, d_in.ptr, n, d_rows.ptr),
                               args.warm, args.reps)
        rbw = cs.rbw
    for p in (d_in, d_rows):
        p.close()
    return dict(text=[
        f"spectra M={M} os={os_} nfft={nfft}: {n} samples -> {M} x {F} frames ({M * F} in one frame-kernel launch), dB rows "
        f"in HBM, RBW {rbw:.1f} Hz: {us:9.1f} us (min {lo:.1f}, max {hi:.1f})"])


def step_diff(args):
    from topdogspectrumanalyser_amd import Channelizer, DownConverter
    M, c, n = 64, 5, 1 << 20
    rng = np.random.default_rng(5)
    iq = rng.integers(-128, 128, 2 * n).astype(np.int8)
    with Channelizer(M, FS, 1) as bank, DownConverter(M, FS, c * FS / M, taps=bank.taps) as ddc:
        assert ddc.phase_step == (c << 32) // M
        y = bank.process(iq)[c]
        z = ddc.process(iq)
    scale = float(np.abs(z).max())
    return dict(text=[
        f"diff M={M} os=1: channel {c} against the DownConverter tuned to {c} fs / M over {n} samples ({y.size} outputs): "
        f"largest |difference| {float(np.abs(y - z).max()):.3e}, largest |output| {scale:.3e}"])


def header(args):
    return (f"polyphase channelizer on one C3 second ({N_SEC} int8 IQ samples in HBM, default prototype); every figure is "
            f"the median of {args.reps} single calls after warm-up calls, between device events on the stream the work runs on")


STEPS = dict(copy=step_copy, **{f"bank_{M}_{os_}": functools.partial(step_bank, M=M, os_=os_) for M, os_ in SHAPES},
             spectra=step_spectra, diff=step_diff)

if __name__ == "__main__":
    main(__file__, STEPS, header)
