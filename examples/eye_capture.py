#!/usr/bin/env python3
"""Eye diagrams of a GFSK and of a QPSK carrier on their recovered symbol clocks, without the samples leaving the device.

    python examples/eye_capture.py

Two complex64 captures at 16 Msps.  The first holds a 1 Msym/s GFSK carrier (BT 0.5, modulation index 0.5), 21 kHz off
tune: the down-converter (decimation 2) leaves 8 samples per symbol in HBM, FskAnalyzer finds the symbol clock of every
4096-sample segment, and EyeDiagram("fm") folds the same samples on those clocks into one eye of the frequency.  The
second holds a 1 Msym/s QPSK carrier, root-raised-cosine shaped, 3 kHz off tune: the down-converter is the matched
filter, SymbolSync recovers timing and carrier per segment, and EyeDiagram("iq") folds the samples into an I and a Q eye,
derotated by the recovered carrier.  All of it runs on the engine's stream; what comes back are the analysers' records
and the two integer images.  Printed: the openings (height in the value's unit and as a fraction of the level spacing,
width as a fraction of a symbol), and the GFSK eye as characters.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import (DeviceBuffer, DownConverter, EyeDiagram, EyeImage, FskAnalyzer, SpectrumEngine,  # noqa: E402
                                        SymbolSync, rrc_taps, _native as nat)

FS, SYMBOL_RATE, D = 16e6, 1e6, 2
SPS_IN = int(FS / SYMBOL_RATE)
SPS = SPS_IN // D
SEG, N_SEG = 4096, 4
SNR_DB, BT, H_MOD, ALPHA, SPAN = 30.0, 0.5, 0.5, 0.5, 3        # 97 taps: the down-converter takes 64 per phase
POINTS, ROWS = 32, 64


def noise(rng, n):
    s = 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0)
    return s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def gfsk(rng, n_sym, offset_hz):
    f = np.repeat(2.0 * rng.integers(0, 2, n_sym) - 1.0, SPS_IN) * (H_MOD / 2 / SPS_IN)      # cycles per sample
    sigma = math.sqrt(math.log(2.0)) / (2.0 * math.pi * BT) * SPS_IN
    t = np.arange(-4 * SPS_IN, 4 * SPS_IN + 1)
    gauss = np.exp(-0.5 * (t / sigma) ** 2)
    f = np.convolve(f, gauss / gauss.sum(), mode="same") + offset_hz / FS
    x = np.exp(2j * np.pi * np.cumsum(f))
    return (x + noise(rng, x.size)).astype(np.complex64)


def qpsk(rng, n_sym, offset_hz):
    up = np.zeros(n_sym * SPS_IN, dtype=np.complex128)
    up[::SPS_IN] = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n_sym)))
    x = np.convolve(up, rrc_taps(SPS_IN, ALPHA, SPAN).astype(np.float64))       # unit energy: unit symbols behind the matched filter
    x = x * np.exp(2j * np.pi * offset_hz / FS * np.arange(x.size) + 0.4j)
    return (x + noise(rng, x.size)).astype(np.complex64)


def fold(eng, ddc, analyser, eye, x):
    """capture -> down-converter -> analyser -> eye on the engine's stream; (the analyser's result, the image)."""
    K = analyser.symbols_per_segment(SEG)
    ny = (x.size + D - 1) // D
    skip = 8 * ddc.first_full_output                                 # past the filter's fill, 8-byte samples
    unit = 8 if isinstance(analyser, SymbolSync) else 4
    with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * ny) as d_y, DeviceBuffer(unit * K * N_SEG) as d_out:
        ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
        seg = d_y.at(skip, 8 * SEG * N_SEG)
        r = analyser.process_device(eng, seg, SEG, SEG, N_SEG, d_out.ptr, K)          # behind it, on the same stream
        eye.process_device(eng, seg, SEG, SEG, N_SEG, eye.clocks(r))                  # and the eye behind both
        return r, eye.read()


def show(img: EyeImage, eye: int = 0) -> None:
    two = img.two_symbols()[eye][::-1]                               # the highest row first
    peak = max(1, int(two.max()))
    for row in two[::2]:
        print("    " + "".join(" .:-=+*#%@"[min(9, int(math.ceil(9 * int(v) / peak)))] for v in row))


def main():
    rng = np.random.default_rng(7)
    n_sym = (SEG * N_SEG * D) // SPS_IN + 64
    with SpectrumEngine(64) as eng:
        with DownConverter(D, FS) as ddc, FskAnalyzer(SPS, 2) as fsk, \
                EyeDiagram(SPS, "fm", points=POINTS, rows=ROWS, v_range=(-0.12, 0.13)) as eye:
            r, img = fold(eng, ddc, fsk, eye, gfsk(rng, n_sym, 21e3))
        th = float(EyeImage.thresholds_from(r)[0])
        height, width = img.opening(th)
        spacing = 2.0 * float(np.median(r.records["dev"]))
        print(f"GFSK, BT {BT}, h = {H_MOD}: {img.segments} segments of {SEG} samples at {SPS} samples per symbol, {int(img.n_points[0])} "
              f"points in {POINTS} x {ROWS} bins ({int(img.n_under[0] + img.n_over[0])} outside the range)")
        print(f"  opening around the threshold {th * FS / D / 2 / 1e3:.1f} kHz: {height * FS / D / 2 / 1e3:.1f} kHz high "
              f"({height / spacing:.2f} of the level spacing), {width:.2f} of a symbol wide")
        show(img)
        with DownConverter(D, FS, taps=rrc_taps(SPS_IN, ALPHA, SPAN)) as ddc, SymbolSync(SPS, "qpsk") as sync, \
                EyeDiagram(SPS, "iq", points=POINTS, rows=ROWS, v_range=(-1.6, 1.6)) as eye:
            r, img = fold(eng, ddc, sync, eye, qpsk(rng, n_sym, 3e3))
        print(f"QPSK, root-raised cosine {ALPHA}: {img.segments} segments, {int(img.n_points[0])} points per eye")
        for q, name in enumerate("IQ"):
            height, width = img.opening(0.0, eye=q)
            print(f"  {name} eye around 0: {height:.3f} high (the points lie {math.sqrt(2.0):.3f} apart), {width:.2f} of a symbol wide")
        assert all(v > 0 for q in (0, 1) for v in img.opening(0.0, eye=q)), "the QPSK eye is shut"


if __name__ == "__main__":
    main()
