#!/usr/bin/env python3
"""Timing of the correlation search.

  copy      the box's device-to-device copy rate (1 GiB, torch), which the memory floors are stated against
  valu      the box's FP32 issue rates: tools/ubench/valu_rate (built from valu_rate.hip if it is not there), ns per
            wave-instruction per SIMD of v_fma_f32 with vector operands, with a scalar operand, and of v_pk_fma_f32
  int8      a C3 second, 20e6 interleaved int8 samples in HBM: noise with a Zadoff-Chu preamble every 100 000 samples,
            Correlator.process_device at L = 16, 64, 256, 1024, each next to (a) its memory floor - the bytes read at the
            copy rate - and (b) its FP32 issue floor: 6 L fused multiply-adds per window (4 L for c, 2 L for the energy)
            at the vector-operand rate on every SIMD of the box
  c64       the same as complex64
  streams   256 channelizer streams of a C3 second: [256][78125] complex64, stride 78125 + 3, L = 64
  passes    L = 64, int8: the correlate pass and the three match passes (block maxima + count, scan, emit), each
            launched alone (tdsa_corr_debug_limits); they read what the last whole call left
  variants  the correlate pass alone at 4, 8, 16 windows per thread, with and without packed multiply-adds, and with the
            reference read from LDS or through scalar loads, at L = 64, 256 and 1024
  torch     for scale only, not part of the product: the same metric with stock PyTorch-ROCm as overlap-save through
            torch.fft (blocks of 2^16), no peak search, at L = 64 and L = 1024 on the complex64 second

Every step runs in a child process of its own under a time limit; a step that fails ends the run with exit status 1
(tools/stepbench.py).  Per device figure: warm-up calls, then the median of `--reps` (at least 20)
single calls, each between device events on the handle's stream.  process_device does not wait, so a figure is the
device time of the passes alone.  No time is fixed in advance: each figure stands next to its two floors.

    python tools/corrbench.py [--out profiles/corrbench.txt] [--reps 20] [--steps int8,variants]
"""
import os
import re
import subprocess
import sys

import numpy as np

from stepbench import main, median_us, step_copy

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N = 20_000_000                    # a C3 second
PERIOD = 100_000
LS = (16, 64, 256, 1024)
STREAMS, PER_STREAM, GAP = 256, N // 256, 3
THRESHOLD = 0.8                   # of noise alone at L = 16, one window in 3e10 comes this high
SIMDS_PER_CU = 4
VARIANTS = ((0, "as shipped"), (4, "4 windows per thread, scalar loads, packed (shipped up to L = 128)"),
            (6, "8, reference from LDS (shipped above)"), (7, "8, LDS, packed"), (2, "8, scalar loads"), (1, "4, scalar loads"),
            (3, "16, scalar loads"), (5, "8, scalar loads, packed"))


def preamble(L):
    from topdogspectrumanalyser_amd import zadoff_chu
    p = L + 1
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return zadoff_chu(p, 2)[:L].copy()


def capture_c64(shape, L, period=PERIOD):
    """Noise of power 0.02 with the preamble of length L at amplitude 0.5 every `period` samples; each row starts
    somewhere else."""
    rng = np.random.default_rng(8)
    x = np.empty(shape, dtype=np.complex64)
    x.real = rng.standard_normal(shape, dtype=np.float32) * 0.1
    x.imag = rng.standard_normal(shape, dtype=np.float32) * 0.1
    r = preamble(L) * np.complex64(0.5)
    rows = x.reshape(-1, shape[-1])
    for k in range(rows.shape[0]):
        for s in range(1000 + 37 * k, shape[-1] - L, period):
            rows[k, s:s + L] += r
    return x


def as_i8(x):
    out = np.empty(x.shape[:-1] + (2 * x.shape[-1],), dtype=np.int8)
    out[..., 0::2] = np.clip(np.rint(x.real * 128.0), -128, 127)
    out[..., 1::2] = np.clip(np.rint(x.imag * 128.0), -128, 127)
    return out


def _floors(args, us, n_windows, L, nbytes):
    mem = nbytes / args.copy_bps * 1e6 if args.copy_bps else float("nan")
    simds = args.cus * SIMDS_PER_CU
    fp = n_windows * 6.0 * L / 64.0 * args.fma_ns / simds * 1e-3 if args.fma_ns and simds else float("nan")
    return (f"(a) memory floor {mem:7.1f} us ({nbytes / 1e6:.0f} MB at the copy rate) = {100 * mem / us:4.1f} %; "
            f"(b) FP32 issue floor {fp:8.1f} us (6 L = {6 * L} multiply-adds per window at {args.fma_ns:.2f} ns on {simds:.0f} SIMDs) = "
            f"{100 * fp / us:4.1f} % of the time")


def _whole(args, data, n, fmt, L, streams=1, stride=None, period=PERIOD):
    from topdogspectrumanalyser_amd import Correlator, DeviceBuffer
    with DeviceBuffer.of(data) as d, Correlator(preamble(L), streams, 4096, max_host_samples=streams) as p:
        p.configure(THRESHOLD, L)
        f = lambda: p.process_device(None, d.ptr, n, stride, fmt)
        us = median_us(p, f, args.warm, args.reps)
        p.reset()
        f()
        p.flush()
        first, last = p.read(0), p.read(streams - 1)
    want = len(range(1000, n - L, period))
    assert first.index.tolist() == list(range(1000, n - L, period)) and abs(last.n_matches - want) <= 1, (first.index[:5], want)
    nbytes = streams * n * (8 if data.dtype == np.complex64 else 2)
    return (f"L = {L:4d}: {us[0]:9.1f} us (min {us[1]:.1f}, max {us[2]:.1f}); {_floors(args, us[0], streams * (n - L + 1), L, nbytes)}; "
            f"{first.n_matches} matches, median metric {np.median(first.metric):.3f}, median snr {np.median(first.snr_db):.1f} dB")


def step_valu(args):
    exe = os.path.join(ROOT, "tools", "ubench", "valu_rate")
    if not os.path.exists(exe):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", exe + ".hip", "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rate = {}
    for name in ("v_fma_f32 distinct srcs", "v_pk_fma_f32", "v_fma_f32 v,s,v"):
        rate[name] = float(re.search(r"^%s\s+[\d.]+ ms\s+([\d.]+) ns" % re.escape(name), out, re.M).group(1))
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(fma_ns=rate["v_fma_f32 distinct srcs"], cus=float(cus), text=[
        f"valu: tools/ubench/valu_rate on this box, ns per wave-instruction per SIMD: v_fma_f32 {rate['v_fma_f32 distinct srcs']:.2f}, with a scalar "
        f"operand {rate['v_fma_f32 v,s,v']:.2f}, v_pk_fma_f32 {rate['v_pk_fma_f32']:.2f} (two multiply-adds a lane); {cus} CUs of {SIMDS_PER_CU} SIMDs"])


def step_int8(args):
    from topdogspectrumanalyser_amd import _native as nat
    return dict(text=[f"int8: {N} int8 samples, one stream, a preamble every {PERIOD}"] +
                ["      " + _whole(args, as_i8(capture_c64((N,), L)), N, nat.IN_I8, L) for L in LS])


def step_c64(args):
    from topdogspectrumanalyser_amd import _native as nat
    return dict(text=[f"c64: the same as {N} complex64 samples"] +
                ["      " + _whole(args, capture_c64((N,), L), N, nat.IN_C64, L) for L in LS])


def step_streams(args):
    from topdogspectrumanalyser_amd import _native as nat
    stride, L = PER_STREAM + GAP, 64
    x = capture_c64((STREAMS, stride), L, 20_000)
    x[:, PER_STREAM:] = preamble(L)[:GAP]                  # the gaps would show
    return dict(text=[f"streams: {STREAMS} streams of {PER_STREAM} complex64 samples (stride {stride}), a preamble every 20000, one call",
                      "      " + _whole(args, x, PER_STREAM, nat.IN_C64, L, STREAMS, stride, 20_000)])


def _alone(args, L, masks_variants):
    """us of process_device with each (passes, variant) of the list, over the int8 second."""
    from topdogspectrumanalyser_amd import Correlator, DeviceBuffer
    from topdogspectrumanalyser_amd.correlate import MAX_LAUNCH_TILES
    from topdogspectrumanalyser_amd import _native as nat
    with DeviceBuffer.of(as_i8(capture_c64((N,), L))) as d, Correlator(preamble(L), 1, 4096, max_host_samples=1) as p:
        p.configure(THRESHOLD, L)
        f = lambda: p.process_device(None, d.ptr, N, None, nat.IN_I8)
        f()                                                # what the match passes launched alone read
        out = []
        for passes, variant in masks_variants:
            p._debug_limits(MAX_LAUNCH_TILES, passes, variant)
            out.append(median_us(p, f, args.warm, args.reps)[0])
        return out


def step_passes(args):
    whole, corr, count, scan, emit = _alone(args, 64, ((15, 0), (1, 0), (2, 0), (4, 0), (8, 0)))
    return dict(text=[f"passes: L = 64, int8, each launched alone: correlate {corr:.1f} us, block maxima + count {count:.1f} us, scan {scan:.1f} us, "
                      f"emit {emit:.1f} us; all of them in one call {whole:.1f} us"])


def step_variants(args):
    text = ["variants: the correlate pass alone over the int8 second (the bits are the same from all of them)"]
    for L in (64, 256, 1024):
        us = _alone(args, L, [(1, v) for v, _ in VARIANTS])
        fp = (N - L + 1) * 6.0 * L / 64.0 * args.fma_ns / (args.cus * SIMDS_PER_CU) * 1e-3 if args.fma_ns else float("nan")
        text.append(f"      L = {L:4d} (FP32 issue floor {fp:.1f} us): " + "; ".join(f"{name} {t:.1f} us" for (_, name), t in zip(VARIANTS, us)))
    return dict(text=text)


def step_torch(args):
    import time
    import torch
    text = []
    for L in (64, 1024):
        x = torch.from_numpy(capture_c64((N,), L)).cuda()
        r = torch.from_numpy(preamble(L)).cuda()
        B = 1 << 16
        hop = B - L + 1
        R = torch.conj(torch.fft.fft(r, B))
        ones = torch.fft.fft(torch.ones(L, device="cuda", dtype=torch.complex64), B).conj()
        e_ref = float((r.abs() ** 2).sum())

        nb = -(-(N - L + 1) // hop)                        # blocks of B samples, hop apart: block b completes windows b hop .. + hop - 1

        def metric():
            blocks = torch.nn.functional.pad(x, (0, (nb - 1) * hop + B - N)).unfold(0, B, hop)
            X = torch.fft.fft(blocks, dim=1)
            c = torch.fft.ifft(X * R, dim=1)[:, :hop]
            e = torch.fft.ifft(torch.fft.fft((blocks.abs() ** 2).to(torch.complex64), dim=1) * ones, dim=1)[:, :hop].real
            return (c.abs() ** 2 / (e_ref * e)).reshape(-1)

        for _ in range(3):
            m = metric()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            m = metric()
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / args.reps
        peaks = int((m[:N - L + 1] > THRESHOLD).sum())
        text.append(f"      L = {L:4d}: {per * 1e6:.1f} us per call (wall clock over {args.reps} calls), {peaks} windows above the threshold")
    return dict(text=["torch: for scale only - the metric alone, no peak search, as overlap-save through torch.fft (blocks of 65536) on the complex64 second"] + text)


def header(args):
    return (f"correlation search (tdsa_corr_*): every device figure is the median of {args.reps} single calls after warm-up calls, "
            f"between device events on the handle's stream; the records stay on the device.  threshold {THRESHOLD}, min_distance L")


STEPS = dict(copy=step_copy, valu=step_valu, int8=step_int8, c64=step_c64, streams=step_streams, passes=step_passes,
             variants=step_variants, torch=step_torch)

if __name__ == "__main__":
    main(__file__, STEPS, header, limit_s=300, carry=("fma_ns", "cus"))
