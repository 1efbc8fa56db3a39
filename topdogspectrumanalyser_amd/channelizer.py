"""Polyphase channelizer: every fs / M channel of a capture in one pass on the device.

What M passes of zoom.DownConverter tuned to c fs / M would give, c = 0 .. M - 1, from one read of the input: a branch
filter of T / M taps per output replaces the T-tap mixer-plus-FIR, and one M-point transform runs per output instant.

  Channelizer      unpack + branch FIR + circular shift + inverse DFT in one HIP pass (tdsa_chan_*); the outputs are
                   stored channel-major, so every channel is a complex64 stream in HBM that SpectrumEngine.process_device,
                   ZeroSpan.push_device and Constellation take as they are.  History stays on the device: any split of
                   the input into calls gives the same bits
  ChannelSpectra   a Channelizer feeding one SpectrumEngine of nfft points: the frames of all channels in ONE frame-kernel
                   launch, rows [M][F][nfft] dB, and the index that stitches them into one row of the whole capture

Channel c is centred at c fs / M for c < M / 2 and at (c - M) fs / M from there on (FFT order).  With the default
prototype (zoom.design_decimator(M): -6 dB at the channel edge fs / 2M, >= 100 dB beyond 0.6 fs / M) and oversample = 2
every alias lies >= 100 dB down inside +-fs / 2M of a channel's centre.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat
from .devmem import DeviceBuffer
from .analytics import _iq_input
from .engine import SpectrumEngine
from .utils.constants import DSPConstants
from .zoom import as_taps, check_same_device, design_decimator, outputs_completed, zoom_window

MIN_CHANNELS, MAX_CHANNELS = 4, 256
MAX_TAPS_PER_BRANCH = 40


def check_parameters(channels: int, oversample: int, n_taps: int) -> None:
    """The library's own rules, raised as ValueError before anything touches a device."""
    M = int(channels)
    if not MIN_CHANNELS <= M <= MAX_CHANNELS or M & (M - 1):
        raise ValueError(f"channels={channels}: a power of two, {MIN_CHANNELS} .. {MAX_CHANNELS}")
    if int(oversample) not in (1, 2):
        raise ValueError(f"oversample={oversample}: 1 or 2")
    if not 1 <= int(n_taps) <= MAX_TAPS_PER_BRANCH * M:
        raise ValueError(f"{n_taps} taps: 1 .. {MAX_TAPS_PER_BRANCH * M} ({MAX_TAPS_PER_BRANCH} per branch at {M} channels)")


def check_output(n_out: int, out_stride: int, out_ptr: int) -> None:
    """A call's output placement: channel c's run starts at out_ptr + 8 c out_stride."""
    if int(out_stride) < int(n_out):
        raise ValueError(f"out_stride={out_stride}: the call completes {n_out} outputs per channel")
    if int(out_ptr) % 8:
        raise ValueError("output pointer must be aligned to one complex64 sample")


def _complex_input(iq):
    a = np.asarray(iq)
    if not (np.iscomplexobj(a) or a.dtype in (np.int8, np.uint8)):
        raise ValueError(f"real input ({a.dtype}): the channelizer takes complex IQ (complex, or interleaved int8 / "
                         "uint8 pairs)")
    return _iq_input(a, None)


class Channelizer(nat._Handle):
    """M channels of fs / M each, decimated by D = M / oversample (complex64 out, one output per channel per D inputs)."""
    _destroy = "tdsa_chan_destroy"

    def __init__(self, channels: int, sample_rate: float, oversample: int = 1, taps=None, device: int = 0,
                 max_host_samples: int = 1 << 22):
        self.taps = None if taps is None else as_taps(taps)
        check_parameters(channels, oversample, self.taps.size if self.taps is not None else int(channels))
        self.channels = int(channels)
        self.oversample = int(oversample)
        self.decimation = self.channels // self.oversample
        self.sample_rate = float(sample_rate)
        if not self.sample_rate > 0:
            raise ValueError(f"sample_rate={sample_rate}")
        self.device = int(device)
        self.max_host_samples = int(max_host_samples)
        if self.taps is None:
            self.taps = design_decimator(self.channels)
        self._inputs = 0
        self._h = C.c_void_p()
        nat.check(nat.lib.tdsa_chan_create(self.device, self.channels, self.oversample, int(self.taps.size),
                                           self.max_host_samples, C.byref(self._h)))
        nat.check(nat.lib.tdsa_chan_set_taps(self._h, self.taps.ctypes.data_as(C.c_void_p), int(self.taps.size)))

    # ------------------------------------------------------------------ configuration
    @property
    def output_rate(self) -> float:
        """Of every channel: fs / D."""
        return self.sample_rate / self.decimation

    @property
    def branch_taps(self) -> int:
        """P = ceil(T / M)."""
        return -(-int(self.taps.size) // self.channels)

    @property
    def first_full_output(self) -> int:
        """m0 = ceil((T-1) / D): the first output whose filter window lies entirely in delivered input."""
        return -(-(int(self.taps.size) - 1) // self.decimation)

    def channel_centres(self, centre_freq: float = 0.0) -> np.ndarray:
        """[M] float64: c fs / M for c < M / 2, (c - M) fs / M from there on, plus centre_freq."""
        return np.fft.fftfreq(self.channels, 1.0 / self.sample_rate) + float(centre_freq)

    def outputs_completed_by(self, n_in: int) -> int:
        """Outputs per channel a call delivering n_in more inputs would complete."""
        return outputs_completed(self._inputs, n_in, self.decimation)

    def reset(self) -> None:
        """History to zero: inputs count from 0 again."""
        nat.check(nat.lib.tdsa_chan_reset(self._h))
        self._inputs = 0

    # ------------------------------------------------------------------ processing
    def process(self, iq, branches: bool = False) -> np.ndarray:
        """One host block (complex, or interleaved int8 / uint8 pairs): complex64 [M][n_out], the outputs it completes.
        branches=True returns the shifted branch sums W_m[p] (row p) instead: the input of a transform of the caller's."""
        a, fmt, n = _complex_input(iq)
        flags = nat.CHAN_BRANCHES if branches else 0
        outs = []
        for s in range(0, max(n, 1), self.max_host_samples):
            k = min(self.max_host_samples, n - s)
            part = a[s:s + k] if fmt == nat.IN_C64 else a[2 * s:2 * (s + k)]
            want = self.outputs_completed_by(k)
            out = np.empty((self.channels, max(want, 1)), dtype=np.complex64)
            n_out = C.c_size_t()
            nat.check(nat.lib.tdsa_chan_process(self._h, fmt, part.ctypes.data_as(C.c_void_p), k,
                                                out.ctypes.data_as(C.c_void_p), out.shape[1], flags, C.byref(n_out)))
            self._inputs += k
            outs.append(out[:, :n_out.value])
        return outs[0] if len(outs) == 1 else np.concatenate(outs, axis=1)

    def process_device(self, engine: Optional[SpectrumEngine], fmt: int, ptr: int, n_in: int, out_ptr: int,
                       out_stride: int, branches: bool = False) -> int:
        """Input and output in device memory, on `engine`'s stream (None: the handle's own), no host wait.  Channel c's
        outputs of the call go to out_ptr + 8 c out_stride.  Returns the number of outputs per channel."""
        if int(fmt) not in (nat.IN_I8, nat.IN_U8, nat.IN_C64):
            raise ValueError(f"in_format={fmt}: the channelizer takes complex IQ")
        check_output(self.outputs_completed_by(n_in), out_stride, out_ptr or 0)
        if engine is not None:
            check_same_device(engine.device, self.device)
        n_out = C.c_size_t()
        nat.check(nat.lib.tdsa_chan_process_dev(self._h, engine._h if engine is not None else None, int(fmt),
                                                C.c_void_p(ptr), int(n_in), C.c_void_p(out_ptr) if out_ptr else None,
                                                int(out_stride), nat.CHAN_BRANCHES if branches else 0, C.byref(n_out)))
        self._inputs += int(n_in)
        return int(n_out.value)


def stitch_index(channels: int, nfft: int, oversample: int) -> np.ndarray:
    """Index into a flattened [M][nfft] row (fftshift-ed channels in FFT order) that lays the central +-fs / 2M of every
    channel side by side in ascending frequency: nfft / oversample bins per channel, from the channel centred at
    -fs / 2 upwards."""
    M, n, keep = int(channels), int(nfft), int(nfft) // int(oversample)
    order = (np.arange(M) + M // 2) % M
    k = np.arange(n // 2 - keep // 2, n // 2 - keep // 2 + keep)
    return (order[:, None] * n + k[None, :]).reshape(-1)


class ChannelSpectra(nat._Handle):
    """Spectra of all M channels at RBW fs os / (M nfft).  Frame f of channel c is y_c[f nfft : (f + 1) nfft]: frames
    start at output 0, hop = nfft, so the first branch_taps - 1 outputs of every channel's first frame carry the filter's
    fill.  A call takes a whole number F of frames per channel, a block of F D nfft inputs.

    `.engine` is the SpectrumEngine the rows come from.  DC removal is off (a channel's DC is the signal at its centre),
    and averaging and holds stay off: one plan's per-bin state would mix the channels."""

    def __init__(self, sample_rate: float, channels: int, nfft: int, oversample: int = 2, taps=None, window=None,
                 device: int = 0, max_frames: int = 8):
        self.nfft = int(nfft)
        self.max_frames = int(max_frames)           # per channel and call
        if self.max_frames < 1:
            raise ValueError(f"max_frames={max_frames}")
        self.device = int(device)
        check_parameters(channels, oversample, int(channels) if taps is None else np.asarray(taps).size)
        D = int(channels) // int(oversample)
        self._max_in = self.max_frames * D * self.nfft
        self.bank = Channelizer(channels, sample_rate, oversample, taps, device, max_host_samples=self._max_in)
        self.engine = SpectrumEngine(self.nfft, max_frames=self.channels * self.max_frames, device=self.device)
        self.engine.set_window(zoom_window(self.nfft) if window is None else window)
        self.engine.configure(db_mode="mag", log_floor=DSPConstants.LOG_FLOOR, dc_alpha=-1.0)
        self._d_in = DeviceBuffer(8 * self._max_in, self.device)
        self._d_y = DeviceBuffer(8 * self.channels * self.max_frames * self.nfft, self.device)
        self._d_rows = DeviceBuffer(4 * self.channels * self.max_frames * self.nfft, self.device)

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        nat._close_all(self, "_d_in", "_d_y", "_d_rows", "bank", "engine", wait="engine")

    # ------------------------------------------------------------------ axis
    @property
    def channels(self) -> int:
        return self.bank.channels

    @property
    def oversample(self) -> int:
        return self.bank.oversample

    @property
    def decimation(self) -> int:
        return self.bank.decimation

    @property
    def sample_rate(self) -> float:
        return self.bank.sample_rate

    @property
    def rbw(self) -> float:
        return self.sample_rate / (self.decimation * self.nfft)

    @property
    def block_samples(self) -> int:
        """Inputs per frame of every channel: a call takes a multiple of it."""
        return self.decimation * self.nfft

    def freq_bins(self, centre_freq: float = 0.0) -> np.ndarray:
        """[M][nfft] float64: the axis of every channel's rows."""
        fb = np.fft.fftshift(np.fft.fftfreq(self.nfft, self.decimation / self.sample_rate))
        return self.bank.channel_centres(centre_freq)[:, None] + fb[None, :]

    def stitch_index(self) -> np.ndarray:
        """rows[:, f, :].reshape(-1)[stitch_index()] is frame f's row of the whole capture, ascending in frequency, and
        freq_bins().reshape(-1)[stitch_index()] its axis: at oversample = 2 a seamless M nfft / 2 bins."""
        return stitch_index(self.channels, self.nfft, self.oversample)

    def reset(self) -> None:
        self.engine.synchronize()
        self.bank.reset()

    # ------------------------------------------------------------------ processing
    def frames_of(self, n_in: int) -> int:
        """Frames per channel of a block of n_in inputs; ValueError unless it is a whole number within max_frames."""
        n_in = int(n_in)
        if n_in < 0 or n_in % self.block_samples:
            raise ValueError(f"block of {n_in} samples: a multiple of D nfft = {self.block_samples}")
        F = n_in // self.block_samples
        if F > self.max_frames:
            raise ValueError(f"block of {F} frames per channel: at most max_frames = {self.max_frames}")
        return F

    def _run(self, fmt: int, ptr: int, n_in: int, rows_ptr: int) -> int:
        """The bank into [M][F][nfft] complex64, then its M F frames in one frame-kernel launch."""
        F = self.frames_of(n_in)
        if F == 0:
            return 0
        d_y = self._d_y.at(0, 8 * self.channels * F * self.nfft)
        n_out = self.bank.process_device(self.engine, fmt, ptr, n_in, d_y, F * self.nfft)
        assert n_out == F * self.nfft
        self.engine.process_device(nat.IN_C64, d_y, self.channels * F * self.nfft, self.nfft, self.channels * F, rows_ptr)
        return F

    def process(self, iq) -> np.ndarray:
        """Host IQ in (complex, or interleaved int8 / uint8 pairs), F D nfft samples: float32 dB rows [M][F][nfft]."""
        a, fmt, n = _complex_input(iq)
        F = self.frames_of(n)
        out = np.empty((self.channels, F, self.nfft), dtype=np.float32)
        if F == 0:
            return out
        bps = 8 if fmt == nat.IN_C64 else 2
        nat.check(nat.lib.tdsa_plan_copy(self.engine._h, self._d_in.at(0, bps * n), a.ctypes.data_as(C.c_void_p),
                                         bps * n, 0))
        self._run(fmt, self._d_in.ptr, n, self._d_rows.ptr)
        nat.check(nat.lib.tdsa_plan_copy(self.engine._h, out.ctypes.data_as(C.c_void_p), self._d_rows.at(0, out.nbytes),
                                         out.nbytes, 1))
        return out

    def process_device(self, fmt: int, ptr: int, n_in: int, out_db_dev: int) -> int:
        """Raw IQ already on the device (ptr, n_in = F D nfft samples): dB rows [M][F][nfft] to out_db_dev, asynchronous
        on the engine's stream.  Returns F."""
        return self._run(int(fmt), int(ptr), int(n_in), int(out_db_dev))
