"""The channelizer without a GPU: the float64 restatement (branch sums, shift, inverse DFT) against the defining sum
and against zoom_contract's down-converter, the default prototype's response, the stitching index, and the argument
errors, which the library and the Python layer report before any device call."""
import ctypes as C

import numpy as np
import pytest

import chan_contract as cc
import zoom_contract as zc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import channelizer as ch
from topdogspectrumanalyser_amd.zoom import design_decimator


def _stream(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("os_", [1, 2])
@pytest.mark.parametrize("M", [4, 8, 64])
def test_restatement_equals_the_direct_sum_and_the_down_converter(M, os_):
    """T is no multiple of M; every channel; both sides float64: 1e-9 max |y|."""
    rng = np.random.default_rng(100 * M + os_)
    D = M // os_
    T = 5 * M - 3
    h = rng.standard_normal(T).astype(np.float32)
    n = 37 * D + D // 2 + 1
    x = _stream(rng, n)
    got = cc.restated(x, h, M, os_)
    ref = cc.direct(x, h, M, os_)
    assert got.shape == ref.shape == (M, zc.n_outputs(n, D))
    tol = 1e-9 * np.abs(ref).max()
    assert np.abs(got - ref).max() <= tol
    for c in range(M):
        step = c * (1 << 32) // M
        assert step * M == c << 32                               # an integer phase step
        y = zc.reference(x, zc.FMT_C64, h, D, [(0, step)])
        assert np.abs(got[c] - y).max() <= tol, c


@pytest.mark.parametrize("os_", [1, 2])
def test_restatement_is_the_same_for_blocks_split_at_odd_points(os_):
    """Output m belongs to the call that delivers input m D: the outputs of the pieces, laid end to end, are the
    outputs of the whole, and a piece's count follows from the inputs before it."""
    M, D = 8, 8 // os_
    rng = np.random.default_rng(5)
    h = rng.standard_normal(3 * M + 1).astype(np.float32)
    x = _stream(rng, 29 * D + 3)
    whole = cc.restated(x, h, M, os_)
    cuts = [0, 1, D - 1, D + 2, 7 * D, 7 * D + 1, 19 * D + D // 2, len(x)]
    done = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        k = ch.outputs_completed(a, b - a, D)
        part = cc.restated(x[:b], h, M, os_)[:, done:done + k]
        assert part.shape[1] == k
        if k == 0:                                  # a piece shorter than D may complete nothing
            continue
        assert np.abs(part - whole[:, done:done + k]).max() <= 1e-9 * np.abs(whole).max()
        done += k
    assert done == whole.shape[1]


@pytest.mark.parametrize("M", [8, 64, 256])
def test_default_prototype_response(M):
    """>= 100 dB down beyond 0.6 fs / M, -6.0 +- 0.1 dB at the channel edge fs / 2M; within the tap limit."""
    h = design_decimator(M).astype(np.float64)
    ch.check_parameters(M, 2, h.size)
    k = np.arange(h.size)
    edge = 20 * np.log10(abs(np.sum(h * np.exp(-2j * np.pi * k * 0.5 / M))))
    assert abs(edge + 6.0) <= 0.1, edge
    N = 1 << int(np.ceil(np.log2(h.size * 32)))
    H = np.abs(np.fft.fft(h, N))
    f = np.arange(N) / N
    stop = (f >= 0.6 / M) & (f <= 1 - 0.6 / M)
    assert 20 * np.log10(H[stop].max()) <= -100.0


@pytest.mark.parametrize("M,nfft", [(4, 8), (16, 256), (64, 1024)])
def test_stitch_index_is_ascending_and_seamless(M, nfft):
    fs = 20e6
    for os_ in (1, 2):
        D = M // os_
        centres = np.fft.fftfreq(M, 1.0 / fs)
        assert centres[1] == fs / M and centres[M // 2] == -fs / 2 and centres[M - 1] == -fs / M
        axis = (centres[:, None] + np.fft.fftshift(np.fft.fftfreq(nfft, D / fs))[None, :]).reshape(-1)
        idx = ch.stitch_index(M, nfft, os_)
        assert idx.dtype.kind == "i" and idx.size == M * nfft // os_ and np.unique(idx).size == idx.size
        f = axis[idx]
        rbw = fs * os_ / (M * nfft)
        assert np.all(np.diff(f) > 0)
        assert np.allclose(np.diff(f), rbw, rtol=0, atol=1e-6 * rbw)         # no gap, no overlap
        assert abs(f[0] - (-fs / 2 - fs / (2 * M))) <= 1e-6 * rbw             # from the channel centred at -fs / 2
        assert abs((f[-1] + rbw - f[0]) - fs) <= 1e-6 * rbw                   # exactly the capture
        # every kept bin lies within +-fs / 2M of its channel's centre
        own = np.repeat(centres, nfft)[idx]
        assert np.all(np.abs(f - own) <= fs / (2 * M) + 1e-6 * rbw)


def test_argument_errors_without_a_device():
    h, n = C.c_void_p(), C.c_size_t()
    bad_create = [(3, 1, 8), (2, 1, 8), (512, 1, 8), (24, 1, 8),        # M: not a power of two, out of range
                  (8, 0, 8), (8, 3, 8), (8, 4, 8),                       # os
                  (8, 1, 0), (8, 1, 8 * ch.MAX_TAPS_PER_BRANCH + 1)]    # T
    for M, os_, T in bad_create:
        assert nat.lib.tdsa_chan_create(0, M, os_, T, 1024, C.byref(h)) == -1, (M, os_, T)
        assert not h.value
        with pytest.raises(ValueError):
            ch.check_parameters(M, os_, T)
        with pytest.raises(ValueError):
            ch.Channelizer(M, 20e6, os_, taps=np.ones(max(T, 1) if T else 0, np.float32))
    with pytest.raises(ValueError):
        ch.ChannelSpectra(20e6, 12, 256)
    # real input formats
    assert nat.lib.tdsa_chan_process(None, nat.IN_F32R, None, 0, None, 0, 0, C.byref(n)) == -1
    assert b"complex IQ" in nat.lib.tdsa_last_error_string()
    assert nat.lib.tdsa_chan_process_dev(None, None, nat.IN_F32R, None, 0, None, 0, 0, C.byref(n)) == -1
    with pytest.raises(ValueError):
        ch._complex_input(np.zeros(16, np.float32))
    # a misaligned output pointer
    assert nat.lib.tdsa_chan_process_dev(None, None, nat.IN_C64, None, 0, C.c_void_p(4100), 0, 0, C.byref(n)) == -1
    assert b"aligned" in nat.lib.tdsa_last_error_string()
    with pytest.raises(ValueError):
        ch.check_output(4, 4, 4100)
    # out_stride smaller than the call's n_out: 10 inputs after 3 at D = 4 complete outputs 1, 2, 3
    assert ch.outputs_completed(3, 10, 4) == 3 and ch.outputs_completed(0, 1, 4) == 1 and ch.outputs_completed(1, 3, 4) == 0
    with pytest.raises(ValueError):
        ch.check_output(3, 2, 4096)
    ch.check_output(3, 3, 4096)
    # plan and handle on different devices
    with pytest.raises(ValueError):
        ch.check_same_device(1, 0)
    # null handles and null counts are argument errors too
    assert nat.lib.tdsa_chan_process(None, nat.IN_I8, None, 0, None, 0, 0, C.byref(n)) == -1
    assert nat.lib.tdsa_chan_set_taps(None, None, 1) == -1 and nat.lib.tdsa_chan_reset(None) == -1
    assert nat.lib.tdsa_chan_destroy(None) == 0
