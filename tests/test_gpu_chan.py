"""The polyphase channelizer on the MI355X, pinned against something other than the kernel:
exact integer branch sums and exact channels bit for bit, the float64 contract under a derived rounding allowance,
split invariance, streams past 2^31 and 2^32 inputs, tdsa_chan_set_taps on a handle that has streamed, host blocks above
max_host_samples, the channel-major layout, ChannelSpectra against the engine run channel by channel, and the handle's
launch order across streams.

Shapes: M in {4, 16, 64, 256} x os in {1, 2} x P in {1, 3, 32} taps per branch, plus one T = 3M - 5: less than a wave,
one wave and several waves per output instant, and a partly filled last phase; M in {8, 32, 128} x os in {1, 2} x
P in {1, 9} - the other thread-group counts, both staging pads and the row skew of 2, one tap and a full register block
followed by a partial one - P = 8, exactly one block, 17 branch taps with a partly filled last phase, and the tap limit
P = 40 at M = 4, 128 and 256 (the last is the largest LDS request the launcher makes).  A workgroup owns 2048 / M output
instants; every case is three such tiles plus a ragged remainder.

The allowance of test 3, per output instant in the 2-norm over channels, with u = 2^-24:
    ||y^_m - y_m||_2 <= u ((P + 1) sqrt(M) ||a_m||_2 + 7 log2(M) ||y_m||_2),  a_m[r] = sum_q |h[qM + r]| |x[mD - qM - r]|
- an fma chain's gamma_{P+1} through a transform of norm sqrt(M), plus Higham's bound for a radix-2 FFT whose twiddles
are correct to u (eta = u (1 + 4 sqrt 2) per stage, rounded up to 7 u).  The test prints the worst ratio it meets."""
import ctypes as C
import functools

import numpy as np
import pytest

import chan_contract as cc
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, ZeroSpan, _native as nat
from topdogspectrumanalyser_amd.channelizer import Channelizer, ChannelSpectra
from topdogspectrumanalyser_amd.utils.constants import DSPConstants
from topdogspectrumanalyser_amd.zoom import design_decimator, zoom_window

pytestmark = pytest.mark.gpu

FS = 20e6
U = 2.0 ** -24
TILE = 2048
SHAPES = [(M, os_, P * M) for M in (4, 16, 64, 256) for os_ in (1, 2) for P in (1, 3, 32)] + [(16, 2, 3 * 16 - 5)]
SHAPES += [(M, os_, P * M) for M in (8, 32, 128) for os_ in (1, 2) for P in (1, 9)]
SHAPES += [(8, 1, 8 * 8), (32, 2, 17 * 32 - 3), (4, 2, 40 * 4), (128, 2, 40 * 128), (256, 1, 40 * 256)]
IDS = [f"M{M}-os{o}-T{T}" for M, o, T in SHAPES]


def _n_in(M, os_):
    """Three tiles of outputs and a ragged remainder, ending between two outputs."""
    D, F = M // os_, TILE // M
    n_out = 3 * F + max(1, F // 3)
    return (n_out - 1) * D + 1 + D // 3, n_out


def _raw(rng, n, fmt):
    if fmt == cc.FMT_I8:
        return rng.integers(-128, 128, 2 * n).astype(np.int8)
    if fmt == cc.FMT_U8:
        return rng.integers(0, 256, 2 * n).astype(np.uint8)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)


def _bits(y):
    return np.ascontiguousarray(y, dtype=np.complex64).view(np.uint64)


# ---- 1 and 2: integer data, every sum an exact float32 ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_case(M, os_, T):
    """int8 IQ, integer taps |h| <= 8, and the exact branch sums (int64, in units of 2^-7)."""
    rng = np.random.default_rng(1000 * M + 10 * T + os_)
    n, n_out = _n_in(M, os_)
    raw = _raw(rng, n, cc.FMT_I8)
    h = rng.integers(-8, 9, T).astype(np.float32)
    h[h == 0] = 3.0
    Wr, Wi = cc.integer_branches(raw[0::2], raw[1::2], h, M, os_)
    assert Wr.shape == (M, n_out)
    for a in (raw, h, Wr, Wi):
        a.setflags(write=False)
    return raw, h, Wr, Wi


def _as_c64(re, im):
    """int64 sums in units of 2^-7 as the complex64 they are exactly."""
    assert max(np.abs(re).max(), np.abs(im).max()) < 1 << 24
    return (re.astype(np.float32) * np.float32(2.0 ** -7) + 1j * (im.astype(np.float32) * np.float32(2.0 ** -7))).astype(np.complex64)


@pytest.mark.parametrize("M,os_,T", SHAPES, ids=IDS)
def test_first_stage_bit_for_bit(M, os_, T):
    raw, h, Wr, Wi = _integer_case(M, os_, T)
    want = _as_c64(Wr, Wi)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=raw.size // 2) as bank:
        got = bank.process(raw, branches=True)
        assert got.shape == want.shape and got.dtype == np.complex64
        assert np.array_equal(got, want)
        bank.reset()
        got64 = bank.process(cc.unpack(raw, cc.FMT_I8), branches=True)       # complex64 of the same values
        assert np.array_equal(_bits(got64), _bits(got))


@pytest.mark.parametrize("M,os_,T", SHAPES, ids=IDS)
def test_exact_channels(M, os_, T):
    """Channels 0 and M / 2 see only twiddles +-1 (every channel at M = 4 only +-1 and +-j): exact for integer data."""
    raw, h, Wr, Wi = _integer_case(M, os_, T)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=raw.size // 2) as bank:
        got = bank.process(raw)
    assert got.shape == Wr.shape
    for c in (range(4) if M == 4 else (0, M // 2)):
        want = _as_c64(*cc.integer_channel(Wr, Wi, c))
        assert np.array_equal(got[c], want), c


# ---- 3: float data against the float64 contract ----------------------------------------------------------------------
def _float_taps(M, T):
    P = cc.branch_taps(T, M)
    return np.ascontiguousarray(design_decimator(M, taps_per_phase=P)[:T])


def _check_allowance(got, x, h, M, os_, what):
    return _check_against(got, cc.restated(x, h, M, os_), cc.abs_branches(x, h, M, os_), len(h), what)


def _check_against(got, ref, a, T, what):
    """got and ref [M][n_out], a [n_out][M] the absolute branch sums: the allowance of the module's docstring."""
    M = ref.shape[0]
    P = cc.branch_taps(T, M)
    assert got.shape == ref.shape
    err = np.linalg.norm(got.astype(np.complex128) - ref, axis=0)
    bound = U * ((P + 1) * np.sqrt(M) * np.linalg.norm(a, axis=1) + 7 * np.log2(M) * np.linalg.norm(ref, axis=0))
    ok = bound > 0                                                      # an instant that has seen only zeros is exact
    assert np.all(err[~ok] == 0)
    ratio = float(np.max(err[ok] / bound[ok]))
    print(f"{what}: worst error / allowance {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.parametrize("M,os_,T", SHAPES + [(64, 1, 34 * 64), (64, 2, 34 * 64)], ids=IDS + ["M64-os1-default", "M64-os2-default"])
def test_against_the_float64_contract(M, os_, T):
    rng = np.random.default_rng(7000 + 100 * M + T + os_)
    n, n_out = _n_in(M, os_)
    h = _float_taps(M, T)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n) as bank:
        for fmt, name in ((cc.FMT_I8, "int8"), (cc.FMT_U8, "uint8"), (cc.FMT_C64, "complex64")):
            raw = _raw(rng, n, fmt)
            bank.reset()
            got = bank.process(raw)
            assert got.shape == (M, n_out)
            _check_allowance(got, cc.unpack(raw, fmt), h, M, os_, f"M={M} os={os_} T={T} {name}")


# ---- 4: any split of the input gives the same bits -------------------------------------------------------------------
def _device_run(bank, raw, fmt, pieces, n_out, engine=None):
    """The block piece by piece through process_device, every piece's outputs behind those before it."""
    bps = 8 if fmt == cc.FMT_C64 else 2
    with DeviceBuffer.of(raw) as d_in, DeviceBuffer(8 * bank.channels * n_out) as d_out:
        got = at = 0
        for k in pieces:
            got += bank.process_device(engine, fmt, d_in.at(bps * at, bps * k), k, d_out.at(8 * got), n_out)
            at += k
        bank.reset()                                    # waits for the handle's work
        assert got == n_out
        return d_out.get(bank.channels * n_out, np.complex64).reshape(bank.channels, n_out)


def _pieces(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


@pytest.mark.parametrize("M,os_,T", [(4, 2, 11), (16, 1, 3 * 16), (64, 2, 32 * 64), (256, 1, 3 * 256 - 5),
                                     (32, 2, 9 * 32), (128, 1, 3 * 128 - 5)],
                         ids=["M4-os2", "M16-os1", "M64-os2", "M256-os1", "M32-os2", "M128-os1"])
def test_split_invariance(M, os_, T):
    rng = np.random.default_rng(31 * M + os_)
    D = M // os_
    n, n_out = _n_in(M, os_)
    h = _float_taps(M, T)
    raw = _raw(rng, n, cc.FMT_U8)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n) as bank:
        one = bank.process(raw)
        assert one.shape == (M, n_out)
        bank.reset()
        assert np.array_equal(_bits(bank.process(raw)), _bits(one))                      # reset reproduces the run
        bank.reset()
        assert np.array_equal(_bits(bank.process(cc.unpack(raw, cc.FMT_U8))), _bits(one))   # uint8 = its unpack
        bank.reset()
        host_parts = [bank.process(raw[2 * a:2 * b]) for a, b in ((0, 1), (1, D + 2), (D + 2, n // 2), (n // 2, n))]
        assert np.array_equal(_bits(np.concatenate(host_parts, axis=1)), _bits(one))
        bank.reset()
        prime = 13 if D != 13 else 17
        for size in (n, 1, D - 1, D, D + 1, prime):                                       # size n: host = device entry
            if size < 1:
                continue
            got = _device_run(bank, raw, cc.FMT_U8, _pieces(n, size), n_out)
            assert np.array_equal(_bits(got), _bits(one)), size
        # pieces shorter than D that complete nothing, between longer ones
        mixed, left = [], n
        for k in [1, D - 1, 1, 1, 3 * D + 1, D - 1, prime]:
            if 0 < k <= left:
                mixed.append(k)
                left -= k
        got = _device_run(bank, raw, cc.FMT_U8, mixed + [left], n_out)
        assert np.array_equal(_bits(got), _bits(one))


# ---- 4b: past 2^31 and 2^32 inputs -----------------------------------------------------------------------------------
LONG_BLOCK = 1 << 24


@functools.lru_cache(maxsize=None)
def _long_block():
    raw = np.random.default_rng(2 ** 32 + 12).integers(-128, 128, 2 * LONG_BLOCK).astype(np.int8)
    raw.setflags(write=False)
    return raw


@pytest.mark.parametrize("M,os_", [(4, 2), (256, 1)], ids=["M4-os2", "M256-os1"])
def test_streams_past_2_32_inputs(M, os_):
    """A block of 2^24 int8 samples replayed 257 times with the default prototype: x[n] = block[n mod 2^24].  Checked
    against the float64 defining sum, regrouped by branch (exp(-2 pi j c n / M) has period M in n) with every index in
    int64, under the allowance of test 3: all M channels of the first and last 160 instants of the calls that end at
    2^31 and 2^32 inputs and of the calls that begin there (the first ones read the history); the call that begins at
    2^32 is the last.  At M = 4, os = 2 the output index itself passes 2^31, with the half-turn shift of odd
    instants."""
    reps, nb, keep = 257, LONG_BLOCK, 160
    D = M // os_
    raw = _long_block()
    checked = (127, 128, 255, 256)
    cap = nb // D + 2
    with Channelizer(M, FS, os_, max_host_samples=64) as bank, DeviceBuffer.of(raw) as d_in, \
            DeviceBuffer(8 * M * cap * (1 + len(checked))) as d_y:
        h = bank.taps
        total, spans = 0, []
        for i in range(reps):                               # every other call overwrites slot 0
            slot = 1 + checked.index(i) if i in checked else 0
            k = bank.process_device(None, cc.FMT_I8, d_in.ptr, nb, d_y.at(8 * M * cap * slot), cap)
            assert k <= cap
            if slot:
                spans.append((total, k, slot))
            total += k
        bank.reset()                                        # waits for the handle's stream
        assert total == -(-(reps * nb) // D)
        got, ms = [], []
        for m0, k, slot in spans:
            for a in (0, k - keep):
                got.append(np.stack([d_y.get(keep, np.complex64, 8 * ((M * slot + c) * cap + a)) for c in range(M)]))
                ms.append(m0 + a + np.arange(keep, dtype=np.int64))
    got, ms = np.concatenate(got, axis=1), np.concatenate(ms)
    assert ms.min() * D < 1 << 31 < ms.max() * D and np.any(ms * D > 1 << 32)
    assert os_ == 1 or (ms.max() > 1 << 31 and np.any(ms & 1) and not np.all(ms & 1))
    T, PM = h.size, cc.branch_taps(h.size, M) * M
    hp = np.zeros(PM)
    hp[:T] = h
    idx = ms[:, None] * D - np.arange(PM, dtype=np.int64)[None, :]
    assert idx.min() > 0 and idx.max() > 1 << 32
    j = idx % nb
    x = (raw[2 * j].astype(np.float64) + 1j * raw[2 * j + 1].astype(np.float64)) / 128.0
    w = (x * hp).reshape(ms.size, -1, M).sum(axis=1)                   # w_m[r], [n][M]
    a = (np.abs(x) * np.abs(hp)).reshape(ms.size, -1, M).sum(axis=1)
    p = (np.arange(M, dtype=np.int64)[None, :] - ms[:, None] * D) % M  # W_m[p] at p = (r - mD) mod M
    W = np.empty_like(w)
    np.put_along_axis(W, p, w, axis=1)
    _check_against(got, cc.transform(W.T), a, T, f"past 2^32 M={M} os={os_}: {ms.size} instants")


# ---- 4c: entry points: taps on a live handle, host blocks above max_host_samples ---------------------------------------
def _set_taps(bank, h):
    h = np.ascontiguousarray(h, dtype=np.float32)
    nat.check(nat.lib.tdsa_chan_set_taps(bank._h, h.ctypes.data_as(C.c_void_p), int(h.size)))
    bank.taps, bank._inputs = h, 0


def test_set_taps_on_a_handle_that_has_streamed():
    """A shorter prototype shortens P inside tap and history buffers sized for the handle's max_taps (40 rows, 3 in
    use); afterwards the handle must behave as a fresh one with those taps: history cleared, inputs counted from 0."""
    M, os_ = 32, 2
    D = M // os_
    rng = np.random.default_rng(78)
    long_h = (rng.standard_normal(40 * M) / M).astype(np.float32)
    short_h = (rng.standard_normal(3 * M - 5) / M).astype(np.float32)
    n, n_out = _n_in(M, os_)
    first = _raw(rng, n + 5 * D + 3, cc.FMT_I8)
    later = _raw(rng, n, cc.FMT_I8)
    cut = (n // 2) | 1                                    # the second call starts between two outputs

    def run(bank):
        return np.concatenate([bank.process(later[:2 * cut]), bank.process(later[2 * cut:])], axis=1)

    def fresh(h):
        with Channelizer(M, FS, os_, taps=h, max_host_samples=first.size // 2) as bank:
            return run(bank)

    with Channelizer(M, FS, os_, taps=long_h, max_host_samples=first.size // 2) as bank:
        bank.process(first)
        _set_taps(bank, short_h)
        y_short = run(bank)
        _set_taps(bank, long_h)
        y_long = run(bank)
    assert y_short.shape == y_long.shape == (M, n_out)
    assert np.array_equal(_bits(y_short), _bits(fresh(short_h)))
    assert np.array_equal(_bits(y_long), _bits(fresh(long_h)))


@pytest.mark.parametrize("fmt", [cc.FMT_I8, cc.FMT_C64], ids=["int8", "complex64"])
def test_host_block_larger_than_max_host_samples(fmt):
    """process() cuts a block above max_host_samples into several library calls: the bits of the single call."""
    M, os_ = 16, 2
    rng = np.random.default_rng(79)
    n, n_out = _n_in(M, os_)
    raw = _raw(rng, n, fmt)
    h = _float_taps(M, 3 * M - 5)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n) as bank:
        one = bank.process(raw)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n // 3 + 1) as bank:
        assert bank.max_host_samples < n < 3 * bank.max_host_samples
        got = bank.process(raw)
        assert got.shape == one.shape == (M, n_out) and np.array_equal(_bits(got), _bits(one))
        bank.reset()
        W = bank.process(raw, branches=True)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n) as bank:
        assert np.array_equal(_bits(W), _bits(bank.process(raw, branches=True)))


# ---- 5: layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branches", [False, True])
def test_stride_leaves_the_gaps_alone(branches):
    M, os_ = 16, 2
    rng = np.random.default_rng(55)
    n, n_out = _n_in(M, os_)
    stride = n_out + 5
    raw = _raw(rng, n, cc.FMT_I8)
    sentinel = np.complex64(complex(-12345.5, 54321.25))
    with Channelizer(M, FS, os_, taps=_float_taps(M, 3 * M), max_host_samples=n) as bank:
        want = bank.process(raw, branches=branches)
        bank.reset()
        host = np.full((M + 1, stride), sentinel, dtype=np.complex64)
        cnt = C.c_size_t()
        nat.check(nat.lib.tdsa_chan_process(bank._h, cc.FMT_I8, raw.ctypes.data_as(C.c_void_p), n,
                                            host.ctypes.data_as(C.c_void_p), stride, int(branches), C.byref(cnt)))
        assert cnt.value == n_out
        bank.reset()
        with DeviceBuffer.of(raw) as d_in, DeviceBuffer.of(np.full((M + 1, stride), sentinel, dtype=np.complex64)) as d_out:
            assert bank.process_device(None, cc.FMT_I8, d_in.ptr, n, d_out.ptr, stride, branches) == n_out
            bank.reset()
            dev = d_out.get((M + 1) * stride, np.complex64).reshape(M + 1, stride)
    for got in (host, dev):
        assert np.array_equal(_bits(got[:M, :n_out]), _bits(want))
        assert np.all(_bits(got[:M, n_out:]) == _bits(sentinel)) and np.all(_bits(got[M]) == _bits(sentinel))


# ---- 6: ChannelSpectra -----------------------------------------------------------------------------------------------
def _spectra_rows_are_the_engine(M, os_):
    nfft = 256
    D = M // os_
    rng = np.random.default_rng(66)
    blocks = [_raw(rng, F * D * nfft, cc.FMT_I8) for F in (2, 3)]
    with ChannelSpectra(FS, M, nfft, oversample=os_, max_frames=3) as cs:
        rows = [cs.process(b) for b in blocks]
        assert [r.shape for r in rows] == [(M, 2, nfft), (M, 3, nfft)] and rows[0].dtype == np.float32
        with pytest.raises(ValueError):
            cs.process(blocks[0][:-2])                       # not a multiple of D nfft
        with pytest.raises(ValueError):
            cs.process(np.zeros(D * nfft, np.float32))       # real input
        with Channelizer(M, FS, os_, max_host_samples=3 * D * nfft) as bank, \
                SpectrumEngine(nfft, max_frames=3) as eng, DeviceBuffer(4 * 3 * nfft) as d_rows:
            eng.set_window(zoom_window(nfft))
            eng.configure(db_mode="mag", log_floor=DSPConstants.LOG_FLOOR, dc_alpha=-1.0)
            for b, got in zip(blocks, rows):
                F = got.shape[1]
                y = bank.process(b)
                assert y.shape == (M, F * nfft)
                with DeviceBuffer.of(y) as d_y:
                    for c in range(M):
                        eng.process_device(nat.IN_C64, d_y.at(8 * c * F * nfft, 8 * F * nfft), F * nfft, nfft, F, d_rows.ptr)
                        eng.synchronize()
                        want = d_rows.get(F * nfft, np.float32).reshape(F, nfft)
                        assert np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), c


def test_channel_spectra_rows_are_the_engine_on_every_channel():
    _spectra_rows_are_the_engine(16, 2)


def test_channel_spectra_rows_without_oversampling_at_8_channels():
    _spectra_rows_are_the_engine(8, 1)


def test_channel_spectra_finds_a_tone_in_the_stitched_row():
    M, os_, nfft = 16, 2, 256
    D = M // os_
    f0 = 3.25 * FS / M
    n = 3 * D * nfft
    x = (0.5 * np.exp(2j * np.pi * f0 / FS * np.arange(n))).astype(np.complex64)
    with ChannelSpectra(FS, M, nfft, oversample=os_, max_frames=3) as cs:
        rows = cs.process(x)
        fb, idx = cs.freq_bins(), cs.stitch_index()
        assert fb.shape == (M, nfft) and idx.size == M * nfft // 2
        axis = fb.reshape(-1)[idx]
        assert np.all(np.diff(axis) > 0)
        row = rows[:, 2, :].reshape(-1)[idx]                 # the last frame: past the filter's fill
        k = int(np.argmax(row))
        assert abs(axis[k] - f0) <= 0.5 * cs.rbw + 1e-6, (axis[k], f0)
        assert k == int(np.argmin(np.abs(axis - f0)))
        assert row[k] - np.median(row) > 80.0                # the aliases of the tone stay far below it


# ---- 7: the handle's launches are ordered whichever stream each goes on ----------------------------------------------
PIECES = 6


def _order_run(streams):
    M, os_ = 8, 2
    rng = np.random.default_rng(77)
    x = _raw(rng, 10 * PIECES, cc.FMT_C64)
    h = _float_taps(M, 3 * M)
    with Channelizer(M, 64.0 * M, os_, taps=h, max_host_samples=64) as bank:
        n_out = bank.outputs_completed_by(x.size)
        with DeviceBuffer.of(x) as d_in, DeviceBuffer(8 * M * n_out) as d_out:
            got = 0
            for i, eng in enumerate(streams):
                got += bank.process_device(eng, cc.FMT_C64, d_in.at(8 * 10 * i, 8 * 10), 10, d_out.at(8 * got), n_out)
            assert got == n_out
            if streams[-1] is None:
                bank.reset()                # the reference run: wait for the bank, the consumer has a stream of its own
            # a consumer on the last producer's stream, behind the bank's work there: zero span of channel 1
            with ZeroSpan(64.0, detector="mag", buffer_s=1.0, max_host_samples=64) as zs:
                assert zs.push_device(streams[-1], nat.IN_C64, d_out.at(8 * n_out, 8 * n_out), n_out) == n_out
                view = zs.view("free_run", n_display=n_out)
            bank.reset()
            y = d_out.get(M * n_out, np.complex64).reshape(M, n_out)
    return y, np.asarray(view.samples), view.total


def test_hopping_streams_and_a_consumer_behind_the_producer():
    with SpectrumEngine(64) as a, SpectrumEngine(64) as b:
        hop = [(a, None, b)[i % 3] for i in range(PIECES)]
        hop[-1] = a
        y, seen, total = _order_run(hop)
        y1, seen1, total1 = _order_run([None] * PIECES)
    assert np.array_equal(_bits(y), _bits(y1))
    n_out = y.shape[1]
    assert total == total1 == n_out
    assert seen.shape == (n_out,) and np.array_equal(seen, seen1)
    assert np.allclose(seen, np.abs(y[1]), rtol=1e-5, atol=0)          # what the bank wrote, not what was there before
