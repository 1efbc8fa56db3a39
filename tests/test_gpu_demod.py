"""The analog demodulator on the MI355X, pinned against something other than the kernels:
exact integer data bit for bit, the float64 contract under derived rounding allowances, split invariance, streams past
2^31 and 2^32 inputs, tdsa_demod_set_taps on a handle that has streamed, host blocks above max_host_samples, the layout,
the measurements, and the chain channelizer -> demodulator on one stream.

Shapes (R, T): (1, 1), (1, 7), (3, 8), (8, 272), (64, 64), (64, 4096) - no filter, fewer residues than lanes, a residue
group that is partly filled, 34 phases, one phase of 8 residue groups, and the largest filter - and (2, 18), (5, 37),
(12, 96), (16, 16), (20, 53), (63, 4032): 9 phases (a register block and one tap), a ragged T, two residue groups with
the second half filled at exactly 8 phases, two and three groups, and eight groups with the last one lane short at the
largest Q; both modes, 1 and 3 channels.  A workgroup owns kDemodTile = 256 outputs: every case is three tiles plus a ragged remainder of 85, ends
between two outputs (R > 1) and inside a pole block (853 = 13 * 64 + 21).

Allowances of test 2, u = 2^-24, A_d the measured worst discriminator error of demod_contract (in u):
    discriminator alone  |d^ - d| <= 2 A_d u                       (FM, half turns; AM: times |d|, its error is relative)
    with the filter      |a^ - a| <= u ((T + 1) sum |g||d| + 2 A_d sum |g|)       (AM: 2 A_d sum |g||d|)
    with the pole        + (B + 3) u max|a| (1 + 1 / (1 - c^B))
The device executes the roundings the host sweep measured, the factor 2 covers the points the sweep did not sample; an
fma chain of T terms has gamma_{T+1}; a block of the pole section is a chain of up to B + 1 terms and the carry's error
is summed over the blocks with ratio c^B.  The test prints the worst ratio of error to allowance per stage."""
import ctypes as C
import functools

import numpy as np
import pytest

import demod_contract as dc
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat
from topdogspectrumanalyser_amd.channelizer import Channelizer
from topdogspectrumanalyser_amd.demod import Demodulator, derive, design_audio_filter
from topdogspectrumanalyser_amd.zoom import design_decimator

pytestmark = pytest.mark.gpu

U = dc.U
FI = 312.5e3
SHAPES = [(1, 1), (1, 7), (3, 8), (8, 272), (64, 64), (64, 4096),
          (2, 18), (5, 37), (12, 96), (16, 16), (20, 53), (63, 63 * 64)]
IDS = [f"R{R}-T{T}" for R, T in SHAPES]
MODES = [("fm", dc.FM), ("am", dc.AM)]
N_OUT = 3 * dc.TILE + 85


def _n_in(R, n_out=N_OUT):
    """n_out outputs, ending between two outputs where R allows it."""
    return (n_out - 1) * R + 1 + R // 3


def _bits(y):
    return np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)


# ---- 1: integer data, every sum an exact float32 ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_case(mode, R, T, chans):
    """(x complex64 [C][n], integer taps, d in units of 1/2 (FM) or 1 (AM) as int64, the exact sums a in those units)."""
    rng = np.random.default_rng(1000 * R + T + 7 * chans + mode)
    n = _n_in(R)
    if mode == dc.FM:
        q = rng.integers(0, 4, (chans, n))
        e = rng.integers(-3, 4, (chans, n))
        x = (np.array([1, 1j, -1, -1j])[q] * np.exp2(e)).astype(np.complex64)
        step = np.diff(q, axis=1, prepend=q[:, :1]) % 4
        d = np.array([0, 1, 2, -1])[step]
        d[:, 0] = 0                                              # x[-1] = 0
    else:
        base = np.array([3 + 4j, 5 + 12j, 8 + 15j, 1 + 0j, 0 + 1j])
        length = np.array([5, 13, 17, 1, 1])
        pick = rng.integers(0, 5, (chans, n))
        k = rng.integers(0, 8, (chans, n))
        sr, si = rng.choice([-1, 1], (chans, n)), rng.choice([-1, 1], (chans, n))
        v = base[pick] * k
        x = (sr * v.real + 1j * (si * v.imag)).astype(np.complex64)
        d = length[pick] * k
    g = rng.integers(-8, 9, T)
    g[g == 0] = 3
    a = np.stack([np.convolve(row, g)[:n:R] for row in d.astype(np.int64)])
    assert a.shape == (chans, N_OUT) and np.abs(a).max() < 1 << 24
    for arr in (x, g, d, a):
        arr.setflags(write=False)
    return x, g.astype(np.float32), d, a


@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("name,mode", MODES)
@pytest.mark.parametrize("R,T", SHAPES, ids=IDS)
def test_exact_data_bit_for_bit(R, T, name, mode, chans):
    x, g, d, a = _integer_case(mode, R, T, chans)
    unit = 0.5 if mode == dc.FM else 1.0
    want = (a.astype(np.float64) * unit * 0.125).astype(np.float32)        # scale 2^-3: exact
    assert np.array_equal(want.astype(np.float64), a * unit * 0.125)
    with Demodulator(name, FI, R, chans, taps=g, scale=0.125, max_host_samples=x.size) as dm:
        got = dm.process(x)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got, want)
        dm.reset()
        again = dm.process(x)                                    # d[0] = 0 again: the last sample of the first run is gone
        assert np.array_equal(_bits(again), _bits(got))
        if mode == dc.FM:
            assert np.all(again[:, 0] == 0.0)


# ---- 2: float data against the float64 contract ----------------------------------------------------------------------
def _float_taps(R, T):
    if T == 1:
        return np.ones(1, np.float32)
    Q = -(-T // R)
    return np.ascontiguousarray(design_decimator(max(R, 2), taps_per_phase=Q)[:T])


def _allow_a(mode, g, absd):
    """u ((T + 1) sum |g||d| + 2 A_d sum |g|) (AM: 2 A_d sum |g||d|) of absd = sum |g||d| per output."""
    disc = 2 * dc.a_d(mode) * (absd if mode == dc.AM else np.abs(g.astype(np.float64)).sum())
    return U * ((g.size + 1) * absd + disc)


@functools.lru_cache(maxsize=None)
def _float_case(mode, R, T):
    """Three channels: an FM tone with |d| <= 0.9, amplitude 0.1 .. 0.3 (AM: modulated around it), noise 3e-3."""
    rng = np.random.default_rng(9000 + 10 * R + T + mode)
    n, chans = _n_in(R), 3
    t = np.arange(n)
    x = np.empty((chans, n), np.complex64)
    for c in range(chans):
        dev = 0.1 * (c - 1) + 0.6 * np.sin(2 * np.pi * t * (0.013 + 0.004 * c) / R + c)
        amp = 0.1 + 0.1 * c
        if mode == dc.AM:
            amp = amp * (1.0 + 0.5 * np.sin(2 * np.pi * t * 0.011 / R))
        noise = 3e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x[c] = (amp * np.exp(1j * np.pi * np.cumsum(dev)) + noise).astype(np.complex64)
    g = _float_taps(R, T)
    d, a, _ = dc.reference(x, mode, g, R)
    if mode == dc.FM:
        assert np.abs(d).max() <= 0.9, np.abs(d).max()           # the +-pi wrap is not in play
    allow_a = _allow_a(mode, g, np.stack([dc.abs_fir(row, g, R) for row in d]))
    for arr in (x, g, d, a, allow_a):
        arr.setflags(write=False)
    return x, g, d, a, allow_a


def _ratio(got, ref, allow, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    ok = allow > 0                                               # an output that has seen only zeros is exact
    assert np.all(err[~ok] == 0)
    r = float(np.max(err[ok] / allow[ok])) if np.any(ok) else 0.0
    print(f"{what}: worst error / allowance {r:.4f}")
    return r


@pytest.mark.parametrize("name,mode", MODES)
@pytest.mark.parametrize("R,T", SHAPES, ids=IDS)
def test_against_the_float64_contract(R, T, name, mode):
    x, g, d, a, allow_a = _float_case(mode, R, T)
    with Demodulator(name, FI, R, 3, taps=g, max_host_samples=x.size) as dm:
        got = dm.process(x)
        if (R, T) == (1, 1):                                     # the discriminator alone
            allow_d = 2 * dc.a_d(mode) * U * (np.abs(d) if mode == dc.AM else np.ones_like(d))
            assert _ratio(got, d, allow_d, f"{name} discriminator") <= 1.0
        assert _ratio(got, a, allow_a, f"{name} R={R} T={T} filter") <= 1.0
        pole_mode = nat.DEMOD_POLE_LOWPASS if mode == dc.FM else nat.DEMOD_POLE_HIGHPASS
        for c in (0.757, 0.999):
            dm.set_pole(pole_mode, c)
            got = dm.process(x)
            ref = np.stack([dc.output(row, pole_mode, c, 1.0) for row in a])
            allow = allow_a + dc.pole_allowance(a, c)
            assert _ratio(got, ref, allow, f"{name} R={R} T={T} pole c={c}") <= 1.0


# ---- 3: any split of the input gives the same bits -------------------------------------------------------------------
def _device_run(dm, x, pieces, n_out, engine=None):
    """The block piece by piece through process_device, every piece's outputs behind those before it."""
    chans, n = x.shape
    with DeviceBuffer.of(x) as d_in, DeviceBuffer(4 * chans * n_out) as d_out:
        got = at = 0
        for k in pieces:
            got += dm.process_device(engine, d_in.at(8 * at, 8 * ((chans - 1) * n + k)), k, n, d_out.at(4 * got), n_out)
            at += k
        dm.reset()                                               # waits for the handle's work
        assert got == n_out and at == n
        return d_out.get(chans * n_out, np.float32).reshape(chans, n_out)


def _pieces(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


@pytest.mark.parametrize("name,R,T,pole_mode,c", [("fm", 1, 7, 1, 0.757), ("am", 3, 8, 2, 0.999), ("fm", 8, 272, 2, 0.9),
                                                  ("am", 64, 64, 1, 0.757), ("fm", 64, 4096, 1, 0.999),
                                                  ("am", 12, 96, 1, 0.9), ("fm", 63, 4032, 2, 0.757)],
                         ids=["fm-R1-low", "am-R3-high", "fm-R8-high", "am-R64-low", "fm-R64-T4096-low", "am-R12-low",
                              "fm-R63-T4032-high"])
def test_split_invariance(name, R, T, pole_mode, c):
    rng = np.random.default_rng(31 * R + T)
    n_out = dc.TILE + 45                                         # past a tile and four pole blocks, ending inside one
    n = _n_in(R, n_out)
    x = (0.3 * (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))).astype(np.complex64)
    with Demodulator(name, FI, R, 2, taps=_float_taps(R, T), max_host_samples=2 * n) as dm:
        dm.set_pole(pole_mode, c)
        one = dm.process(x)
        assert one.shape == (2, n_out)
        dm.reset()
        assert np.array_equal(_bits(dm.process(x)), _bits(one))                          # reset reproduces the run
        dm.reset()
        cuts = [0, 1, min(R + 2, n // 3), n // 2, n]
        host_parts = [dm.process(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(_bits(np.concatenate(host_parts, axis=1)), _bits(one))
        dm.reset()
        prime = 13 if R != 13 else 17
        for size in (n, 1, R - 1, R, R + 1, prime):                                       # size n: host = device entry
            if size < 1:
                continue
            got = _device_run(dm, x, _pieces(n, size), n_out)
            assert np.array_equal(_bits(got), _bits(one)), size
        mixed, left = [], n                                      # pieces that complete no output, between longer ones
        for k in [1, R - 1, 1, 1, 3 * R + 1, R - 1, prime, 70 * R, 1, 1]:
            if 0 < k <= left:
                mixed.append(k)
                left -= k
        got = _device_run(dm, x, mixed + ([left] if left else []), n_out)
        assert np.array_equal(_bits(got), _bits(one))


# ---- 3b: past 2^31 and 2^32 inputs -----------------------------------------------------------------------------------
LONG_BLOCK = 1 << 22


@functools.lru_cache(maxsize=None)
def _long_block():
    """One period of x[n] = block[n mod 2^22]: the phase steps 0.6 sin(2 pi 5 n / nb) half turns sum to nothing over a
    period, so the step across the seam is as small as the others (|d| <= 0.61, the +-pi wrap is not in play); the
    envelope 0.2 (1 + 0.5 sin(2 pi 3 n / nb)) has the same period; noise 1e-3."""
    nb = LONG_BLOCK
    rng = np.random.default_rng(2 ** 32 + 13)
    t = np.arange(nb) / nb
    phase = np.pi * np.cumsum(0.6 * np.sin(2 * np.pi * 5 * t))
    amp = 0.2 * (1.0 + 0.5 * np.sin(2 * np.pi * 3 * t))
    noise = 1e-3 * (rng.standard_normal(nb) + 1j * rng.standard_normal(nb))
    x = (amp * np.exp(1j * phase) + noise).astype(np.complex64)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("name,mode,R,pole_mode,c", [("fm", dc.FM, 64, dc.POLE_OFF, 0.0), ("am", dc.AM, 8, dc.POLE_LOW, 0.757)],
                         ids=["fm-R64", "am-R8-low"])
def test_streams_past_2_32_inputs(name, mode, R, pole_mode, c):
    """A block of 2^22 complex64 samples of one channel replayed 1025 times with the default audio filter: x[n] =
    block[n mod 2^22].  Checked against the float64 defining sum with every index in int64, under test 2's allowances:
    the first and last 160 outputs of the calls that end at 2^31 and 2^32 inputs and of the calls that begin there (the
    first ones read the history and the last raw sample); the call that begins at 2^32 is the last.  The pole's
    memory is c^256 < 2^-100 at c = 0.757, so its reference starts from y = 0 256 outputs before the first checked one.
    The output index stays below 2^31 here (2^32 / R outputs): only the input indices n_total, n_lo and the staged
    (jlo + j) R pass 2^31 and 2^32; m_first, jlo and m_first % 64 are long long by reading and stay untested beyond.
    Measured on the MI355X: 0.5 s at R = 64 and 3.2 s at R = 8, where demod_post_kernel walks a channel's 2^29 outputs
    with one workgroup (the time halves with every doubling of R); the down-converter's test takes 0.3 s."""
    nb, keep, lead = LONG_BLOCK, 160, 256
    reps = (1 << 32) // nb + 1
    checked = (reps // 2 - 1, reps // 2, reps - 2, reps - 1)
    x = _long_block()
    cap = nb // R + 2
    with Demodulator(name, FI, R, 1, max_host_samples=64) as dm, DeviceBuffer.of(x) as d_in, \
            DeviceBuffer(4 * cap * (1 + len(checked))) as d_a:
        g = dm.taps
        dm.set_pole(pole_mode, c)
        total, spans = 0, []
        for i in range(reps):                               # every other call overwrites slot 0
            slot = 1 + checked.index(i) if i in checked else 0
            k = dm.process_device(None, d_in.ptr, nb, nb, d_a.at(4 * cap * slot), cap)
            assert k <= cap
            if slot:
                spans.append((total, k, slot))
            total += k
        dm.reset()                                          # waits for the handle's stream
        assert total == -(-(reps * nb) // R)
        audio = d_a.get(cap * (1 + len(checked)), np.float32)
    T = g.size
    g64 = g.astype(np.float64)
    worst, n_lo, n_hi = 0.0, 1 << 62, 0
    for m0, k, slot in spans:
        for at in (0, k - keep):
            ms = m0 + at - (lead if pole_mode else 0) + np.arange(keep + (lead if pole_mode else 0), dtype=np.int64)
            idx = ms[:, None] * R - np.arange(T, dtype=np.int64)[None, :]
            assert idx.min() > 0
            n_lo, n_hi = min(n_lo, int(idx.min())), max(n_hi, int(idx.max()))
            xs = x[idx % nb]
            d = np.abs(xs.astype(np.complex128)) if mode == dc.AM else dc.phase_step(xs, x[(idx - 1) % nb])
            assert mode == dc.AM or np.abs(d).max() <= 0.9
            a = d @ g64
            allow = _allow_a(mode, g, np.abs(d) @ np.abs(g64))
            ref = dc.output(a, pole_mode, c, 1.0)
            if pole_mode:
                allow = allow + dc.pole_allowance(a, c)
                ref, allow = ref[lead:], allow[lead:]
            got = audio[cap * slot + at:cap * slot + at + keep]
            worst = max(worst, _ratio(got, ref, allow, f"past 2^32 {name} R={R}: outputs {m0 + at} .."))
    assert n_lo < 1 << 31 < 1 << 32 < n_hi
    assert worst <= 1.0


# ---- 3c: entry points: taps on a live handle, host blocks above max_host_samples ---------------------------------------
def _set_taps(dm, g):
    g = np.ascontiguousarray(g, dtype=np.float32)
    nat.check(nat.lib.tdsa_demod_set_taps(dm._h, g.ctypes.data_as(C.c_void_p), int(g.size)))
    dm.taps, dm._inputs = g, 0


def _meas_equal(m, want):
    return all(np.array_equal(getattr(m, f), getattr(want, f)) for f in ("count", "max", "min", "sum", "sumsq"))


@pytest.mark.parametrize("name", ["fm", "am"])
def test_set_taps_on_a_handle_that_has_streamed(name):
    """A shorter filter shortens Q inside tap and history buffers sized for the handle's max_taps (64 phases, 3 in
    use, the history's channel stride still 64 R); afterwards the handle must behave as a fresh one with those taps:
    history, last sample and pole state cleared, inputs counted from 0, the pole kept, the measurements restarted."""
    R, chans = 12, 2
    rng = np.random.default_rng(78)
    long_g = (rng.standard_normal(64 * R) / R).astype(np.float32)
    short_g = (rng.standard_normal(3 * R - 5) / R).astype(np.float32)
    n_out = dc.TILE + 45
    n = _n_in(R, n_out)
    first = (0.3 * (rng.standard_normal((chans, n + 5 * R + 3)) + 1j * rng.standard_normal((chans, n + 5 * R + 3)))).astype(np.complex64)
    later = (0.3 * (rng.standard_normal((chans, n)) + 1j * rng.standard_normal((chans, n)))).astype(np.complex64)
    cut = n // 2 + 1
    assert cut % R and -(-cut // R) % dc.POLE_BLOCK      # the second call starts between two outputs, inside a pole block
    kw = dict(deemphasis=75e-6, scale=0.5, max_host_samples=first.size)

    def run(dm):
        y = np.concatenate([dm.process(later[:, :cut]), dm.process(later[:, cut:])], axis=1)
        return y, dm.measure()

    def fresh(g):
        with Demodulator(name, FI, R, chans, taps=g, **kw) as dm:
            return run(dm)

    with Demodulator(name, FI, R, chans, taps=long_g, **kw) as dm:
        dm.process(first)
        assert np.all(dm.measure().count == dc.n_outputs(first.shape[1], R))
        _set_taps(dm, short_g)
        none = dm.measure()
        assert np.all(none.count == 0) and np.all(none.sum == 0) and np.all(none.sumsq == 0)
        assert np.all(none.max == -np.inf) and np.all(none.min == np.inf)
        y_short, m_short = run(dm)
        _set_taps(dm, long_g)
        assert np.all(dm.measure().count == 0)
        y_long, m_long = run(dm)
    for got, m, g in ((y_short, m_short, short_g), (y_long, m_long, long_g)):
        want, m_want = fresh(g)
        assert got.shape == (chans, n_out) and np.array_equal(_bits(got), _bits(want))
        assert np.all(m.count == n_out) and _meas_equal(m, m_want)


@pytest.mark.parametrize("name", ["fm", "am"])
def test_host_block_larger_than_max_host_samples(name):
    """process() cuts a block above max_host_samples / C per channel into several library calls, each an offset into
    the rows of the whole block with in_stride = n: the bits of the single call, and its measurements' count and extremes."""
    R, T, chans = 3, 8, 3
    rng = np.random.default_rng(79)
    n_out = dc.TILE + 45
    n = _n_in(R, n_out)
    x = (0.3 * (rng.standard_normal((chans, n)) + 1j * rng.standard_normal((chans, n)))).astype(np.complex64)
    kw = dict(taps=_float_taps(R, T), deemphasis=75e-6)
    with Demodulator(name, FI, R, chans, max_host_samples=chans * n, **kw) as dm:
        one, m_one = dm.process(x), dm.measure()
    with Demodulator(name, FI, R, chans, max_host_samples=chans * (n // 3 + 1), **kw) as dm:
        assert dm.max_host_samples // chans < n < 3 * (dm.max_host_samples // chans)
        got, m = dm.process(x), dm.measure()
    assert got.shape == one.shape == (chans, n_out) and np.array_equal(_bits(got), _bits(one))
    for f in ("count", "max", "min"):
        assert np.array_equal(getattr(m, f), getattr(m_one, f)), f
    assert np.allclose(m.sum, m_one.sum, rtol=1e-12, atol=1e-12) and np.allclose(m.sumsq, m_one.sumsq, rtol=1e-12, atol=1e-12)


# ---- 4: layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fm", "am"])
def test_strides_leave_the_gaps_alone_and_channels_are_independent(name):
    R, T, chans = 3, 8, 3
    rng = np.random.default_rng(55)
    n_out = dc.TILE + 45
    n = _n_in(R, n_out)
    in_stride, out_stride = n + 7, n_out + 5
    x = np.zeros((chans, in_stride), np.complex64)
    x[:] = (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)).astype(np.complex64)
    g = _float_taps(R, T)
    sentinel = np.float32(-12345.5)
    kw = dict(taps=g, deemphasis=75e-6, scale=0.5)
    singles = []
    for c in range(chans):
        with Demodulator(name, FI, R, 1, max_host_samples=n, **kw) as one:
            singles.append(one.process(x[c, :n])[0])
    want = np.stack(singles)
    with Demodulator(name, FI, R, chans, max_host_samples=chans * n, **kw) as dm:
        assert np.array_equal(_bits(dm.process(x[:, :n])), _bits(want))        # C = 3 is three single-channel handles
        dm.reset()
        host = np.full((chans + 1, out_stride), sentinel, dtype=np.float32)
        cnt = C.c_size_t()
        nat.check(nat.lib.tdsa_demod_process(dm._h, x.ctypes.data_as(C.c_void_p), n, in_stride,
                                             host.ctypes.data_as(C.c_void_p), out_stride, C.byref(cnt)))
        assert cnt.value == n_out
        dm.reset()
        with DeviceBuffer.of(x) as d_in, DeviceBuffer.of(np.full((chans + 1, out_stride), sentinel, dtype=np.float32)) as d_out:
            assert dm.process_device(None, d_in.ptr, n, in_stride, d_out.ptr, out_stride) == n_out
            dm.reset()
            dev = d_out.get((chans + 1) * out_stride, np.float32).reshape(chans + 1, out_stride)
    for got in (host, dev):
        assert np.array_equal(_bits(got[:chans, :n_out]), _bits(want))
        assert np.all(_bits(got[:chans, n_out:]) == _bits(sentinel)) and np.all(_bits(got[chans]) == _bits(sentinel))


# ---- 5: measurements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", MODES)
def test_measurements(name, mode):
    R, T, chans = 3, 8, 3
    x, g, d, a = _integer_case(mode, R, T, chans)
    unit = 0.5 if mode == dc.FM else 1.0
    a64 = a.astype(np.float64) * unit
    cnt, mx, mn, s, ss = dc.measurements(a64)
    n = x.shape[1]
    with Demodulator(name, FI, R, chans, taps=g, deemphasis=75e-6, max_host_samples=x.size) as dm:
        none = dm.measure()
        assert np.all(none.count == 0) and np.all(none.sum == 0) and np.all(np.isnan(none.mean))
        whole = dm.process(x)
        cuts = [0, 5, 5 + R - 1, 400, 400 + 64 * R, n]                  # the same input in split calls, measured again
        for rerun in range(2):
            m = dm.measure()
            assert np.array_equal(m.count, cnt) and m.max.dtype == np.float32
            assert np.array_equal(m.max.astype(np.float64), mx) and np.array_equal(m.min.astype(np.float64), mn)
            assert np.all(np.abs(m.sum - s) <= N_OUT * 2.0 ** -52 * np.abs(a64).sum(axis=1))
            assert np.all(np.abs(m.sumsq - ss) <= N_OUT * 2.0 ** -52 * ss)
            want = derive(name, FI, cnt, mx, mn, s, ss)
            if mode == dc.FM:
                assert np.allclose(m.offset_hz, want.offset_hz, rtol=1e-12, atol=1e-9)
                assert np.allclose(m.peak_plus_hz, FI / 2 * (mx - s / N_OUT), rtol=1e-12)
                assert np.allclose(m.rms_hz, want.rms_hz, rtol=1e-9)
            else:
                assert np.allclose(m.carrier, s / N_OUT, rtol=1e-12)
                assert np.allclose(m.depth, (mx - mn) / (mx + mn), rtol=1e-12)
            if rerun == 0:
                dm.reset()                                        # also zeroes the measurements
                parts = [dm.process(x[:, p:q]) for p, q in zip(cuts[:-1], cuts[1:])]
                assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
        # reset_measure between two calls: the accumulators start again, the audio does not notice
        dm.reset()
        first = dm.process(x[:, :400])
        dm.reset_measure()
        zero = dm.measure()
        assert np.all(zero.count == 0) and np.all(zero.sum == 0) and np.all(zero.sumsq == 0)
        rest = dm.process(x[:, 400:])
        assert np.array_equal(_bits(np.concatenate([first, rest], axis=1)), _bits(whole))
        tail = dm.measure()
        k = first.shape[1]
        assert np.array_equal(tail.count, cnt - k)
        assert np.array_equal(tail.max.astype(np.float64), a64[:, k:].max(axis=1))
        assert np.array_equal(tail.min.astype(np.float64), a64[:, k:].min(axis=1))


# ---- 6: the chain channelizer -> demodulator -------------------------------------------------------------------------
M, OS, RA = 16, 2, 2
FS = 16 * 48e3                       # channels 48 kHz apart at 96 kHz each; audio at 48 kHz
TONE, CH = 1000.0, 5


@functools.lru_cache(maxsize=None)
def _capture():
    """A 1 kHz tone FM-modulated (+-5 kHz) onto the centre of channel 5, over weak noise: 0.1 s."""
    n = 4800 * RA * (M // OS)
    t = np.arange(n) / FS
    rng = np.random.default_rng(66)
    phase = 2 * np.pi * CH * FS / M * t + (5000.0 / TONE) * np.sin(2 * np.pi * TONE * t)
    x = 0.5 * np.exp(1j * phase) + 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def _chain(streams, pieces):
    """The capture in `pieces` through the bank and the demodulator, each piece on streams[i]; returns (audio, y)."""
    x = _capture()
    n = x.size
    with Channelizer(M, FS, OS, max_host_samples=n) as bank, \
            Demodulator("fm", FS * OS / M, RA, M, deemphasis=75e-6, max_host_samples=M * (n * OS // M + 1)) as dm:
        ny = bank.outputs_completed_by(n)
        na = dm.outputs_completed_by(ny)
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * M * ny) as d_y, DeviceBuffer(4 * M * na) as d_a:
            at = gy = ga = 0
            for eng, k in zip(streams, pieces):
                ky = bank.process_device(eng, nat.IN_C64, d_x.at(8 * at, 8 * k), k, d_y.at(8 * gy), ny)
                ga += dm.process_device(eng, d_y.at(8 * gy), ky, ny, d_a.at(4 * ga), na)   # no host wait between
                at += k
                gy += ky
            assert (at, gy, ga) == (n, ny, na)
            meas = dm.measure()                                  # waits for the demodulator, which waited for the bank
            bank.reset()
            y = d_y.get(M * ny, np.complex64).reshape(M, ny)
            audio = d_a.get(M * na, np.float32).reshape(M, na)
    return audio, y, meas


def test_chain_equals_the_path_staged_through_the_host_and_finds_the_tone():
    x = _capture()
    n = x.size
    pieces = [n // 3, n // 5 + 3, n - n // 3 - n // 5 - 3]
    with SpectrumEngine(64) as eng:
        audio, y, meas = _chain([eng] * 3, pieces)
    with Channelizer(M, FS, OS, max_host_samples=n) as bank:
        y_host = bank.process(x)
    assert np.array_equal(y.view(np.uint64), y_host.view(np.uint64))
    with Demodulator("fm", FS * OS / M, RA, M, deemphasis=75e-6, max_host_samples=y_host.size) as dm:
        staged = dm.process(y_host)
        m_host = dm.measure()
    assert np.array_equal(_bits(audio), _bits(staged))
    for f in ("count", "max", "min", "sum", "sumsq"):
        if f in ("sum", "sumsq"):                                # one tree per call: the calls differ, the values barely
            assert np.allclose(getattr(meas, f), getattr(m_host, f), rtol=1e-12, atol=1e-12)
        else:
            assert np.array_equal(getattr(meas, f), getattr(m_host, f)), f
    # the tone: the largest bin of channel 5's audio past the filters' fill is 1 kHz
    a5 = audio[CH, 800:].astype(np.float64)
    spec = np.abs(np.fft.rfft(a5 * np.hanning(a5.size)))
    spec[0] = 0.0
    f_peak = np.argmax(spec) * (FS * OS / M / RA) / a5.size
    assert abs(f_peak - TONE) <= (FS * OS / M / RA) / a5.size, f_peak
    # measure() on it is the contract applied to the channelizer's own output for that channel
    g = design_audio_filter(RA)
    d, a, _ = dc.reference(y[CH], dc.FM, g, RA)
    cnt, mx, mn, s, ss = dc.measurements(a)
    allow = U * ((g.size + 1) * dc.abs_fir(d[0], g, RA) + 2 * dc.A_D_FM * np.abs(g.astype(np.float64)).sum())
    assert meas.count[CH] == cnt[0]
    assert abs(float(meas.max[CH]) - mx[0]) <= allow.max() and abs(float(meas.min[CH]) - mn[0]) <= allow.max()
    assert abs(meas.sum[CH] - s[0]) <= allow.sum() and abs(meas.sumsq[CH] - ss[0]) <= 2 * np.abs(a[0]).max() * allow.sum() + allow.sum() ** 2
    want = derive("fm", FS * OS / M, cnt, mx, mn, s, ss)
    assert abs(meas.offset_hz[CH] - want.offset_hz[0]) < 0.05
    assert abs(meas.rms_hz[CH] - want.rms_hz[0]) < 0.05


def test_hopping_streams_give_the_bits_of_one_stream():
    """The Lane order rule: the same calls alternating between two plans' streams and the handle's own give the bits of
    all on one stream.  The input is complete before the first call, so only the handle's own state is at stake."""
    x = _capture()
    with Channelizer(M, FS, OS, max_host_samples=x.size) as bank:
        y = bank.process(x)[:, :1500]
    n = y.shape[1]
    pieces = [n // 6 + i for i in range(5)]
    pieces.append(n - sum(pieces))

    def run(streams):
        with Demodulator("fm", FS * OS / M, RA, M, deemphasis=75e-6, max_host_samples=M) as dm:
            na = dm.outputs_completed_by(n)
            with DeviceBuffer.of(y) as d_y, DeviceBuffer(4 * M * na) as d_a:
                at = ga = 0
                for eng, k in zip(streams, pieces):
                    ga += dm.process_device(eng, d_y.at(8 * at, 8 * ((M - 1) * n + k)), k, n, d_a.at(4 * ga), na)
                    at += k
                meas = dm.measure()                              # on the handle's stream, behind the last launch
                return d_a.get(M * na, np.float32).reshape(M, na), meas

    with SpectrumEngine(64) as a, SpectrumEngine(64) as b:
        audio, meas = run([(a, None, b)[i % 3] for i in range(6)])
    audio1, meas1 = run([None] * 6)
    assert np.array_equal(_bits(audio), _bits(audio1))
    assert np.array_equal(meas.count, meas1.count) and np.array_equal(meas.sum, meas1.sum)
    assert np.array_equal(meas.max, meas1.max) and np.array_equal(meas.sumsq, meas1.sumsq)
