"""The down-converter's six kernel widths on the MI355X, pinned against something other than the kernel itself: an
exact integer FIR (every tap, residue, output and tile, bit for bit), the float64 restatement with a rotating NCO at the
widths and tap depths test_gpu_zoom.py leaves out, retunes in mid-stream, the rotator at every table entry, streams past
2^32 inputs, ZoomSpectrum's multi-launch and hop > nfft paths, and tdsa_ddc_set_taps on a handle that has streamed.

LANES and the outputs per workgroup MT = 2048 / LANES by decimation (launch_ddc in tdsa_ddc.hip, zc.lanes here):
D = 2: 2, 1024;  3-4: 4, 512;  5-8: 8, 256;  9-16: 16, 128;  17-63: 32, 64;  >= 64: 64, 32."""
import ctypes as C
import functools

import numpy as np
import pytest

import zoom_contract as zc
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat
from topdogspectrumanalyser_amd.utils.constants import DSPConstants
from topdogspectrumanalyser_amd.zoom import DownConverter, ZoomSpectrum, design_decimator, zoom_window

pytestmark = pytest.mark.gpu

FS = 20e6
ULP1 = float(np.spacing(np.float32(1)))


def _raw(rng, n, fmt):
    if fmt == zc.FMT_I8:
        return rng.integers(-128, 128, 2 * n).astype(np.int8)
    if fmt == zc.FMT_U8:
        return rng.integers(0, 256, 2 * n).astype(np.uint8)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)


def _split(raw, fmt, cuts):
    step = 1 if fmt == zc.FMT_C64 else 2
    edges = [0] + list(cuts) + [len(raw) // step]
    return [raw[step * a:step * b] for a, b in zip(edges[:-1], edges[1:])]


def _run(ddc, parts):
    return np.concatenate([ddc.process(p) for p in parts])


def _set_step(ddc, s):
    nat.check(nat.lib.tdsa_ddc_set_nco(ddc._h, int(s)))


def _set_taps(ddc, h):
    h = np.ascontiguousarray(h, dtype=np.float32)
    nat.check(nat.lib.tdsa_ddc_set_taps(ddc._h, h.ctypes.data_as(C.c_void_p), int(h.size)))


def _check_bound(y, ref, bound, what):
    """The project's accuracy bound (test_accuracy_against_the_restatement): max <= 1e-5, rms <= 1e-6 of
    sum|h| max|x|, over every output.  Returns the two ratios to their bounds."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    err = np.abs(y - ref)
    rmax, rrms = err.max() / (1e-5 * bound), np.sqrt(np.mean(err ** 2)) / (1e-6 * bound)
    assert rmax <= 1.0, (what, "max", rmax)
    assert rrms <= 1.0, (what, "rms", rrms)
    return rmax, rrms


# ---- 1. exact-integer FIR ------------------------------------------------------------------------------------------
# With offset 0 the phase is 0 at every input, and ddc_mix returns x exactly: the table entry is (1, -0), t = 0, so
# sl = fma(0, 1/6, -0) = +0 and cm1 = -0, rr = 1 + fma(1, -0, -(-0 * 0)) = 1, ri = -0 + fma(-0, -0, 1 * 0) = +0, and the
# product is (fma(xr, 1, -(xi * 0)), fma(xr, 0, xi * 1)) = (xr, xi) by value.  Inputs with integer parts in [-A, A]
# (int8 raw: the same integers over 128, a dyadic scaling) and integer taps in [-B, B] with A B T < 2^24 make every
# partial sum, in any order, an integer (or a multiple of 2^-7) below 2^24: float32 is exact, so the kernel must give
# the int64 convolution.  A = B = 7 holds up to T = 64 * 4096.
A_MAX = B_MAX = 7
# (D, Q = ceil(T / D)); each runs T = Q D and T = (Q - 1) D + 1 (Q = 1: T = D and T = 1).
#   LANES 2:  D = 2                      LANES 4:  D = 3 (part of a group), 4 (a full group)
#   LANES 8:  D = 5, 8                   LANES 16: D = 9, 13, 16
#   LANES 32: D = 17, 24, 32, 33 (a second group of 1 residue), 63 (a second group of 31)
#   LANES 64: D = 64, 65 (second group of 1), 100, 128 (two full groups), 4095 (last group of 63), 4096
#   Q = 1, 7, 8, 9, 16, 34, 63, 64 each at least twice; Q = 64 at D = 2, 9, 24, 65, 4096
EXACT_CASES = [
    (2, 1), (2, 9), (2, 34), (2, 64),
    (3, 7), (3, 63), (4, 8), (4, 16),
    (5, 34), (5, 9), (8, 16), (8, 63),
    (9, 1), (9, 64), (13, 34), (13, 8), (16, 63), (16, 7),
    (17, 9), (24, 64), (24, 1), (32, 16), (33, 34), (33, 8), (63, 7), (63, 63),
    (64, 34), (64, 1), (65, 64), (65, 9), (100, 16), (128, 8), (128, 63), (4095, 7), (4095, 34), (4096, 1), (4096, 64),
]


@pytest.mark.parametrize("fmt", [zc.FMT_C64, zc.FMT_I8])
@pytest.mark.parametrize("D,Q", EXACT_CASES)
def test_integer_fir_is_exact(D, Q, fmt):
    MT = 2048 // zc.lanes(D)
    for T in sorted({Q * D, (Q - 1) * D + 1}):
        assert A_MAX * B_MAX * T < 1 << 24 and -(-T // D) == Q
        rng = np.random.default_rng([D, T, fmt])
        n = T + (2 * MT + 5) * D + 3          # three tiles of outputs with a full window, the last tile partial
        re, im = rng.integers(-A_MAX, A_MAX + 1, (2, n))
        h = rng.choice(np.r_[-B_MAX:0, 1:B_MAX + 1], T).astype(np.float32)      # no zero tap: a dropped one shows
        if fmt == zc.FMT_C64:
            raw, scale = (re + 1j * im).astype(np.complex64), 1.0
        else:
            raw, scale = np.stack([re, im], axis=1).reshape(-1).astype(np.int8), 128.0
        cut = (Q + MT + 3) * D + 1            # the second call starts inside a tile and reads the device history
        assert cut % D and -(-cut // D) % MT
        with DownConverter(D, FS, 0.0, taps=h, max_host_samples=max(cut, n - cut) + 1) as ddc:
            assert ddc.phase_step == 0
            y = _run(ddc, _split(raw, fmt, [cut]))
        yr, yi = zc.integer_fir(re, im, h, D)
        want = ((yr + 1j * yi) / scale).astype(np.complex64)
        assert np.abs(yr).max() < 1 << 24 and np.abs(yi).max() < 1 << 24
        assert y.size == want.size == zc.n_outputs(n, D) and y.size >= 2 * MT + 5
        bad = np.nonzero(y != want)[0]
        assert bad.size == 0, (T, bad.size, bad[:8], y[bad[:4]], want[bad[:4]])


# ---- 2. accuracy with a rotating NCO at the untested widths and depths -----------------------------------------------
@pytest.mark.parametrize("D", [13, 24, 33, 63, 65])
@pytest.mark.parametrize("fmt", [zc.FMT_I8, zc.FMT_U8, zc.FMT_C64])
def test_accuracy_against_the_restatement_at_other_widths(D, fmt):
    """test_accuracy_against_the_restatement's bound at LANES 16, 32 and 64 with partly filled groups, over three tiles
    and every output; the tap sets are the default design (Q = 34), random 3 D + 1 (Q = 4) and random 64 D (Q = 64)."""
    rng = np.random.default_rng(D * 7 + fmt)
    MT = 2048 // zc.lanes(D)
    worst = (0.0, 0.0)
    for T in (None, 3 * D + 1, 64 * D):
        h = design_decimator(D) if T is None else rng.standard_normal(T).astype(np.float32) / D
        T = h.size
        n = T + (2 * MT + 5) * D + 5
        raw = _raw(rng, n, fmt)
        bound = np.abs(h.astype(np.float64)).sum() * np.abs(zc.unpack(raw, fmt)).max()
        for off in (0.0, 0.3 * FS, -0.3 * FS, 0.49 * FS, -0.49 * FS):
            with DownConverter(D, FS, off, taps=h, max_host_samples=n) as ddc:
                y = ddc.process(raw)
                step = ddc.phase_step
            assert y.size == zc.n_outputs(n, D)
            r = _check_bound(y, zc.reference(raw, fmt, h, D, [(0, step)]), bound, (T, off))
            worst = max(worst[0], r[0]), max(worst[1], r[1])
    print(f"\naccuracy D={D} fmt={fmt}: worst max / bound {worst[0]:.4f}, worst rms / bound {worst[1]:.4f}")


# ---- 3. retunes against the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 24])
@pytest.mark.parametrize("fmt", [zc.FMT_I8, zc.FMT_U8, zc.FMT_C64])
def test_retunes_in_mid_stream_follow_the_contract(D, fmt):
    """Three retunes at inputs that are no multiple of D, with calls also split elsewhere: a wrong phase carried over a
    retune turns everything after it by a constant angle, an error of the order of the signal."""
    rng = np.random.default_rng(100 * D + fmt)
    h = design_decimator(D)
    T = h.size
    n = 6 * T + 301 * D + 7
    raw = _raw(rng, n, fmt)
    steps = [int(rng.integers(1, 1 << 32)), 0x80000000, 0xFFFFFFFF, int(rng.integers(1, 1 << 32))]
    at = [T + 7 * D + 1, 2 * T + 90 * D + D - 1, 4 * T + 155 * D + D // 2 + 1]
    assert all(a % D for a in at) and at[-1] < n - T
    retunes = list(zip([0] + at, steps))
    cuts = sorted(set(at) | {5, T + 1, at[0] + 3, at[1] + 11 * D, at[2] - 2, n - 9})
    with DownConverter(D, FS, 0.0, taps=h, max_host_samples=n) as ddc:
        _set_step(ddc, steps[0])
        out = []
        for part, end in zip(_split(raw, fmt, cuts), cuts + [n]):
            out.append(ddc.process(part))
            if end in at:
                _set_step(ddc, steps[1 + at.index(end)])
        y = np.concatenate(out)
    bound = np.abs(h.astype(np.float64)).sum() * np.abs(zc.unpack(raw, fmt)).max()
    r = _check_bound(y, zc.reference(raw, fmt, h, D, retunes), bound, retunes)
    print(f"\nretunes D={D} fmt={fmt}: max / bound {r[0]:.4f}, rms / bound {r[1]:.4f}")


# ---- 4. rotator sweep ------------------------------------------------------------------------------------------------
def test_rotator_at_every_table_entry_and_low_bit_extreme():
    """T = 1, h = [1], D = 2, x = 1: y[m] is the rotator at p[2m].  One input at step low + 2^19, then 8192 at step
    2^19, put p[2m] = low + m 2^20 for m = 1 .. 4096: every table entry at one value of the low 20 bits.  DESIGN.md
    section 4.8 states 1.5 ulp of |h| = 1; the worst ratio measured on the MI355X is printed (0.50 in the float32
    emulation of test_zoom_host.py)."""
    rng = np.random.default_rng(48)
    one = np.ones(1, np.float32)
    worst, count = 0.0, 0

    def check(y, p):
        nonlocal worst, count
        want = np.exp(-2j * np.pi * (p[::2].astype(np.float64) / 2.0 ** 32))
        assert y.size == want.size
        err = np.maximum(np.abs(y.real.astype(np.float64) - want.real), np.abs(y.imag.astype(np.float64) - want.imag))
        k = int(np.argmax(err))
        assert err[k] <= 1.5 * ULP1, (hex(int(p[2 * k])), err[k] / ULP1)
        worst, count = max(worst, err[k] / ULP1), count + y.size

    lows = [0, 1, 2, 0x7FFFF, 0x80000, 0xFFFFD, 0xFFFFE, 0xFFFFF] + [int(v) for v in rng.integers(0, 1 << 20, 8)]
    with DownConverter(2, FS, 0.0, taps=one, max_host_samples=1 << 16) as ddc:
        for low in lows:
            ddc.reset()
            retunes = [(0, (low + (1 << 19)) % (1 << 32)), (1, 1 << 19)]
            _set_step(ddc, retunes[0][1])
            y0 = ddc.process(np.ones(1, np.complex64))
            _set_step(ddc, retunes[1][1])
            y = np.concatenate([y0, ddc.process(np.ones(8192, np.complex64))])
            p = zc.phases(8193, retunes)
            assert np.array_equal(p[2::2] & 0xFFFFF, np.full(4096, low)) and np.unique(p[2::2] >> 20).size == 4096
            check(y, p)
        for _ in range(2):                                  # random phases: a random odd step visits 2^15 of them
            s = int(rng.integers(0, 1 << 31)) * 2 + 1
            ddc.reset()
            _set_step(ddc, s)
            check(ddc.process(np.ones(1 << 16, np.complex64)), zc.phases(1 << 16, [(0, s)]))
    assert count >= 100_000
    print(f"\nrotator: {count} phases, worst error {worst:.3f} x spacing(1) (bound 1.5)")


# ---- 5. past 2^32 inputs ---------------------------------------------------------------------------------------------
LONG_BLOCK = 1 << 24


@functools.lru_cache(maxsize=None)
def _long_block():
    raw = np.random.default_rng(2 ** 32 + 1).integers(-128, 128, 2 * LONG_BLOCK).astype(np.int8)
    raw.setflags(write=False)
    iq = raw.astype(np.int32).reshape(-1, 2)
    return raw, float(np.sqrt((iq[:, 0] ** 2 + iq[:, 1] ** 2).max())) / 128.0      # and max |x|


@pytest.mark.parametrize("D", [64, 3])
def test_streams_past_2_32_inputs(D):
    """A block of 2^24 int8 samples replayed 257 times: x[n] = block[n mod 2^24], p[n] = n s mod 2^32.  Checked against
    the float64 defining sum: the last outputs of the calls that end at 2^31 and 2^32 and the first and last outputs of
    the calls that begin there (the first ones read the history); the call that begins at 2^32 is the last."""
    reps, nb = 257, LONG_BLOCK
    raw, x_max = _long_block()
    h = design_decimator(D)
    T = h.size
    checked = (127, 128, 255, 256)
    cap = nb // D + 2
    with DownConverter(D, FS, 0.123 * FS, max_host_samples=64) as ddc, DeviceBuffer(raw.nbytes) as d_in, \
            DeviceBuffer(8 * cap * (1 + len(checked))) as d_y:
        step = ddc.phase_step
        d_in.put(raw)
        total, spans = 0, []
        for i in range(reps):                               # every other call overwrites slot 0
            slot = 1 + checked.index(i) if i in checked else 0
            k = ddc.process_device(None, nat.IN_I8, d_in.ptr, nb, d_y.at(8 * cap * slot))
            assert k <= cap
            if slot:
                spans.append((total, k, slot))
            total += k
        ddc.reset()                                         # waits for the handle's stream
        assert total == -(-(reps * nb) // D)
        got, ms = [], []
        for m0, k, slot in spans:
            for a in (0, k - 160):
                got.append(d_y.get(160, np.complex64, 8 * (cap * slot + a)))
                ms.append(m0 + a + np.arange(160, dtype=np.int64))
    got, ms = np.concatenate(got), np.concatenate(ms)
    assert ms.min() * D < 1 << 31 < ms.max() * D and np.any(ms * D > 1 << 32)
    idx = ms[:, None] * D - np.arange(T, dtype=np.int64)[None, :]
    assert idx.min() > 0
    j = idx % nb
    x = (raw[2 * j].astype(np.float64) + 1j * raw[2 * j + 1].astype(np.float64)) / 128.0
    p = (idx.astype(np.uint64) * np.uint64(step)) & np.uint64(0xFFFFFFFF)          # wraps mod 2^64, then mod 2^32
    n_big = int(idx.max())
    assert int(p.reshape(-1)[np.argmax(idx)]) == (n_big * step) % (1 << 32)
    ref = (x * np.exp(-2j * np.pi * (p.astype(np.float64) / 2.0 ** 32))) @ h.astype(np.float64)
    bound = np.abs(h.astype(np.float64)).sum() * x_max
    r = _check_bound(got, ref, bound, D)
    print(f"\npast 2^32 D={D}: {got.size} outputs, max / bound {r[0]:.4f}, rms / bound {r[1]:.4f}")


# ---- 6. ZoomSpectrum paths -------------------------------------------------------------------------------------------
def _zoom_rows(raw, D, N, hop, cuts, mhs):
    with ZoomSpectrum(FS, D, N, offset_hz=0.07 * FS, hop=hop, max_host_samples=mhs) as z:
        z.engine.configure(hold_max=True, hold_min=True)
        rows = [z.process(p) for p in _split(raw, zc.FMT_I8, cuts)]
        mx, mn = z.hold()
        return np.concatenate(rows), mx, mn, z.engine.max_frames, [r.shape[0] for r in rows]


def _separate_engine_rows(raw, D, N, hop, max_frames):
    """The down-converter's host output from first_full_output on, through an engine configured as ZoomSpectrum's."""
    with DownConverter(D, FS, 0.07 * FS, max_host_samples=len(raw) // 2) as ddc:
        y = ddc.process(raw)
        m0 = ddc.first_full_output
    with SpectrumEngine(N, max_frames=max_frames) as eng:
        eng.set_window(zoom_window(N))
        eng.configure(db_mode="mag", log_floor=DSPConstants.LOG_FLOOR, dc_alpha=-1.0, hold_max=True, hold_min=True)
        rows = eng.process(y[m0:], hop=hop)
        mx, mn = eng.hold()
    return rows, mx, mn


def test_zoom_spectrum_more_frames_than_one_launch():
    D, N, hop, nf = 2, 64, 16, 600
    m0 = -(-(34 * D - 1) // D)
    n = D * (m0 + (nf - 1) * hop + N)
    raw = _raw(np.random.default_rng(61), n, zc.FMT_I8)
    r0, mx0, mn0, max_frames, per_call = _zoom_rows(raw, D, N, hop, [], n)
    assert r0.shape == (nf, N) and max_frames == 256 and per_call == [nf]      # three engine launches in one call
    rs, mxs, mns = _separate_engine_rows(raw, D, N, hop, nf)
    assert np.array_equal(r0, rs) and np.array_equal(mx0, mxs) and np.array_equal(mn0, mns)
    r1, mx1, mn1, _, per_call = _zoom_rows(raw, D, N, hop, list(range(2999, n, 2999)), n)
    assert max(per_call) < 256 and len(per_call) > 3
    assert np.array_equal(r1, r0) and np.array_equal(mx1, mx0) and np.array_equal(mn1, mn0)


def test_zoom_spectrum_hop_beyond_the_frame():
    D, N, hop, nf = 5, 64, 101, 40
    m0 = -(-(34 * D - 1) // D)
    n = D * (m0 + (nf - 1) * hop + N) + 3
    rng = np.random.default_rng(62)
    raw = _raw(rng, n, zc.FMT_I8)
    r0, mx0, mn0, _, _ = _zoom_rows(raw, D, N, hop, [], n)
    assert r0.shape == (nf, N)
    rs, mxs, mns = _separate_engine_rows(raw, D, N, hop, nf)
    assert np.array_equal(r0, rs) and np.array_equal(mx0, mxs) and np.array_equal(mn0, mns)
    # ragged: calls far shorter than hop - nfft outputs, so the next frame's start lies beyond what is held
    for cuts in (list(np.cumsum(rng.integers(1, 140, 2000))), list(range(D * (m0 + N) + 1, n, D * hop)),
                 [1, D - 1, D * (m0 + N), D * (m0 + N) + 1, D * (m0 + hop) - 1, D * (m0 + hop), n - 1]):
        r, mx, mn, _, _ = _zoom_rows(raw, D, N, hop, [int(c) for c in cuts if 0 < c < n], n)
        assert np.array_equal(r, r0) and np.array_equal(mx, mx0) and np.array_equal(mn, mn0)


# ---- 7. tdsa_ddc_set_taps on a live handle ---------------------------------------------------------------------------
def test_set_taps_on_a_handle_that_has_streamed():
    """A shorter filter shortens `phases` inside buffers sized for the handle's max_phases; afterwards the handle must
    behave as a fresh one: history cleared, input count and phase from 0, the step kept."""
    D = 13
    rng = np.random.default_rng(77)
    long_h = rng.standard_normal(64 * D).astype(np.float32) / D
    short_h = rng.standard_normal(3 * D + 1).astype(np.float32) / D
    first = _raw(rng, 300 * D + 5, zc.FMT_I8)
    later = _raw(rng, 400 * D + 7, zc.FMT_I8)
    cuts = [150 * D + 3]
    mhs = 400 * D + 7

    def fresh(h):
        with DownConverter(D, FS, 0.19 * FS, taps=h, max_host_samples=mhs) as ddc:
            return _run(ddc, _split(later, zc.FMT_I8, cuts))

    with DownConverter(D, FS, 0.19 * FS, taps=long_h, max_host_samples=mhs) as ddc:
        ddc.process(first)
        _set_taps(ddc, short_h)
        y_short = _run(ddc, _split(later, zc.FMT_I8, cuts))
        _set_taps(ddc, long_h)
        y_long = _run(ddc, _split(later, zc.FMT_I8, cuts))
    assert y_short.size == y_long.size == zc.n_outputs(400 * D + 7, D)
    assert np.array_equal(y_short.view(np.uint64), fresh(short_h).view(np.uint64))
    assert np.array_equal(y_long.view(np.uint64), fresh(long_h).view(np.uint64))
