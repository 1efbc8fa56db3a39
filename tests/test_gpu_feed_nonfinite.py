"""Non-finite samples through the three streaming filters on the MI355X (DESIGN.md sections 4.8, 4.12 and 4.13): the
down-converter, the channelizer and the demodulator.  The rule, as zoom_contract, chan_contract and demod_contract state
it: an output depends on the inputs of its padded window (mD - H, mD] only - H = ceil(T / D) D, P M, Q R - so a NaN or
inf at x[n*] changes no bit of any output outside it, in one call or split anywhere, and makes every output non-finite
that meets it under a non-zero tap; outputs that meet it only under the zero padding of the tap table are unspecified
and not looked at.  All three kernels multiply that padding and select "zero after the call" and "history before it"
after a load: what these tests hold them to.

Every case runs a stream x and its twin, equal except that the twin's x[n*] is finite, once in one call and once cut
right behind n* - the bad value is then the last sample of a call and reaches the next outputs through the history
kernel (the demodulator's FM also through the last raw sample) - followed by pieces shorter than D, which move it
through the history's own copy, hist[k + n_in].  Finite values are compared as bits.  n* is sample 0, the middle of the
second tile, and the last input of the first tile's outputs.  Three tiles plus a ragged remainder, as everywhere."""
import functools

import numpy as np
import pytest

import chan_contract as cc
import demod_contract as dc
import zoom_contract as zc
from topdogspectrumanalyser_amd.channelizer import Channelizer
from topdogspectrumanalyser_amd.demod import Demodulator
from topdogspectrumanalyser_amd.zoom import DownConverter, design_decimator

pytestmark = pytest.mark.gpu

FS = 20e6
FI = 312.5e3
NAN, INF = float("nan"), float("inf")
BAD = [complex(NAN, NAN), complex(NAN, 0.1), complex(INF, 0.0)]
BAD_IDS = ["nan-nan", "nan-re", "inf-re"]


def _noise(rng, shape):
    return (0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)


def _positions(D, tile):
    """Sample 0, the middle of the second tile of outputs, the input that completes the first tile's last output."""
    return [0, (tile + tile // 2) * D + D // 2, (tile - 1) * D]


def _splits(n, n_star, D):
    """One call; and a call that ends with x[n*], pieces shorter than D behind it, then the rest."""
    cut = [n_star + 1] + [k for k in (1, D - 1, 1, max(1, D // 2)) if k > 0]
    assert sum(cut) < n and all(k < D or D == 1 for k in cut[1:])
    return [[n], cut + [n - sum(cut)]]


def _cut(x, pieces):
    edges = np.cumsum([0] + list(pieces))
    assert edges[-1] == x.shape[-1]
    return [x[..., a:b] for a, b in zip(edges[:-1], edges[1:])]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {np.dtype(np.complex64): np.uint64, np.dtype(np.float32): np.uint32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(word), b.view(word))


def _check(y_bad, y_twin, inside, hit, what):
    """[..., n_out] outputs of the stream and its twin: the twin's bits outside the padded windows, non-finite at the
    hit outputs."""
    assert np.all(np.isfinite(y_twin)), what
    outside = np.ones(y_twin.shape[-1], bool)
    outside[inside] = False
    assert hit.size and not np.any(outside[hit]), what
    assert _same_bits(y_bad[..., outside], y_twin[..., outside]), what
    assert not np.any(np.isfinite(y_bad[..., hit])), what


# ---- the down-converter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
def test_down_converter(bad):
    D, T = 13, 3 * 13 + 1
    H, tile = -(-T // D) * D, 2048 // zc.lanes(D)
    rng = np.random.default_rng(130)
    h = rng.choice(np.r_[-7:0, 1:8], T).astype(np.float32) / np.float32(16 * D)        # no zero tap
    n_out = 3 * tile + tile // 3
    n = (n_out - 1) * D + 1 + D // 3
    x = _noise(rng, n)
    with DownConverter(D, FS, 0.19 * FS, taps=h, max_host_samples=n) as ddc:
        def run(v, pieces):
            ddc.reset()
            return np.concatenate([ddc.process(p) for p in _cut(v, pieces)])

        whole = run(x, [n])
        assert whole.size == n_out
        for n_star in _positions(D, tile):
            xb = x.copy()
            xb[n_star] = bad
            inside, hit = zc.padded_window_outputs(n_star, H, D, n_out), zc.hit_outputs(n_star, h, D, n_out)
            assert inside.size == H // D and hit.size == -(-(T - (-n_star) % D) // D)
            for pieces in _splits(n, n_star, D):
                twin = run(x, pieces)
                assert _same_bits(twin, whole)
                _check(run(xb, pieces), twin, inside, hit, (n_star, len(pieces)))


# ---- the channelizer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
@pytest.mark.parametrize("M,os_,T", [(16, 2, 3 * 16 - 5), (64, 1, 34 * 64)], ids=["M16-os2-T43", "M64-os1-default"])
def test_channelizer(M, os_, T, bad):
    D, tile = M // os_, 2048 // M
    P = cc.branch_taps(T, M)
    H = P * M
    rng = np.random.default_rng(1200 + M)
    h = np.ascontiguousarray(design_decimator(M, taps_per_phase=P)[:T])
    n_out = 3 * tile + max(1, tile // 3)
    n = (n_out - 1) * D + 1 + D // 3
    x = _noise(rng, n)
    with Channelizer(M, FS, os_, taps=h, max_host_samples=n) as bank:
        def run(v, pieces, branches=False):
            bank.reset()
            return np.concatenate([bank.process(p, branches=branches) for p in _cut(v, pieces)], axis=1)

        whole = run(x, [n])
        assert whole.shape == (M, n_out)
        for n_star in _positions(D, tile):
            xb = x.copy()
            xb[n_star] = bad
            inside, hit = cc.padded_window_outputs(n_star, H, D, n_out), cc.hit_outputs(n_star, h, D, n_out)
            assert inside.size == H // D
            for pieces in _splits(n, n_star, D):
                twin = run(x, pieces)
                assert _same_bits(twin, whole)
                _check(run(xb, pieces), twin, inside, hit, (n_star, len(pieces)))      # every channel of the instants
        # the first stage alone: the sample sits in ONE branch of an instant, the others keep the twin's bits
        n_star = _positions(D, tile)[1]
        xb = x.copy()
        xb[n_star] = bad
        Wb, Wt = run(xb, [n], branches=True), run(x, [n], branches=True)
        differ = np.nonzero(Wb.view(np.uint64) != Wt.view(np.uint64))
        assert np.all(differ[0] == (-n_star) % M)                    # r = (mD - n*) mod M lands at p = (r - mD) mod M
        assert np.all(np.isin(cc.hit_outputs(n_star, h, D, n_out), differ[1]))
        assert np.all(np.isin(differ[1], cc.padded_window_outputs(n_star, H, D, n_out)))
        assert not np.any(np.isfinite(Wb[differ]))


# ---- the demodulator -------------------------------------------------------------------------------------------------
def _demod_sets(n_star, mode, g, R, n_out):
    Q = -(-g.size // R)
    at = dc.bad_discriminator_values(n_star, mode)
    inside = np.unique(np.concatenate([zc.padded_window_outputs(k, Q * R, R, n_out) for k in at]))
    hit = np.unique(np.concatenate([zc.hit_outputs(k, g, R, n_out) for k in at]))
    return inside, hit


@functools.lru_cache(maxsize=None)
def _demod_case(R, T):
    rng = np.random.default_rng(1300 + R)
    n_out = 3 * dc.TILE + 85
    n = (n_out - 1) * R + 1 + R // 3
    x = _noise(rng, (3, n))
    g = rng.choice(np.r_[-7:0, 1:8], T).astype(np.float32) / np.float32(8 * R)         # no zero tap
    for a in (x, g):
        a.setflags(write=False)
    return x, g, n, n_out


@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
@pytest.mark.parametrize("name,mode", [("fm", dc.FM), ("am", dc.AM)])
@pytest.mark.parametrize("R,T", [(3, 8), (12, 96)], ids=["R3-T8", "R12-T96"])
def test_demodulator(R, T, name, mode, bad):
    x, g, n, n_out = _demod_case(R, T)
    with Demodulator(name, FI, R, 3, taps=g, max_host_samples=3 * n) as dm:
        def run(v, pieces):
            dm.reset()
            return np.concatenate([dm.process(p) for p in _cut(v, pieces)], axis=1)

        whole = run(x, [n])
        assert whole.shape == (3, n_out)
        for n_star in _positions(R, dc.TILE):
            xb = x.copy()
            xb[1, n_star] = bad                                      # channel 1 only
            inside, hit = _demod_sets(n_star, mode, g, R, n_out)
            for pieces in _splits(n, n_star, R):
                twin = run(x, pieces)
                assert _same_bits(twin, whole)
                got = run(xb, pieces)
                assert _same_bits(got[[0, 2]], twin[[0, 2]]), (n_star, len(pieces))    # the others never see it
                _check(got[1], twin[1], inside, hit, (n_star, len(pieces)))


@pytest.mark.parametrize("bad", [BAD[0], BAD[2]], ids=[BAD_IDS[0], BAD_IDS[2]])
@pytest.mark.parametrize("name,mode,pole_mode", [("fm", dc.FM, dc.POLE_LOW), ("am", dc.AM, dc.POLE_HIGH)])
def test_demodulator_pole_and_measurements_keep_it_until_reset(name, mode, pole_mode, bad):
    R, T, c = 3, 8, 0.757
    x, g, n, n_out = _demod_case(R, T)
    n_star = _positions(R, dc.TILE)[1]
    xb = x.copy()
    xb[1, n_star] = bad
    x2 = _noise(np.random.default_rng(1399), (3, 100 * R))
    inside, hit = _demod_sets(n_star, mode, g, R, n_out)
    first = int(inside[0])
    assert first == hit[0] and 64 < first % 256 and first % dc.POLE_BLOCK          # inside a pole block

    def run(dm, v):
        """The block, its measurements; then, the accumulators restarted, a finite block and its measurements."""
        y, m = dm.process(v), dm.measure()
        dm.reset_measure()
        y2, m2 = dm.process(x2), dm.measure()
        return y, m, y2, m2

    with Demodulator(name, FI, R, 3, taps=g, max_host_samples=3 * n) as plain:
        a_bad = plain.process(xb)                                    # a[m] itself: pole off, scale 1
    with Demodulator(name, FI, R, 3, taps=g, max_host_samples=3 * n) as dm:
        dm.set_pole(pole_mode, c)
        ty, tm, ty2, tm2 = run(dm, x)                                # the twin
        dm.reset()
        y, m, y2, m2 = run(dm, xb)
        # audio: the other channels and everything before the window as the twin; from the first hit on, non-finite
        assert _same_bits(y[[0, 2]], ty[[0, 2]]) and _same_bits(y2[[0, 2]], ty2[[0, 2]])
        assert _same_bits(y[1, :first], ty[1, :first])
        assert not np.any(np.isfinite(y[1, first:])) and not np.any(np.isfinite(y2[1]))
        # measurements over a[m]: count counts it, max and min skip a NaN, the sums keep it ...
        assert np.array_equal(m.count, tm.count) and np.all(m.count == n_out)
        for f in ("max", "min", "sum", "sumsq"):
            assert np.array_equal(getattr(m, f)[[0, 2]], getattr(tm, f)[[0, 2]]), f
        with np.errstate(invalid="ignore", over="ignore"):
            _, mx, mn, s, ss = dc.measurements(a_bad[1].astype(np.float64))
        assert not np.isfinite(m.sum[1]) and not np.isfinite(m.sumsq[1])
        assert not np.isfinite(s[0]) and not np.isfinite(ss[0])
        assert float(m.max[1]) == mx[0] and float(m.min[1]) == mn[0]
        # ... until reset_measure(): a[m] of the next block is finite again, whatever the pole still holds
        for f in ("count", "max", "min", "sum", "sumsq"):
            assert np.array_equal(getattr(m2, f), getattr(tm2, f)), f
        # and reset() gives the bits of a fresh handle
        dm.reset()
        again = dm.process(x)
        assert _same_bits(again, ty)
        ma = dm.measure()
        for f in ("count", "max", "min", "sum", "sumsq"):
            assert np.array_equal(getattr(ma, f), getattr(tm, f)), f
