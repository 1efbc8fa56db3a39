"""The eye diagrams without a device: the contract alone (tests/eye_contract.py) on the signals of the two producers'
contracts, the EyeImage helpers on hand-made count arrays, the ValueErrors of the Python layer that come before any
device is touched, and the text of every -1 of tdsa_eye_* that needs no live handle."""
import ctypes as C

import numpy as np
import pytest

import eye_contract as ec
import fsk_contract as fc
import symsync_contract as sc
from topdogspectrumanalyser_amd import _native as nat
from topdogspectrumanalyser_amd import eye as ey

ONE = 1 << 32
SPS = (4, 4.37, 8, 33.3, 64)
POINTS = (4, 16, 64)
lib = nat.lib


# ---- the contract alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fsk_segments():
    """Per sps: (x, K, delta_fx, b, v) of a GFSK segment (BT = 0.5) of some 40 symbols, B = default."""
    out = {}
    for sps in SPS:
        n = int(44 * sps) + 8
        x, _, _ = fc.make_fsk(2, sps, n, 0.5, bt=0.5, seed=3)
        a = fc.analyse(x, sps, 2)
        out[sps] = (x, a["K"], a["delta_fx"], a["b"], a["v"], a["B"])
    return out


@pytest.fixture(scope="module")
def qpsk_segments():
    out = {}
    for sps in SPS:
        n = int(44 * sps) + 8
        x, _, _ = sc.make_signal("qpsk", sps, n, seed=3)
        out[sps] = (x, sc.recover(x, sps, 4))
    return out


@pytest.mark.parametrize("P", POINTS)
@pytest.mark.parametrize("sps", SPS)
def test_every_tap_lies_inside_the_series_at_the_extreme_clocks(sps, P):
    step = sc.step_of(sps)
    for kind, B in ((ec.IQ, 1), (ec.FM, 1), (ec.FM, 64), (ec.REAL, 1), (ec.REAL, 7)):
        for K in (3, 4, 57):
            # the shortest segment that gives K symbols
            seg = next(n for n in range(8, 70 * 66) if ec.symbols_per_segment(step, n, kind, B) == K)
            n = ec.series_len(seg, kind, B)
            for delta in (ONE, ONE + 1, step + ONE - 1, ONE + step // 2):
                lo, hi = ec.tap_range(delta, step, K, P)
                assert 0 <= lo and hi <= n - 1, (kind, B, K, delta, lo, hi, n)


@pytest.mark.parametrize("P", POINTS)
@pytest.mark.parametrize("sps", SPS)
def test_the_centre_column_is_the_producers_symbols(sps, P, fsk_segments, qpsk_segments):
    step = sc.step_of(sps)
    x, K, delta, b, v, B = fsk_segments[sps]
    tr = ec.traces(x, ec.FM, B, step, P, (delta, 0, 0))
    assert tr.shape == (K - 2, P)
    assert np.array_equal(tr[:, P // 2], fc.resample(b, delta, step, K)[1:K - 1])
    x, r = qpsk_segments[sps]
    K = r["K"]
    tr = ec.traces(x, ec.IQ, 1, step, P, (r["delta_fx"], r["step_f"], r["theta_fx"]))
    want = sc.derotate(sc.resample(x, r["delta_fx"], step, K), r["step_f"], r["theta_fx"])[1:K - 1]
    assert np.array_equal(tr[:, P // 2], want)
    # a step_f that is negative as int32 turns the columns left of the centre forwards
    neg = ec.phases(5, ONE - 4 * P, K, P)
    assert int(neg[0, 0]) == (5 + (ONE - 4 * P) + 2 * P) & sc.MASK and int(neg[0, P // 2]) == (5 + ONE - 4 * P) & sc.MASK


@pytest.mark.parametrize("P", POINTS)
@pytest.mark.parametrize("sps", SPS)
def test_the_invariant_holds_with_values_outside_the_range(sps, P, fsk_segments):
    x, K, delta, b, v, B = fsk_segments[sps]
    tr = ec.traces(x, ec.FM, B, sc.step_of(sps), P, (delta, 0, 0)).astype(np.float32)
    mid, top = float(np.median(v)), float(np.max(v))
    lo, hi = np.float32(mid), np.float32(mid + 0.5 * (top - mid))   # half of the eye is under, some of it over
    tr[0, 0], tr[1, 1] = np.nan, np.inf
    counts, totals = ec.bin_traces(tr, lo, hi, 17)
    assert ec.invariant(counts, totals, 1, 0, K, P)
    assert totals[0][3] == 1 and totals[0][2] >= 1 and totals[0][1] >= 1
    both, t2 = ec.bin_traces(np.stack([tr, tr]), lo, hi, 17)
    assert np.array_equal(both, 2 * counts) and ec.invariant(both, t2, 3, 1, K, P)


@pytest.mark.parametrize("sps", (4, 8, 33.3))
def test_the_opening_is_there_at_40_db_and_no_larger_at_25_db(sps):
    step, P, H = sc.step_of(sps), 16, 64
    n = int(300 * sps) + 8

    def fsk_opening(noise_db):
        x, _, _ = fc.make_fsk(2, sps, n, 0.5, bt=0.5, seed=5, noise_db=noise_db)
        a = fc.analyse(x, sps, 2)
        tr = ec.traces(x, ec.FM, a["B"], step, P, (a["delta_fx"], 0, 0)).astype(np.float32)
        span = 2.0 * float(a["dev"])
        lo, hi = np.float32(float(a["offset"]) - span), np.float32(float(a["offset"]) + span)
        return ec.opening(ec.bin_traces(tr, lo, hi, H)[0][0], lo, hi, float(a["offset"]))

    def qpsk_opening(noise_db):
        x, _, _ = sc.make_signal("qpsk", sps, n, seed=5, noise_db=noise_db)
        r = sc.recover(x, sps, 4, ref_arg=sc.reference_phase(sc.points("qpsk"), 4))      # the points off the axes
        tr = ec.traces(x, ec.IQ, 1, step, P, (r["delta_fx"], r["step_f"], r["theta_fx"])).astype(np.complex64)
        return ec.opening(ec.bin_traces(tr, -1.5, 1.5, H)[0][0], -1.5, 1.5, 0.0)

    for opening in (fsk_opening, qpsk_opening):
        clean, noisy = opening(-40.0), opening(-25.0)
        assert clean[0] > 0 and clean[1] > 0, clean
        assert noisy[0] <= clean[0] and noisy[1] <= clean[1], (clean, noisy)


def test_rows_are_two_float32_roundings():
    lo, hi, H = np.float32(-0.3), np.float32(1.1), 17
    scale = ec.scale_of(H, lo, hi)
    assert scale == np.float32(17.0 / (float(hi) - float(lo))) and scale.dtype == np.float32
    v = np.array([lo, hi, np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(-2)), -0.0, np.inf, -np.inf, np.nan,
                  1e-45, 3.4e38, -3.4e38], dtype=np.float32)
    rows = ec.rows_of(v, lo, hi, H)
    assert rows[0] == 0 and rows[1] == ec.OVER and rows[2] == ec.UNDER and rows[3] in (H - 1, ec.OVER)
    assert list(rows[5:8]) == [ec.OVER, ec.UNDER, ec.NAN] and rows[9] == ec.OVER and rows[10] == ec.UNDER
    assert rows[4] == rows[8] == int(np.float32(np.float32(0.3) * scale))


# ---- EyeImage ------------------------------------------------------------------------------------------------------------
def image(counts, lo=-1.0, hi=1.0):
    counts = np.asarray(counts, dtype=np.uint64)
    counts = counts[None] if counts.ndim == 2 else counts
    totals = np.zeros(10, dtype=np.uint64)
    for e in range(counts.shape[0]):
        totals[4 * e] = counts[e].sum()
    totals[8] = 1
    return ey.image_from(counts, totals, lo, hi)


def test_opening_of_hand_made_images():
    H, P = 9, 8                                          # H odd: the threshold 0 lies in the middle row, 4
    c = np.zeros((H, P), dtype=np.uint64)
    c[1, :] = 3
    c[7, :] = 2
    c[4, 0] = c[4, 7] = 1                                # the crossings, at the edges of the symbol
    img = image(c, -0.9, 0.9)
    assert img.row_of(0.0) == 4 and img.row_of(-5.0) == 0 and img.row_of(5.0) == 8 and img.row_of(0.9) == 8
    h, w = img.opening(0.0)
    assert h == pytest.approx(5 * 1.8 / 9) and w == (1 + 3 + 2) / 8          # left 3, 2, 1; right 5, 6
    assert (h, w) == ec.opening(c, -0.9, 0.9, 0.0)
    # wrap-free: an empty row counts to the edges and no further
    c[4, 0] = c[4, 7] = 0
    assert image(c, -0.9, 0.9).opening(0.0) == (pytest.approx(1.0), 1.0) == ec.opening(c, -0.9, 0.9, 0.0)
    # left and right on their own
    c[4, 2] = 1
    assert image(c, -0.9, 0.9).opening(0.0)[1] == (1 + 1 + 3) / 8
    c[4, 2], c[4, 5] = 0, 1
    assert image(c, -0.9, 0.9).opening(0.0)[1] == (1 + 4 + 0) / 8
    # a one-row gap
    c[:] = 0
    c[3, 4] = c[5, 4] = 1
    assert image(c, -0.9, 0.9).opening(0.0)[0] == pytest.approx(1.8 / 9)
    # an occupied centre
    c[4, 4] = 1
    assert image(c, -0.9, 0.9).opening(0.0) == (0.0, 0.0) == ec.opening(c, -0.9, 0.9, 0.0)
    # nothing above or below: the image's edges
    c[:] = 0
    assert image(c, -0.9, 0.9).opening(0.0) == (pytest.approx(1.8), 1.0)


def test_views_and_thresholds_of_an_image():
    c = np.arange(2 * 8 * 4, dtype=np.uint64).reshape(2, 8, 4)
    img = image(c)
    assert (img.rows, img.points) == (8, 4)
    two = img.two_symbols()
    assert two.shape == (2, 8, 8) and np.array_equal(two[:, :, :4], c) and np.array_equal(two[:, :, 4:], c)
    d = img.density()
    assert d.dtype == np.float64 and np.allclose(d.sum(axis=(1, 2)), 1.0) and d[1, 7, 3] == 63 / c[1].sum()
    assert np.array_equal(image(np.zeros((8, 4))).density(), np.zeros((1, 8, 4)))
    assert np.allclose(ey.EyeImage.thresholds_from((0.1, 0.05, 4)), [0.0, 0.1, 0.2])
    assert np.allclose(ey.EyeImage.thresholds_from((0.0, 0.25, 2)), [0.0])


# ---- ValueErrors before any device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, text", [
    (dict(points=12), "points=12: 4, 8, 16, 32 or 64"),
    (dict(points=128), "points=128: 4, 8, 16, 32 or 64"),
    (dict(points=64, rows=129), "points=64 x rows=129 = 8256 bins: at most 8192"),
    (dict(rows=7), "rows=7: 8 .. 256"),
    (dict(rows=257), "rows=257: 8 .. 256"),
    (dict(v_range=(1.0, 1.0)), "lo < hi"),
    (dict(v_range=(2.0, 1.0)), "lo < hi"),
    (dict(v_range=(0.0, float("inf"))), "finite float32"),
    (dict(v_range=(float("nan"), 1.0)), "finite float32"),
    (dict(v_range=(0.0, 1e39)), "finite float32"),
    (dict(samples_per_symbol=3.9), "samples_per_symbol=3.9: 4 .. 64"),
    (dict(input="freq"), "input='freq': 'iq', 'fm' or 'real'"),
    (dict(boxcar=65), "boxcar=65: 1 .. 64"),
])
def test_the_constructor_refuses_before_it_touches_a_device(kw, text):
    args = dict(samples_per_symbol=8, device=1 << 20)          # a device that does not exist: never reached
    args.update(kw)
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("..", r"\.\.")):
        ey.EyeDiagram(**args)


def test_k_and_clocks_are_checked_on_the_host():
    step = 8 * ONE
    assert ey.symbols_per_segment(step, 44, nat.EYE_IQ, 1) == sc.symbols_per_segment(step, 44) == 4
    assert ey.symbols_per_segment(step, 44, nat.EYE_FM, 4) == fc.symbols_per_segment(step, 44, fc.IQ, 4)
    assert ey.symbols_per_segment(step, 44, nat.EYE_REAL, 4) == fc.symbols_per_segment(step, 44, fc.FREQ, 4)
    assert ey.checked_symbols(step, 36, nat.EYE_IQ, 1) == 3
    with pytest.raises(ValueError, match=r"seg_len=35 gives 2 symbols per segment: 3 \.\. 4096"):
        ey.checked_symbols(step, 35, nat.EYE_IQ, 1)
    with pytest.raises(ValueError, match=r"symbols per segment: 3 \.\. 4096"):
        ey.checked_symbols(step, 8 * 4200, nat.EYE_IQ, 1)
    ck = ey.clock_array(step, delta=1.0, n_seg=3)
    assert ck.dtype == ey.CLOCK and list(ck["delta_fx"]) == [ONE] * 3 and not ck["step_f"].any()
    for bad in (0.999, 9.0):
        with pytest.raises(ValueError, match="1 <= delta < samples_per_symbol"):
            ey.clock_array(step, delta=bad)
    rec = np.zeros(3, dtype=[("delta_fx", np.uint64), ("step_f", np.uint32), ("theta_fx", np.uint32), ("flags", np.uint32)])
    rec["delta_fx"] = [ONE, 5 * ONE, step + ONE - 1]
    rec["step_f"], rec["theta_fx"], rec["flags"] = [1, 2, 3], [4, 5, 6], [0, 1, 2]
    ck = ey.clock_array(step, rec)
    assert list(ck["delta_fx"]) == [ONE, 0, step + ONE - 1] and list(ck["step_f"]) == [1, 2, 3] and list(ck["theta_fx"]) == [4, 5, 6]
    rec["delta_fx"][2] = step + ONE
    with pytest.raises(ValueError, match=rf"clock of segment 2: delta_fx={step + ONE}: 0 \(skip\) or 2\^32 <= delta_fx < step \+ 2\^32"):
        ey.clock_array(step, rec)
    fsk_rec = np.zeros(2, dtype=[("delta_fx", np.uint64), ("flags", np.uint32)])
    fsk_rec["delta_fx"] = [2 * ONE, ONE - 1]
    with pytest.raises(ValueError, match="clock of segment 1"):
        ey.clock_array(step, fsk_rec)
    with pytest.raises(ValueError, match="either a result or delta="):
        ey.clock_array(step)


# ---- every -1 that needs no live handle -----------------------------------------------------------------------------------
BUF = (C.c_ubyte * 256)()
HND = C.c_void_p()
N = C.c_int(0)
STEP_RANGE = "4 .. 64 samples per symbol in 32.32 fixed point"
EYE_OK = (4 * ONE, 0, 1, 32, 128, -1.0, 1.0)            # step, kind, boxcar, points, rows, lo, hi
WHO = "null eye diagram handle"

CASES = [
    ("tdsa_eye_create", (0, 4096, 16, None), "null out"),
    ("tdsa_eye_create", (0, 8, 16, C.byref(HND)), "max_host_samples=8: at least 16"),
    ("tdsa_eye_create", (0, 4096, 0, C.byref(HND)), "max_segments=0: at least 1"),
    ("tdsa_eye_configure", (None, 4 * ONE - 1) + EYE_OK[1:], f"step={4 * ONE - 1}: {STEP_RANGE}"),
    ("tdsa_eye_configure", (None, 64 * ONE + 1) + EYE_OK[1:], f"step={64 * ONE + 1}: {STEP_RANGE}"),
    ("tdsa_eye_configure", (None, 4 * ONE, 3, 1, 32, 128, -1.0, 1.0), "kind=3: TDSA_EYE_IQ, _FM or _REAL"),
    ("tdsa_eye_configure", (None, 4 * ONE, 1, 0, 32, 128, -1.0, 1.0), "boxcar=0: 1 .. 64 samples"),
    ("tdsa_eye_configure", (None, 4 * ONE, 1, 65, 32, 128, -1.0, 1.0), "boxcar=65: 1 .. 64 samples"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 2, 128, -1.0, 1.0), "points=2: 4, 8, 16, 32 or 64 per symbol"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 12, 128, -1.0, 1.0), "points=12: 4, 8, 16, 32 or 64 per symbol"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 128, 8, -1.0, 1.0), "points=128: 4, 8, 16, 32 or 64 per symbol"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 7, -1.0, 1.0), "rows=7: 8 .. 256"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 257, -1.0, 1.0), "rows=257: 8 .. 256"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 64, 129, -1.0, 1.0), "points=64 x rows=129 = 8256 bins: at most 8192"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 128, 1.0, 1.0), "range 1 .. 1: finite, lo < hi"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 128, 1.0, -1.0), "range 1 .. -1: finite, lo < hi"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 128, float("-inf"), 1.0), "range -inf .. 1: finite, lo < hi"),
    ("tdsa_eye_configure", (None, 4 * ONE, 0, 1, 32, 128, 0.0, float("nan")), "range 0 .. nan: finite, lo < hi"),
    ("tdsa_eye_configure", (None,) + EYE_OK, WHO),
    ("tdsa_eye_symbols_per_segment", (4 * ONE, 100, 0, 1, None), "null K"),
    ("tdsa_eye_symbols_per_segment", (64 * ONE + 1, 100, 0, 1, C.byref(N)), f"step={64 * ONE + 1}: {STEP_RANGE}"),
    ("tdsa_eye_symbols_per_segment", (4 * ONE, 100, -1, 1, C.byref(N)), "kind=-1: TDSA_EYE_IQ, _FM or _REAL"),
    ("tdsa_eye_symbols_per_segment", (4 * ONE, 100, 1, 65, C.byref(N)), "boxcar=65: 1 .. 64 samples"),
    ("tdsa_eye_process", (None, BUF, 100, 100, 100, 1, BUF, None), WHO),
    ("tdsa_eye_process", (None, None, 0, 0, 0, 0, None, None), WHO),
    ("tdsa_eye_process_dev", (None, None, BUF, 100, 100, 1, BUF, None), WHO),
    ("tdsa_eye_process_dev", (None, None, C.c_void_p(4098), 100, 100, 1, BUF, None), WHO),
    ("tdsa_eye_read", (None, BUF, BUF), WHO),
    ("tdsa_eye_reset", (None,), WHO),
    ("tdsa_eye_timer_begin", (None,), WHO),
    ("tdsa_eye_timer_end", (None, None), WHO),
]


@pytest.mark.parametrize("fn, args, text", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_argument_errors_that_need_no_handle(fn, args, text):
    assert getattr(lib, fn)(*args) == -1
    assert lib.tdsa_last_error_string().decode() == text


def test_symbols_per_segment_is_the_producers_own():
    k, kp = C.c_int(), C.c_int()
    for sps in (4, 4.37, 33.3, 64):
        step = sc.step_of(sps)
        for seg in (3, 40, 301, 4096):
            assert lib.tdsa_eye_symbols_per_segment(step, seg, nat.EYE_IQ, 1, C.byref(k)) == 0
            assert lib.tdsa_symsync_symbols_per_segment(step, seg, C.byref(kp)) == 0
            assert k.value == kp.value == max(0, ec.symbols_per_segment(step, seg, ec.IQ, 1))
            for kind, fk in ((nat.EYE_FM, nat.FSK_IQ), (nat.EYE_REAL, nat.FSK_FREQ)):
                for B in (1, 5, 64):
                    assert lib.tdsa_eye_symbols_per_segment(step, seg, kind, B, C.byref(k)) == 0
                    assert lib.tdsa_fsk_symbols_per_segment(step, seg, fk, B, C.byref(kp)) == 0
                    assert k.value == kp.value == max(0, ec.symbols_per_segment(step, seg, kind, B))
