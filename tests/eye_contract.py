"""The eye diagrams' contract in numpy: what tdsa_eye_* computes.  Positions and phases are
integers (32.32 fixed point, turns / 2^32) as in symsync_contract.py, whose resampler and rotation this file shares, and
the series of the FM and REAL kinds are fsk_contract.py's stages 0 and 1.  The traces are float64 here and float32 on
the device, held together by the two files' bounds; the rows are defined in float32 operation by operation and restated
exactly, so that from the same traces this file gives the device's counts bit for bit."""
import numpy as np

import fsk_contract as fc
import symsync_contract as sc
from symsync_contract import MASK, ONE, U, step_of  # noqa: F401

IQ, FM, REAL = 0, 1, 2
POINTS = (4, 8, 16, 32, 64)
MIN_ROWS, MAX_ROWS, MAX_BINS = 8, 256, 8192
MIN_SYMBOLS, MAX_SYMBOLS = 3, 4096
F32 = np.float32
UNDER, OVER, NAN = -1, -2, -3          # what rows_of gives a value outside the image


# ---- parameters -------------------------------------------------------------------------------------------------------
def eyes(kind: int) -> int:
    return 2 if kind == IQ else 1


def series_len(seg_len: int, kind: int, B: int) -> int:
    """n: seg_len (IQ), seg_len - B (FM), seg_len - B + 1 (REAL)."""
    return int(seg_len) if kind == IQ else fc.boxcar_outputs(seg_len, fc.IQ if kind == FM else fc.FREQ, B)


def symbols_per_segment(step: int, seg_len: int, kind: int, B: int) -> int:
    """K, the producer's own formula."""
    if kind == IQ:
        return sc.symbols_per_segment(step, seg_len)
    return fc.symbols_per_segment(step, seg_len, fc.IQ if kind == FM else fc.FREQ, B)


def series(x, kind: int, B: int):
    """The series the traces are read from, float64 (complex128 for IQ)."""
    if kind == IQ:
        return np.asarray(x, dtype=np.complex128)
    d = fc.discriminate(x) if kind == FM else np.asarray(x, dtype=np.float64)
    return fc.boxcar(d, B)


def series32_real(x, B: int):
    """The device's series of the REAL kind, bit for bit: fsk_contract.boxcar32."""
    return fc.boxcar32(np.asarray(x, dtype=F32), B)


# ---- points -----------------------------------------------------------------------------------------------------------
def column_offsets(step: int, P: int):
    """floor((c - P / 2) step / P), c < P: Python's // floors the signed product as the arithmetic shift does."""
    return [((c - P // 2) * int(step)) // P for c in range(P)]


def positions(delta_fx: int, step: int, K: int, P: int):
    """(i, mu) of the points, [K - 2][P] each: symbols k = 1 .. K - 2, columns c < P."""
    off = column_offsets(step, P)
    pos = [[int(delta_fx) + k * int(step) + off[c] for c in range(P)] for k in range(1, K - 1)]
    i = np.array([[p >> 32 for p in row] for row in pos], dtype=np.int64).reshape(K - 2, P)
    mu = np.array([[(p & MASK) >> 8 for p in row] for row in pos], dtype=np.float64).reshape(K - 2, P) * 2.0 ** -24
    return i, mu


def tap_range(delta_fx: int, step: int, K: int, P: int):
    """(lowest, highest) index of the series any point reads."""
    i, _ = positions(delta_fx, step, K, P)
    return int(i.min()) - 1, int(i.max()) + 2


def phases(theta_fx: int, step_f: int, K: int, P: int):
    """phi [K - 2][P] uint64 below 2^32: theta_fx + k step_f + floor((c - P / 2) int32(step_f) / P) mod 2^32."""
    sf = int(step_f) & MASK
    signed = sf - ONE if sf >= ONE // 2 else sf
    off = [((c - P // 2) * signed) // P for c in range(P)]
    return np.array([[(int(theta_fx) + k * sf + off[c]) & MASK for c in range(P)] for k in range(1, K - 1)],
                    dtype=np.uint64).reshape(K - 2, P)


def interpolate(s, delta_fx: int, step: int, K: int, P: int, with_bound: bool = False):
    """The cubic Lagrange interpolation of the series s at the points, float64 [K - 2][P]; with_bound also
    sum |c| |taps| (per part: the larger of re and im) and sum |c|."""
    s = np.asarray(s)
    i, mu = positions(delta_fx, step, K, P)
    c = sc.coeffs(mu)
    taps = np.stack([s[i - 1], s[i], s[i + 1], s[i + 2]])
    with np.errstate(invalid="ignore"):
        y = np.sum(c * taps, axis=0)
    if not with_bound:
        return y
    a = np.maximum(np.abs(taps.real), np.abs(taps.imag)) if np.iscomplexobj(taps) else np.abs(taps)
    return y, np.sum(np.abs(c) * a, axis=0), np.sum(np.abs(c), axis=0)


def derotate(y, theta_fx: int, step_f: int):
    """v = y exp(-2 pi i phi / 2^32) at the points' phases."""
    K2, P = np.asarray(y).shape
    phi = phases(theta_fx, step_f, K2 + 2, P)
    return np.asarray(y, dtype=np.complex128) * np.exp(-2j * np.pi * phi.astype(np.float64) / ONE)


def traces(x, kind: int, B: int, step: int, P: int, clock, K=None):
    """One segment's traces in float64, [K - 2][P] (complex128 for IQ): clock = (delta_fx, step_f, theta_fx)."""
    K = symbols_per_segment(step, len(x), kind, B) if K is None else K
    y = interpolate(series(x, kind, B), clock[0], step, K, P)
    return derotate(y, clock[2], clock[1]) if kind == IQ else y


# ---- how far float32 may stand from the traces ------------------------------------------------------------------------
# No tolerance of this file's own: the resampler's and the rotation's bounds are symsync_contract's, the boxcar's and
# the discriminator's fsk_contract's.  The rotation's argument is an integer on both sides.
def iq_bound(y, mag):
    """|v_dev - v| of the IQ traces as complex numbers: the resampler's error per part (as a vector at most sqrt 2 of
    it), which a rotation of modulus one carries unchanged, and the rotation's and the product's own on the device's y."""
    return np.sqrt(2.0) * sc.resample_bound(mag) * 1.01 + sc.derotate_bound(np.abs(y) + np.sqrt(2.0) * sc.resample_bound(mag))


def real_bound(mag, sumc, absd_mean: float, kind: int, B: int):
    """|v_dev - v| of the FM and REAL traces: fsk_contract.resample_bound over the boxcar's own error."""
    return fc.resample_bound(mag, sumc, fc.boxcar_bound(absd_mean, fc.IQ if kind == FM else fc.FREQ, B))


# ---- rows, exactly -----------------------------------------------------------------------------------------------------
def scale_of(H: int, lo, hi) -> np.float32:
    """float32(double(H) / (double(hi) - double(lo))) of a float32 range."""
    return F32(float(H) / (float(F32(hi)) - float(F32(lo))))


def rows_of(v, lo, hi, H: int):
    """The row of every float32 value, or UNDER, OVER, NAN: t = (v - lo) * scale in float32, two roundings."""
    v = np.asarray(v, dtype=F32)
    scale = scale_of(H, lo, hi)
    with np.errstate(all="ignore"):
        t = ((v - F32(lo)).astype(F32) * scale).astype(F32)
        row = np.where(np.isnan(t), NAN, np.where(t < 0, UNDER, np.where(t >= F32(H), OVER, 0))).astype(np.int64)
        inside = row == 0
        row[inside] = t[inside].astype(np.int64)
    return row


def bin_traces(tr, lo, hi, H: int):
    """counts [eyes][H][P] uint64 and totals [eyes][4] uint64 = {n_points, n_under, n_over, n_nan} of float32 (or
    complex64: two eyes) traces [...][P]."""
    tr = np.asarray(tr)
    P = tr.shape[-1]
    parts = [tr.real, tr.imag] if np.iscomplexobj(tr) else [tr]
    counts = np.zeros((len(parts), H, P), dtype=np.uint64)
    totals = np.zeros((len(parts), 4), dtype=np.uint64)
    for e, part in enumerate(parts):
        row = rows_of(part.reshape(-1, P), lo, hi, H)
        col = np.broadcast_to(np.arange(P), row.shape)
        ok = row >= 0
        np.add.at(counts[e], (row[ok], col[ok]), 1)
        totals[e] = [row.size, np.count_nonzero(row == UNDER), np.count_nonzero(row == OVER), np.count_nonzero(row == NAN)]
    return counts, totals


def invariant(counts, totals, segments: int, skipped: int, K: int, P: int) -> bool:
    """sum counts + under + over + nan = n_points = (segments - skipped) (K - 2) P, per eye."""
    n = (int(segments) - int(skipped)) * (K - 2) * P
    return all(int(counts[e].sum()) + int(totals[e][1:].sum()) == int(totals[e][0]) == n for e in range(counts.shape[0]))


# ---- the opening, from the integers ------------------------------------------------------------------------------------
def row_of(value: float, lo, hi, H: int) -> int:
    t = (float(value) - float(lo)) * (H / (float(hi) - float(lo)))
    return int(min(max(np.floor(t), 0), H - 1))


def opening(img, lo, hi, threshold: float):
    """(height, width) of one eye's counts [H][P] around `threshold`."""
    img = np.asarray(img)
    H, P = img.shape
    r, mid = row_of(threshold, lo, hi, H), P // 2
    if img[r, mid]:
        return 0.0, 0.0
    top = next((q for q in range(r + 1, H) if img[q, mid]), H)
    bottom = next((q for q in range(r - 1, -1, -1) if img[q, mid]), -1)
    left = next((n for n in range(mid) if img[r, mid - 1 - n]), mid)
    right = next((n for n in range(P - mid - 1) if img[r, mid + 1 + n]), P - mid - 1)
    return (top - bottom - 1) * (float(hi) - float(lo)) / H, (1 + left + right) / P
