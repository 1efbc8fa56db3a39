"""Vectorised numpy restatement of Constellation2D.update_iq_data (displays/constellation_2d.py:104-160 of the
reference), written with explicit IEEE operations so that it does not depend on which SIMD loops the host's numpy
dispatches to.  It is the CPU yardstick of the device constellation pass:

  rms   = sqrt(mean(|iq|^2)), float32, |.| as numpy's complex64 absolute: L * sqrtf(fmaf(S/L, S/L, 1))
  iq   /= rms when rms > float32(1e-10): re * (1/rms), im * (1/rms) via numpy's complex division
  evm   = sqrt(mean(min over the reference points of fl(fl(i-px)^2 + fl(q-py)^2))) in the table's dtype
  counts[q_bin][i_bin] of histogram2d over float64 linspace(-r, r, bins + 1) edges

Every mean is numpy's add.reduce: a sequential fold from 0 over consecutive 8192-element blocks, each block summed
by the pairwise rule of numpy's pairwise_sum (n < 8 plain loop, n <= 128 eight accumulators, else split).
"""
import numpy as np

BLOCK = 8192
IN_I8, IN_U8, IN_C64 = 0, 1, 2


def reference_points(name):
    """The reference's _CONST_REFS[name] (the same values and dtypes), or None for an unknown name."""
    if name == "bpsk":
        return np.array([[-1.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    if name == "qpsk":
        return np.array([[-1, -1], [-1, 1], [1, -1], [1, 1]], dtype=np.float32) / np.sqrt(2.0)
    if name == "8psk":
        return np.array([[np.cos(a), np.sin(a)] for a in (k * np.pi / 4 for k in range(8))], dtype=np.float32)
    if name in ("16qam", "64qam"):
        side = 4 if name == "16qam" else 8
        lv = np.arange(1 - side, side, 2, dtype=np.float32)
        grid = np.stack([np.repeat(lv, side), np.tile(lv, side)], axis=1)
        return grid / np.sqrt(np.mean(grid[:, 0] ** 2 + grid[:, 1] ** 2))
    return None


def to_complex(raw, fmt):
    """The a1 input conventions: interleaved int8 / uint8 pairs or complex64 -> complex64."""
    if fmt == IN_I8:
        v = np.asarray(raw, dtype=np.int8).astype(np.float32) / np.float32(128.0)
    elif fmt == IN_U8:
        v = (np.asarray(raw, dtype=np.uint8).astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    else:
        return np.asarray(raw).astype(np.complex64)
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)


def _pairwise(a):
    """numpy's pairwise_sum applied to every row of a [rows, n] array at once (rows share n)."""
    n = a.shape[1]
    t = a.dtype.type
    if n < 8:
        res = np.full(a.shape[0], t(-0.0), dtype=a.dtype)
        for i in range(n):
            res = res + a[:, i]
        return res
    if n <= 128:
        r = [a[:, k].copy() for k in range(8)]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] = r[k] + a[:, i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for j in range(i, n):
            res = res + a[:, j]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:, :n2]) + _pairwise(a[:, n2:])


def block_sums(x):
    """Per-8192-block pairwise sums of a 1-D float array, in block order."""
    nfull = len(x) // BLOCK
    parts = []
    if nfull:
        parts.append(_pairwise(x[:nfull * BLOCK].reshape(nfull, BLOCK)))
    if len(x) % BLOCK:
        parts.append(_pairwise(x[nfull * BLOCK:].reshape(1, -1)))
    return np.concatenate(parts) if parts else np.zeros(0, x.dtype)


def np_sum(x):
    """np.add.reduce of a contiguous 1-D float32 / float64 array."""
    acc = x.dtype.type(0)
    for b in block_sums(x):
        acc = x.dtype.type(acc + b)
    return acc


def np_mean(x):
    s = np_sum(x)
    if x.dtype == np.float32:
        return np.float32(np.float64(s) / np.float64(len(x)))
    return np.float64(s / np.float64(len(x)))


def _fmaf_rr1(r):
    """fmaf(r, r, 1) for float32 r in [0, 1] (or NaN), correctly rounded: r*r and 1 + r*r in double are exact up to
    one rounding whose error Fast2Sum recovers; the float32 rounding is fixed up on the midpoints."""
    s = r.astype(np.float64) * r.astype(np.float64)           # exact: 48 significant bits
    t = 1.0 + s
    e = s - (t - 1.0)                                          # exact error of t (|1| >= |s|)
    f = t.astype(np.float32)
    half = np.float64(2.0 ** -24)                              # half an ulp of float32 on [1, 2)
    mid = np.abs(f.astype(np.float64) - t) == half
    up = (t + half).astype(np.float32)
    dn = (t - half).astype(np.float32)
    return np.where(mid & (e > 0), up, np.where(mid & (e < 0), dn, f))


def cabs(iq):
    """numpy 2.x complex64 absolute: inf wins over NaN, NaN over finite, else L * sqrtf(fmaf(S/L, S/L, 1))."""
    re = np.abs(iq.real.astype(np.float32))
    im = np.abs(iq.imag.astype(np.float32))
    big = np.maximum(re, im)
    small = np.minimum(re, im)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(big > 0, small / np.where(big > 0, big, np.float32(1)), np.float32(0)).astype(np.float32)
        out = (big * np.sqrt(_fmaf_rr1(r))).astype(np.float32)
    out = np.where(np.isnan(re) | np.isnan(im), np.float32(np.nan), out)
    out = np.where(np.isinf(re) | np.isinf(im), np.float32(np.inf), out)
    return out.astype(np.float32)


def edges(r, bins):
    """np.histogram2d's float64 edges for range [-r, r]."""
    return np.linspace(-float(r), float(r), int(bins) + 1)


def histogram(i_data, q_data, r, bins=128):
    """counts[q_bin][i_bin] (uint32) = np.histogram2d(i, q, bins, [[-r, r], [-r, r]])[0].T."""
    e = edges(r, bins)

    def idx(v):
        k = np.searchsorted(e, v.astype(np.float64), side="right")
        k[v.astype(np.float64) == e[-1]] -= 1
        return k

    ki, kq = idx(i_data), idx(q_data)
    keep = (ki >= 1) & (ki <= bins) & (kq >= 1) & (kq <= bins)
    flat = (kq[keep] - 1) * bins + (ki[keep] - 1)
    return np.bincount(flat, minlength=bins * bins).astype(np.uint32).reshape(bins, bins)


def histogram_rows(i_data, q_data, r, bins=128):
    """histogram() of every row of two [rows, n] arrays: counts[row][q_bin][i_bin]."""
    e = edges(r, bins)

    def idx(v):
        v = v.astype(np.float64)
        k = np.searchsorted(e, v.reshape(-1), side="right").reshape(v.shape)
        k[v == e[-1]] -= 1
        return k

    ki, kq = idx(i_data), idx(q_data)
    keep = (ki >= 1) & (ki <= bins) & (kq >= 1) & (kq <= bins)
    row = np.broadcast_to(np.arange(ki.shape[0])[:, None], ki.shape)
    flat = (row[keep] * bins + (kq[keep] - 1)) * bins + (ki[keep] - 1)
    return np.bincount(flat, minlength=ki.shape[0] * bins * bins).astype(np.uint32).reshape(ki.shape[0], bins, bins)


def min_dist_sq(i_data, q_data, pts):
    """Brute-force nearest-point squared distance in the table's dtype, NaN propagating."""
    dt = pts.dtype
    i = i_data.astype(dt)
    q = q_data.astype(dt)
    best = None
    for px, py in pts:
        dx = i - dt.type(px)
        dy = q - dt.type(py)
        d = dx * dx + dy * dy
        best = d if best is None else np.where(np.isnan(best) | np.isnan(d), dt.type(np.nan), np.minimum(best, d))
    return best


def split_leaves(n, depth=0):
    """(leaf sizes in order, depth of the deepest leaf) of numpy's pairwise_sum over n elements; the root is at 0."""
    if n <= 128:
        return [n], depth
    n2 = n // 2
    n2 -= n2 % 8
    left, dl = split_leaves(n2, depth + 1)
    right, dr = split_leaves(n - n2, depth + 1)
    return left + right, max(dl, dr)


def sequential_sum(x):
    """A plain left-to-right fold in x's dtype: what a summation that ignores numpy's tree would give."""
    return np.cumsum(x, dtype=x.dtype)[-1] if len(x) else x.dtype.type(0)


def evaluate(iq, modulation="qpsk", r=1.5, bins=128, pts=None):
    """dict(rms float32, evm float or None, counts [bins][bins] uint32, i, q float32) of update_iq_data; pts (an
    [n, 2] float32 / float64 table, possibly empty) overrides reference_points(modulation).  evaluate_rows() below is
    its twin over many rows at once: a change here belongs there too."""
    iq = np.asarray(iq).astype(np.complex64)
    a = cabs(iq)
    with np.errstate(over="ignore", invalid="ignore"):        # |x|^2 may overflow: rms is inf then, as numpy's
        rms = np.sqrt(np_mean((a * a).astype(np.float32))).astype(np.float32)
    re = iq.real.astype(np.float32)
    im = iq.imag.astype(np.float32)
    if rms > np.float32(1e-10):
        scl = np.float32(1.0) / rms
        z = np.float32(0.0)
        with np.errstate(invalid="ignore"):
            i_data = ((re + im * z) * scl).astype(np.float32)
            q_data = ((im - re * z) * scl).astype(np.float32)
    else:
        i_data, q_data = re, im
    if pts is None:
        pts = reference_points(modulation)
    evm = None
    if pts is not None and len(pts):
        d = min_dist_sq(i_data, q_data, pts)
        evm = float(np.sqrt(np_mean(d)))
    return {"rms": np.float32(rms), "evm": evm, "counts": histogram(i_data, q_data, r, bins), "i": i_data,
            "q": q_data}


def _rows_mean(x):
    """np_mean of every row of a [rows, n] float array."""
    acc = np.zeros(x.shape[0], x.dtype)
    for lo in range(0, x.shape[1], BLOCK):
        acc = acc + _pairwise(x[:, lo:lo + BLOCK])
    mean = acc.astype(np.float64) / np.float64(x.shape[1])
    return mean.astype(x.dtype)


def evaluate_rows(rows, modulation="qpsk", r=1.5, bins=128, pts=None):
    """evaluate() of every row of a [rows, n] complex array at once (the segments of a capture), with the same
    operations in the same order: dict(rms [rows] float32, evm [rows] float64 (NaN without a table), counts
    [rows][bins][bins] uint32, i, q [rows, n] float32).  It restates evaluate(): keep the two in step
    (tests/test_constellation_host.py compares them row by row)."""
    rows = np.asarray(rows).astype(np.complex64)
    a = cabs(rows)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rms = np.sqrt(_rows_mean((a * a).astype(np.float32))).astype(np.float32)
        re = rows.real.astype(np.float32)
        im = rows.imag.astype(np.float32)
        on = (rms > np.float32(1e-10))[:, None]
        scl = (np.float32(1.0) / rms).astype(np.float32)[:, None]
        z = np.float32(0.0)
        i_data = np.where(on, (re + im * z) * scl, re).astype(np.float32)
        q_data = np.where(on, (im - re * z) * scl, im).astype(np.float32)
    if pts is None:
        pts = reference_points(modulation)
    evm = np.full(len(rows), np.nan)
    if pts is not None and len(pts):
        with np.errstate(over="ignore", invalid="ignore"):
            evm = np.sqrt(_rows_mean(min_dist_sq(i_data, q_data, pts))).astype(np.float64)
    return {"rms": rms, "evm": evm, "counts": histogram_rows(i_data, q_data, r, bins), "i": i_data, "q": q_data}


def readout(evm, modulation):
    """DataProcessor._process_constellation_data's label text for a measured EVM."""
    if evm is None or not evm > 0:
        return ""
    return f"EVM  {modulation.upper()}\n{evm * 100.0:.1f}%  ({20.0 * np.log10(evm):+.1f} dB)"
