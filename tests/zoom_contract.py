"""The zoom front end's contract, restated in numpy float64.

Inputs count from the last reset, across calls: n = 0, 1, ...
  x[n]  the existing unpack: int8 (I + jQ)/128 (oracle.spectrum_oracle.unpack_iq_int8), uint8 float32 of pyrtlsdr's
        float64 u/127.5 - 1, complex64 as is
  p[n]  (p_b + (n - n_b) s) mod 2^32 with (p_b, n_b) the phase and index at the last change of the step s; a reset
        sets p = 0 at n = 0; s = round(f_off 2^32 / fs) mod 2^32, |f_off| <= fs/2
  v[n]  x[n] exp(-2 pi j p[n] / 2^32), and 0 for n < 0
  y[m]  sum_{k < T} h[k] v[mD - k]; output m is emitted by the call that delivers input mD, so n_total inputs give
        ceil(n_total / D) outputs

Non-finite samples (the rule of all three streaming filters; H = phases D here with phases = ceil(T / D), P M for the
channelizer, Q R for the demodulator).  Output m depends on the inputs of its padded window (mD - H, mD] only: outside
it a non-finite x[n*] changes no bit of any output, whatever the split into calls: the device history carries it for
that window (the down-converter's, rounded up to 8 phases, for longer, where no output reads it).  Inside, every output whose tap h[mD - n*] is not zero is non-finite (all channels of a
channelizer instant); an output that meets x[n*] only under the zero padding T <= k < H is unspecified.
"""
import numpy as np

from oracle import spectrum_oracle as so

FMT_I8, FMT_U8, FMT_C64 = 0, 1, 2


def unpack(raw, fmt: int) -> np.ndarray:
    """complex64 x[n] of a raw block."""
    if fmt == FMT_I8:
        return so.unpack_iq_int8(raw)
    if fmt == FMT_U8:
        return so.unpack_iq_uint8_rtl(raw).astype(np.complex64)
    return np.asarray(raw, dtype=np.complex64)


def phases(n_total: int, retunes) -> np.ndarray:
    """p[n] (int64, 0 .. 2^32-1) for n < n_total; retunes = [(n_b, s), ...] in order, the first at n_b = 0."""
    p = np.empty(n_total, dtype=np.int64)
    p_b = 0
    for i, (n_b, s) in enumerate(retunes):
        n_e = retunes[i + 1][0] if i + 1 < len(retunes) else n_total
        n = np.arange(n_b, n_e, dtype=np.int64)
        p[n_b:n_e] = (p_b + (n - n_b) * int(s)) % (1 << 32)
        p_b = (p_b + (n_e - n_b) * int(s)) % (1 << 32)
    return p


def mix(x: np.ndarray, p: np.ndarray) -> np.ndarray:
    return x.astype(np.complex128) * np.exp(-2j * np.pi * (p.astype(np.float64) / 2.0 ** 32))


def n_outputs(n_total: int, D: int) -> int:
    return -(-n_total // D)


def direct(v: np.ndarray, h: np.ndarray, D: int, ms) -> np.ndarray:
    """y[m] for the chosen m, as the defining sum (float64)."""
    h = np.asarray(h, dtype=np.float64)
    k = np.arange(h.size)
    out = np.empty(len(ms), dtype=np.complex128)
    for i, m in enumerate(ms):
        idx = int(m) * D - k
        ok = idx >= 0
        out[i] = np.sum(h[ok] * v[idx[ok]])
    return out


def by_convolution(v: np.ndarray, h: np.ndarray, D: int) -> np.ndarray:
    """Every output at once: np.convolve(v, h)[::D], ceil(n / D) of them."""
    return np.convolve(v, np.asarray(h, dtype=np.float64))[::D][:n_outputs(len(v), D)]


def padded_window_outputs(n_star: int, H: int, D: int, n_out: int) -> np.ndarray:
    """The outputs m < n_out whose padded window (mD - H, mD] holds input n_star; H a multiple of D."""
    lo, hi = -(-int(n_star) // D), (int(n_star) + H - 1) // D
    return np.arange(lo, min(hi, n_out - 1) + 1)


def hit_outputs(n_star: int, h, D: int, n_out: int) -> np.ndarray:
    """The outputs m < n_out that meet input n_star under a non-zero tap: these a non-finite x[n_star] makes non-finite."""
    h = np.asarray(h)
    m = np.arange(-(-int(n_star) // D), n_out)
    k = m * D - int(n_star)
    ok = k < h.size
    return m[ok][h[k[ok]] != 0]


def lanes(D: int) -> int:
    """Residue lanes of the FIR kernel the launcher picks for D (a workgroup owns 2048 / lanes outputs)."""
    return 64 if D >= 64 else 32 if D > 16 else 16 if D > 8 else 8 if D > 4 else 4 if D > 2 else 2


def integer_fir(re, im, h, D: int):
    """y[m] = sum_k h[k] x[mD - k] of integer-valued x = re + j im and integer-valued taps, every output, in int64:
    one dot product per output (as direct() does), so a long filter stays cheap.  Returns (real, imag) int64."""
    hr = np.asarray(h).astype(np.int64)[::-1].copy()
    assert np.array_equal(hr[::-1], np.asarray(h)), "taps must be integers"
    T = hr.size
    pr = np.concatenate([np.zeros(T - 1, np.int64), np.asarray(re, dtype=np.int64)])
    pi = np.concatenate([np.zeros(T - 1, np.int64), np.asarray(im, dtype=np.int64)])
    n_out = n_outputs(len(re), D)
    yr = np.empty(n_out, np.int64)
    yi = np.empty(n_out, np.int64)
    for m in range(n_out):                      # window x[mD - T + 1 .. mD] against the reversed taps
        yr[m] = hr @ pr[m * D:m * D + T]
        yi[m] = hr @ pi[m * D:m * D + T]
    return yr, yi


def reference(raw, fmt: int, h, D: int, retunes, ms=None) -> np.ndarray:
    """y of a whole stream (ms = None) or of the chosen outputs, in float64."""
    x = unpack(raw, fmt)
    v = mix(x, phases(len(x), retunes))
    return by_convolution(v, h, D) if ms is None else direct(v, h, D, ms)
