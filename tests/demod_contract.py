"""The analog demodulator's contract in numpy float64: what tdsa_demod_* computes, stated
without reference to how the kernels compute it.

    d[n] = arg(x[n] conj x[n-1]) / pi (FM, x[-1] = 0, 0 where the product is 0, +1 where it is negative real) or |x[n]|
    a[m] = sum_{k < T} g[k] d[mR - k], d = 0 before sample 0
    y[m] = c y[m-1] + (1 - c) a[m], y[-1] = 0
    out  = s a | s y | s (a - y)

Non-finite samples.  An output depends on the samples of its padded window only: a[m] on d[n] for n in (mR - QR, mR],
Q = ceil(T / R), and d[n] on x[n] (FM: and x[n-1]).  FM gives d[n] = NaN when any part of x[n] or x[n-1] is not finite;
AM gives a non-finite |x[n]|: NaN with a NaN part, inf with an infinite one (with both, np.abs says inf and the device's
sqrt(fma(xr, xr, xi xi)) NaN: either).  Such a d[n] makes a[m] non-finite wherever g[mR - n] != 0; an output
that meets it only under the zero padding T <= k < QR is unspecified, every other output does not see it.  The one-pole
section and sum / sumsq keep a non-finite value as their recurrences do, until reset() / reset_measure(); count counts
it; max and min skip NaN (np.fmax / np.fmin).  Other channels never see it.
"""
import numpy as np

FM, AM = 0, 1
POLE_OFF, POLE_LOW, POLE_HIGH = 0, 1, 2
U = 2.0 ** -24
POLE_BLOCK = 64          # kDemodPoleBlock
TILE = 256               # kDemodTile

# Worst |error| of the device's discriminators against double, in u = 2^-24 (FM: of a half turn, wrapped; AM: of |x|),
# over the sweep of tests/demod_math_host.cpp: 10^5 angles per octant with the neighbourhoods of every axis, diagonal and
# of +-pi, magnitudes 2^-20 .. 1 on both samples.  Measured 2026-10-18 with
#   clang++ -O2 -std=c++17 -I topdogspectrumanalyser_amd/csrc tests/demod_math_host.cpp -o demod_math_host && ./demod_math_host
# (the host compiler that ships with ROCm), which printed "fm 1.29" and "am 1.88"; the constants are those, rounded up
# to the next 0.05 so that another libm's sin / cos in the sweep's inputs cannot tip them.
A_D_FM = 1.30
A_D_AM = 1.90


def a_d(mode):
    return A_D_AM if mode == AM else A_D_FM


def n_outputs(n_in, R):
    return -(-int(n_in) // int(R))


def phase_step(x, prev):
    """arg(x conj prev) / pi elementwise (float64): 0 where the product is 0, +1 where it is negative real, NaN where
    any part of x or prev is not finite."""
    x, prev = np.asarray(x, dtype=np.complex128), np.asarray(prev, dtype=np.complex128)
    with np.errstate(invalid="ignore"):
        re = x.real * prev.real + x.imag * prev.imag
        im = x.imag * prev.real - x.real * prev.imag
        d = np.arctan2(im, re) / np.pi
    d[(re == 0) & (im == 0)] = 0.0
    d[(im == 0) & (re < 0)] = 1.0
    bad = ~(np.isfinite(x.real) & np.isfinite(x.imag) & np.isfinite(prev.real) & np.isfinite(prev.imag))
    d[bad] = np.nan                        # arctan2 alone gives a number for (finite, inf) and (inf, inf)
    return d


def discriminator(x, mode, as_stored=True):
    """d[n], float64, of one channel x, taken as the complex64 the device stores (as_stored=False: as it is given)."""
    x = np.asarray(x, dtype=np.complex64 if as_stored else np.complex128).astype(np.complex128)
    if mode == AM:
        return np.abs(x)
    return phase_step(x, np.concatenate([[0.0 + 0.0j], x[:-1]]))


def bad_discriminator_values(n_star, mode):
    """The indices n at which a non-finite x[n_star] makes d[n] non-finite."""
    return (n_star,) if mode == AM else (n_star, n_star + 1)


def fir(d, g, R):
    """a[m] = sum_k g[k] d[mR - k], m < ceil(n / R), float64."""
    d = np.asarray(d, dtype=np.float64)
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    full = np.convolve(d, g)[:len(d)]
    return full[::int(R)].copy()


def abs_fir(d, g, R):
    """sum_k |g[k]| |d[mR - k]|: what the rounding allowance of a[m] scales with."""
    return fir(np.abs(d), np.abs(np.asarray(g, dtype=np.float32)), R)


def one_pole(a, c):
    y = np.empty(len(a), dtype=np.float64)
    acc = 0.0
    c = float(c)
    for m, v in enumerate(np.asarray(a, dtype=np.float64)):
        acc = c * acc + (1.0 - c) * v
        y[m] = acc
    return y


def output(a, pole_mode, c, scale):
    s = float(np.float32(scale))
    if pole_mode == POLE_OFF:
        return s * a
    y = one_pole(a, c)
    return s * y if pole_mode == POLE_LOW else s * (a - y)


def reference(x, mode, g, R, pole_mode=POLE_OFF, c=0.0, scale=1.0):
    """(d, a, out) of every channel of x [C][n] (or [n]), float64."""
    x = np.atleast_2d(np.asarray(x))
    d = np.stack([discriminator(row, mode) for row in x])
    a = np.stack([fir(row, g, R) for row in d])
    out = np.stack([output(row, pole_mode, c, scale) for row in a])
    return d, a, out


def measurements(a):
    """(count, max, min, sum, sumsq) per channel over a [C][n_out]; max and min skip NaN, the sums keep it."""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    n = a.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.full(a.shape[0], n, dtype=np.int64), np.fmax.reduce(a, axis=1, initial=-np.inf),
                np.fmin.reduce(a, axis=1, initial=np.inf), a.sum(axis=1), (a * a).sum(axis=1))


def pole_allowance(a, c):
    """(B + 3) u max|a| (1 + 1 / (1 - c^B)): the block sums' fma chains, and the carry's error summed over the blocks."""
    B = POLE_BLOCK
    return (B + 3) * U * float(np.max(np.abs(a))) * (1.0 + 1.0 / (1.0 - float(c) ** B))
