"""The FSK analysis' contract in numpy: what tdsa_fsk_* computes, stage by stage.  Positions are
integers in 32.32 fixed point as in symsync_contract.py, whose resampler, rotation and constants this file shares.
Stages 0 - 3 (discriminator, boxcar, timing, resampling) are float64 here and float32 on the device, held together by the
bounds below; stages 4 and 5 (decisions, fit, errors) are defined in float32 and float64 operation by operation, and
this file restates them exactly, summation trees included, so that from the same levels v it gives the device's bits.
The test signals both sides are tried on are made here too."""
import math

import numpy as np

import symsync_contract as sc
from demod_contract import A_D_FM
from symsync_contract import A_ATAN, A_C, A_ROT, MASK, ONE, THREADS, U, nu_of, step_of, tree_depth  # noqa: F401

IQ, FREQ = 0, 1
MAX_SYMBOLS = 4096
NONFINITE, ONE_LEVEL = 1, 2
F32 = np.float32


# ---- parameters -------------------------------------------------------------------------------------------------------
def default_boxcar(sps: float) -> int:
    return max(1, int(math.floor(float(sps) / 2)))


def boxcar_outputs(seg_len: int, kind: int, B: int) -> int:
    """n_b = n_d - B + 1, n_d = seg_len - 1 (iq) or seg_len (freq)."""
    return int(seg_len) - (1 if kind == IQ else 0) - int(B) + 1


def symbols_per_segment(step: int, seg_len: int, kind: int, B: int) -> int:
    nb = boxcar_outputs(seg_len, kind, B)
    return ((nb - 4) * ONE) // int(step) - 1 if nb >= 4 else -1


def group_delay(kind: int, B: int) -> float:
    """Where b_0 sits among the input samples: d_j lies between x[j] and x[j + 1] (iq), the boxcar adds (B - 1) / 2."""
    return B / 2.0 if kind == IQ else (B - 1) / 2.0


# ---- stages 0 - 3, float64 ---------------------------------------------------------------------------------------------
def discriminate(x):
    """d_j = arg(x[j + 1] conj x[j]) / pi, half turns per sample, not unwrapped."""
    x = np.asarray(x, dtype=np.complex128)
    return np.angle(x[1:] * np.conj(x[:-1])) / np.pi


def boxcar(d, B: int):
    """b_j = (d_j + ... + d_j+B-1) / B, added in ascending order."""
    d = np.asarray(d, dtype=np.float64)
    n = d.size - B + 1
    b = d[:n].copy()
    for i in range(1, B):
        b = b + d[i:i + n]
    return b / B


def boxcar32(d, B: int):
    """The device's b from float32 d, operation by operation: float32 adds in ascending order, then float32(1 / B)."""
    d = np.asarray(d, dtype=F32)
    n = d.size - B + 1
    b = d[:n].copy()
    for i in range(1, B):
        b = (b + d[i:i + n]).astype(F32)
    return (b * (F32(1.0) / F32(B))).astype(F32)


def delta_from_t(t, step: int, L: int) -> int:
    """The exact integer expression of stage 2's end, from t (0 <= t <= 1; the device's is a float32)."""
    tq = int(math.floor(float(t) * ONE))
    d = (tq * int(step)) >> 32
    d = (d + (int(L) << 31) + (int(step) >> 1)) % int(step)
    return d + int(step) if d < ONE else d


def delta_of(C: complex, step: int, L: int) -> int:
    a = 0.0 if C == 0 else math.atan2(C.imag, C.real) / math.pi
    t = -a / 2
    if t < 0:
        t += 1
    return delta_from_t(t, step, L)


def timing(b, nu: int, step: int, L: int):
    """Stage 2 of one segment: (C, P, delta_fx); an empty e gives (0, 0, delta of t = 0)."""
    b = np.asarray(b, dtype=np.float64)
    if b.size <= L:
        return 0j, 0.0, delta_of(0j, step, L)
    e = (b[L:] - b[:-L]) ** 2
    ph = (np.arange(e.size, dtype=np.uint64) * np.uint64(nu)) & np.uint64(MASK)
    P = float(np.sum(e))
    C = complex(np.sum(e * np.exp(-2j * np.pi * ph.astype(np.float64) / ONE)))
    return C, P, delta_of(C, step, L)


def resample(b, delta_fx: int, step: int, K: int, with_bound: bool = False):
    """Stage 3: v[K] float64; with_bound also sum |c| |b| and sum |c| per symbol."""
    b = np.asarray(b, dtype=np.float64)
    i, mu = sc.positions(delta_fx, step, K)
    c = sc.coeffs(mu)
    taps = np.stack([b[i - 1], b[i], b[i + 1], b[i + 2]])
    with np.errstate(invalid="ignore"):             # 0 x inf under a tap: a NaN, as on the device
        v = np.sum(c * taps, axis=0)
    if not with_bound:
        return v
    return v, np.sum(np.abs(c) * np.abs(taps), axis=0), np.sum(np.abs(c), axis=0)


# ---- stages 4 and 5, exactly -------------------------------------------------------------------------------------------
def tree_sum(values) -> float:
    """The kernel's float64 sum: thread t folds elements t, t + 256, ... in order, then the partials fold pairwise,
    (t, t + 128), (t, t + 64), ..."""
    a = np.asarray(values, dtype=np.float64)
    rows = -(-a.size // THREADS)
    pad = np.zeros(rows * THREADS, dtype=np.float64)
    pad[:a.size] = a
    pad = pad.reshape(rows, THREADS)
    p = np.zeros(THREADS, dtype=np.float64)
    for r in range(rows):
        n = min(THREADS, a.size - r * THREADS)
        p[:n] = p[:n] + pad[r, :n]
    o = THREADS // 2
    while o >= 1:
        p[:o] = p[:o] + p[o:2 * o]
        o //= 2
    return float(p[0])


def first_guess(lo, hi, M: int):
    lo, hi = F32(lo), F32(hi)
    with np.errstate(all="ignore"):
        return F32((hi + lo) * F32(0.5)), F32((hi - lo) * (F32(1.0) / F32(2 * (M - 1))))


def decide(v, o, g, M: int):
    """i = clamp(floor((v - o) / (g + g) + M / 2), 0, M - 1), four float32 operations; a NaN gives 0."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        q = np.floor(((v - F32(o)).astype(F32) / F32(F32(g) + F32(g))).astype(F32) + F32(M // 2)).astype(F32)
    return np.where(q >= M - 1, M - 1, np.where(q > 0, q, 0)).astype(np.int64)


def fit(v, l):
    """(o, g) float32 of the least-squares line through (l_k, v_k), or None when D = 0; also sum l."""
    v64 = np.asarray(v, dtype=F32).astype(np.float64)
    l = np.asarray(l, dtype=np.int64)
    K, sl, sl2 = int(v64.size), int(l.sum()), int((l * l).sum())
    D = K * sl2 - sl * sl
    if D == 0:
        return None, sl
    sv, slv = tree_sum(v64), tree_sum(l.astype(np.float64) * v64)
    num = float(K) * slv - float(sl) * sv
    g64 = num / float(D)
    o64 = (sv - g64 * float(sl)) / float(K)
    return (F32(o64), F32(g64)), sl


def fmaf(a, b, c):
    """fmaf(a, b, c) in float32 for float32 a, c and small integers b: the product is exact in float64; the float64 sum
    s is rounded to float32 as it is unless s lies exactly half way between two float32 while the exact sum does not:
    only then is s moved one float64 step towards the exact sum, off the tie, before the rounding.  (A float64 rounding
    that moved the sum onto or across a float32 number changes nothing: it is monotone and keeps float32 numbers.)"""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64) + np.zeros_like(p)
    s = p + c
    # the error of the float64 sum, exactly (two-sum)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    with np.errstate(all="ignore"):
        r = s.astype(F32).astype(np.float64)
        other = np.where(r > s, np.nextafter(r.astype(F32), F32(-np.inf)), np.nextafter(r.astype(F32), F32(np.inf))).astype(np.float64)
        tie = (r != s) & (np.abs(r - s) == np.abs(other - s))
    s = np.where(tie & (err > 0), np.nextafter(s, np.inf), np.where(tie & (err < 0), np.nextafter(s, -np.inf), s))
    return s.astype(F32)


def levels(v, M: int):
    """Stages 4 and 5 of one segment from its float32 levels v: dict(lo, hi, offset, dev, indices, l, sum_l, flags, err,
    err_sumsq, err_peak, err_peak_k, deciders) with the device's bits."""
    v = np.asarray(v, dtype=F32)
    lo, hi = F32(v.min()), F32(v.max())
    o, g = first_guess(lo, hi, M)
    flags, sum_l, deciders = 0, 0, []
    for _ in range(2):
        od, gd = o, g
        deciders.append((od, gd))
        i = decide(v, od, gd, M)
        l = 2 * i - (M - 1)
        got, sum_l = fit(v, l)
        if got is None:
            flags |= ONE_LEVEL
        else:
            o, g = got
    with np.errstate(all="ignore"):
        err = (v - fmaf(g, l, o)).astype(F32)
    e64 = err.astype(np.float64)
    ae = np.abs(err)
    k = int(np.argmax(ae)) if np.any(ae > 0) else 0
    return dict(lo=lo, hi=hi, offset=o, dev=g, indices=i.astype(np.uint8), l=l, sum_l=sum_l, flags=flags, err=err,
                err_sumsq=tree_sum(e64 * e64), err_peak=F32(ae[k]), err_peak_k=k, deciders=deciders)


def analyse(x, sps: float, M: int = 2, kind: int = IQ, B=None, L=None, delta_fx=None):
    """All stages of one segment: stages 0 - 3 in float64, v rounded to float32, then levels()."""
    step, nu = step_of(sps), nu_of(sps)
    B = default_boxcar(sps) if B is None else int(B)
    L = default_boxcar(sps) if L is None else int(L)
    d = discriminate(x) if kind == IQ else np.asarray(x, dtype=np.float64)
    b = boxcar(d, B)
    K = symbols_per_segment(step, len(x), kind, B)
    C, P, dl = timing(b, nu, step, L)
    if delta_fx is not None:
        dl = int(delta_fx)
    v = resample(b, dl, step, K)
    out = dict(delta_fx=dl, C=C, P=P, b=b, v=v, K=K, B=B, L=L, delta=dl / ONE + group_delay(kind, B))
    if not (np.isfinite(P) and np.isfinite(C.real) and np.isfinite(C.imag) and np.all(np.isfinite(v.astype(F32)))):
        out.update(flags=NONFINITE)            # P, C or a level is not finite: NaN levels, zero indices, a zero record
        return out
    out.update(levels(v.astype(F32), M))
    outer = float(out["dev"]) * (M - 1)
    out["deviation"] = outer
    out["fsk_error"] = math.sqrt(out["err_sumsq"] / K) / outer if outer > 0 else 0.0
    return out


# ---- how far float32 may stand from stages 0 - 3 -----------------------------------------------------------------------
# Bounds in u = 2^-24, the relative error of one float32 rounding, counted from the roundings tdsa_fsk_math.hpp and the
# headers it includes write out; tests/fsk_math_host.cpp measures the new functions against double and long double, and
# the CPU test asserts that what it measures stays at or below MEASURED, and MEASURED at or below the counted bounds.
# MEASURED is what
#   clang++ -O2 -std=c++17 -I topdogspectrumanalyser_amd/csrc tests/fsk_math_host.cpp -o fsk_math_host && ./fsk_math_host
# (the host compiler that ships with ROCm) printed - "t 0.89", "dec 2.30", "fit 0.86" - rounded up to the next 0.05 so
# that another libm's sin / cos in the sweep's inputs cannot tip them.
MEASURED = dict(t=0.90, dec=2.30, fit=0.90)
# t, the clock phase in symbols, from C, against -atan2 / (2 pi) in double: the arctangent's A_ATAN u of a half turn,
# which the halving halves (and does not round), and the + 1 of a negative t (u of a value below 1): A_ATAN / 2 + 1,
# in u of a symbol.  delta_fx from that t is integers throughout: the sweep holds it to the count against
# delta_from_t's expression in 128-bit integers at every L.
A_T = 1.9
# The decision's argument (v - o) / (g + g) + M / 2 against the same in long double: v - o and the quotient each round
# once (g + g is exact), 2 u of |t|, and the sum once more, u of |t + M / 2|: 3 u of max(|t|, |t + M / 2|, 1).  The
# sweep goes next to every threshold, from both sides, over seven decades of g and offsets up to 64 g.
A_DEC = 3.0
# The fit: float64 throughout and one rounding to float32 at the end, u of |g| and u of |o|.  The float64 part is below
# 1e-6 u for K <= 4096 whenever D != 0, so the bound is u (1 + 1e-6) of |o| + |g| for either result.
A_FIT = 1.05


def boxcar_bound(absd_mean: float, kind: int, B: int) -> float:
    """|b_dev - b|: B - 1 additions, the scale and its own rounding, each u of at most sum |d| / B ... and, for iq,
    the discriminator's own A_D_FM u of a half turn, which an average does not enlarge."""
    return ((B + 1) * absd_mean + (A_D_FM if kind == IQ else 0.0)) * U * 1.01


def timing_bound(b, L: int, eb: float) -> float:
    """|C_dev - C| and |P_dev - P| per part.  With every b off by at most eb, a difference is off by 2 eb + u |df| and its
    square by 4 eb |df| + 4 eb^2 + 3 u df^2; the sum carries the rotation's error and the depth of its tree."""
    b = np.asarray(b, dtype=np.float64)
    df = np.abs(b[L:] - b[:-L])
    P = float(np.sum(df ** 2))
    return float(np.sum(4 * eb * df + 4 * eb * eb)) * 1.01 + (tree_depth(df.size) + 3 + A_ROT + 3) * U * P * 1.01


def delta_bound(C: complex, e: float, step: int) -> int:
    """|delta_dev - delta| modulo step for |C_dev - C| <= e per part: arg C moves by at most asin(sqrt 2 e / |C|), t
    takes A_T u of a symbol (2 A_T of a half turn), and the floor and the 32-bit t add two counts (+ step >> 32 for the floor's scale)."""
    da = math.asin(min(1.0, math.sqrt(2.0) * e / abs(C))) / math.pi + 2 * A_T * U
    return int(math.ceil(da / 2 * step)) + 2 + (step >> 32)


def resample_bound(mag, sumc, eb: float):
    """|v_dev - v| for sum |c| |b| = mag: four roundings of the sum and the coefficients' own error, and b's own error
    through sum |c|."""
    return (4 + A_C) * U * mag + sumc * eb * 1.01


def fit_bound(o: float, g: float) -> float:
    return A_FIT * U * (abs(float(o)) + abs(float(g)))


def threshold_margin(v, o, g, M: int):
    """Per symbol, how far v lies from the nearest decision threshold o + g (2 j - M), j = 1 .. M - 1, in units of v."""
    v = np.asarray(v, dtype=np.float64)
    th = float(o) + float(g) * (2.0 * np.arange(1, M) - M)
    return np.min(np.abs(v[:, None] - th[None, :]), axis=1)


def threshold_shift(l, vb: float, M: int) -> float:
    """How far a threshold can move when every v_k moves by at most vb and the decisions stay: the fitted g by vb sum
    |l - mean| / sum (l - mean)^2, o by vb + |mean| of that, a threshold by the o's plus (M - 2) times the g's; the first
    guess from lo and hi moves by no more than 2 vb either.  Plus the decision's own rounding, A_DEC u of M / 2 + 1
    spacings, which the caller adds in units of g."""
    l = np.asarray(l, dtype=np.float64)
    c = l - l.mean()
    dg = vb * float(np.sum(np.abs(c))) / float(np.sum(c * c))
    return max(2 * vb, vb + abs(float(l.mean())) * dg + (M - 2) * dg)


# ---- test signals -------------------------------------------------------------------------------------------------------
_erf = np.frompyfunc(math.erf, 1, 1)


def _pulse_integral(t, bt):
    """The integral from -inf to t (in symbols) of the frequency pulse of unit area: a rectangle over [0, 1) for bt =
    None, else that rectangle through a Gaussian filter of bandwidth-time product bt."""
    t = np.asarray(t, dtype=np.float64)
    if bt is None:
        return np.clip(t, 0.0, 1.0)
    s = math.sqrt(math.log(2.0)) / (2.0 * math.pi * bt)           # the Gaussian's sigma in symbols

    def big_phi_integral(x):                                        # integral of the normal CDF: x Phi(x) + phi(x)
        cdf = 0.5 * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))
        return x * cdf + np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return s * (big_phi_integral(t / s) - big_phi_integral((t - 1.0) / s))


def make_fsk(M: int, sps: float, n: int, h: float, bt=None, seed: int = 1, offset: float = 0.37, cfo: float = 0.01,
             noise_db: float = -40.0, span: int = 4, symbols=None):
    """n samples of a random M-level FSK stream of modulation index h (adjacent levels h symbol rates apart): symbol m
    occupies [(m + offset) sps, (m + 1 + offset) sps), its centre half a symbol later; rectangular frequency pulses or
    Gaussian ones (bt); a carrier offset of cfo cycles per sample; white noise at noise_db relative to the unit carrier
    over the full sample rate.  Returns (x complex128, the level indices by symbol with symbol m at [m + span + 1], the
    first symbol centre's position modulo sps in samples)."""
    rng = np.random.default_rng(seed)
    n_sym = int(n / sps) + 2 * span + 4
    idx = rng.integers(0, M, n_sym) if symbols is None else np.asarray(symbols)[:n_sym]
    lev = 2.0 * idx - (M - 1)
    t = np.arange(n, dtype=np.float64) / sps - offset              # in symbols, >= -offset > -1
    m0 = np.floor(t).astype(np.int64)
    ph = np.zeros(n, dtype=np.float64)                              # in cycles: (h / 2) sum l_m Q(t - m)
    for d in range(-span, span + 1):
        m = m0 + d
        ph += lev[m + span + 1] * _pulse_integral(t - m, bt)
    # the symbols before the window (stored at 0 .. m0) have delivered all of their area
    ph += np.concatenate([[0.0], np.cumsum(lev)])[m0 + 1]
    x = np.exp(2j * np.pi * (0.5 * h * ph + cfo * np.arange(n)))
    s = 10.0 ** (noise_db / 20.0) / math.sqrt(2.0)
    x = x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x, idx, ((offset + 0.5) * sps) % sps


def make_freq(M: int, sps: int, n: int, dev: float, o: float = 0.0, seed: int = 1, t0: int = 0, bt=None, symbols=None):
    """A float64 frequency stream for the `freq` input: M-level symbols of half spacing dev about o, rectangular or
    Gaussian pulses, symbol boundaries at t0 + m sps.  Returns (f, indices with symbol m at [m + 5])."""
    rng = np.random.default_rng(seed)
    span = 4
    n_sym = n // sps + 2 * span + 4
    idx = rng.integers(0, M, n_sym) if symbols is None else np.asarray(symbols)[:n_sym]
    lev = 2.0 * idx - (M - 1)
    t = (np.arange(n, dtype=np.float64) + 0.5 - t0) / sps
    m0 = np.floor(t).astype(np.int64)
    f = np.zeros(n)
    for d in range(-span, span + 1):
        m = m0 + d
        f += lev[m + span + 1] * (_pulse_integral(t - m + 0.5 / sps, bt) - _pulse_integral(t - m - 0.5 / sps, bt)) * sps
    return o + dev * f, idx
