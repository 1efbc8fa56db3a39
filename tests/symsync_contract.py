"""The symbol recovery's contract in numpy float64: what tdsa_symsync_* computes, stage by
stage, with every position an integer in 32.32 fixed point.  The device works in float32 with the arithmetic of
csrc/tdsa_symsync_math.hpp; the constants at the end bound how far that may stand from this file, and the test signals
both sides are tried on are made here too."""
import math

import numpy as np

ONE = 1 << 32
MASK = ONE - 1
U = 2.0 ** -24
THREADS = 256                # the kernel's workgroup: the shape of its summation trees
MAX_SYMBOLS = 4096


# ---- parameters -------------------------------------------------------------------------------------------------------
def step_of(sps: float) -> int:
    return int(round(float(sps) * ONE))


def nu_of(sps: float) -> int:
    return int(round(ONE / float(sps)))


def symbols_per_segment(step: int, seg_len: int) -> int:
    return ((int(seg_len) - 4) * ONE) // int(step) - 1 if seg_len >= 4 else -1


def grid(K: int) -> int:
    return 2 * (1 << max(0, (int(K) - 1).bit_length()))


def reference_phase(points, M: int) -> float:
    p = np.asarray(points, dtype=np.complex128).reshape(-1)
    return float(np.angle(np.sum(p ** int(M))))


# ---- the four stages ----------------------------------------------------------------------------------------------------
def timing(x, nu: int, step: int):
    """Stage 1 of one segment: (C, P, delta_fx)."""
    x = np.asarray(x, dtype=np.complex128)
    p = x.real ** 2 + x.imag ** 2
    ph = (np.arange(x.size, dtype=np.uint64) * np.uint64(nu)) & np.uint64(MASK)
    P = float(np.sum(p))
    C = complex(np.sum(p * np.exp(-2j * np.pi * ph.astype(np.float64) / ONE)))
    return C, P, delta_of(C, step)


def delta_of(C: complex, step: int) -> int:
    a = 0.0 if C == 0 else math.atan2(C.imag, C.real) / math.pi
    t = -a / 2
    if t < 0:
        t += 1
    d = int(math.floor(t * step))
    return d + step if d < ONE else d


def coeffs(mu):
    mu = np.asarray(mu, dtype=np.float64)
    return np.stack([-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2,
                     (mu + 1) * mu * (mu - 1) / 6])


def positions(delta_fx: int, step: int, K: int):
    """(i, mu) of the K symbols: integer arithmetic, mu the top 24 bits of the fraction."""
    pos = [int(delta_fx) + k * int(step) for k in range(K)]
    i = np.array([p >> 32 for p in pos], dtype=np.int64)
    mu = np.array([((p & MASK) >> 8) for p in pos], dtype=np.float64) * 2.0 ** -24
    return i, mu


def resample(x, delta_fx: int, step: int, K: int, with_bound: bool = False):
    """Stage 2: y[K]; with_bound also sum |c| |x| per symbol (per part: the larger of re and im)."""
    x = np.asarray(x, dtype=np.complex128)
    i, mu = positions(delta_fx, step, K)
    c = coeffs(mu)
    taps = np.stack([x[i - 1], x[i], x[i + 1], x[i + 2]])
    y = np.sum(c * taps, axis=0)
    if not with_bound:
        return y
    mag = np.sum(np.abs(c) * np.maximum(np.abs(taps.real), np.abs(taps.imag)), axis=0)
    return y, mag


def carrier(y, M: int, ref_arg: float, g=None, step_f=None):
    """Stage 3: dict(g, step_f, theta_fx, peak, mean, power, f, ...).  g, step_f: go on from these (the device's)
    instead of the stage's own."""
    y = np.asarray(y, dtype=np.complex128)
    K, G = y.size, grid(y.size)
    z = y ** M
    Z = np.fft.fft(z, G)
    power = Z.real ** 2 + Z.imag ** 2
    g_max = int(np.argmax(power))
    g = g_max if g is None else int(g)
    f0 = g / G if g < G // 2 else (g - G) / G
    k = np.arange(K)
    zd = z * np.exp(-2j * np.pi * ((k * g) % G) / G)
    H = K // 2
    S1, S2 = np.sum(zd[:H]), np.sum(zd[H:2 * H])
    d = S2 * np.conj(S1)
    f = f0 + (0.0 if d == 0 else math.atan2(d.imag, d.real)) / (2 * math.pi * H)
    step_own = int(round(f / M * ONE)) & MASK
    step_f = step_own if step_f is None else int(step_f)
    s = np.sum(z * np.exp(-2j * np.pi * ((k * M * step_f) & MASK) / ONE))
    a = 0.0 if s == 0 else math.atan2(s.imag, s.real)
    theta_fx = int(round((a - ref_arg) / (2 * math.pi * M) * ONE)) & MASK
    return dict(a=a / math.pi, g=g, step_f=step_f, theta_fx=theta_fx, peak=float(power[g]), mean=float(np.mean(power)), power=power,
                f=f, z=z, S1=S1, S2=S2, s=s, g_max=g_max, step_own=step_own, H=H, G=G)


def derotate(y, step_f: int, theta_fx: int):
    k = np.arange(np.asarray(y).size)
    return np.asarray(y, dtype=np.complex128) * np.exp(-2j * np.pi * ((theta_fx + k * step_f) & MASK) / ONE)


def recover(x, sps: float, M: int, ref_arg: float = 0.0, delta_fx=None):
    """All four stages of one segment: dict(delta_fx, C, P, y, symbols, and stage 3's entries when M != 0)."""
    step, nu = step_of(sps), nu_of(sps)
    K = symbols_per_segment(step, len(x))
    C, P, d = timing(x, nu, step)
    if delta_fx is not None:
        d = int(delta_fx)
    y = resample(x, d, step, K)
    out = dict(delta_fx=d, C=C, P=P, y=y, K=K, step_f=0, theta_fx=0)
    if M:
        out.update(carrier(y, M, ref_arg))
    out["symbols"] = derotate(y, out["step_f"], out["theta_fx"]) if M else y
    return out


# ---- how far float32 may stand from the above ------------------------------------------------------------------------
# Bounds in u = 2^-24, the relative error of one float32 rounding, from the roundings tdsa_symsync_math.hpp writes out;
# tests/symsync_math_host.cpp measures the same quantities against double (random and structured sweeps) and the CPU
# test asserts that what it measures stays below these.
# A Lagrange coefficient, relative to itself: at most five roundings - mu + 1 or mu - 2 (mu - 1 is exact), three
# products, the constant 1/6 (measured 3.5).
A_C = 5.0
# y^M relative to |y|^M.  One squaring (r r - i i fused, (r + r) i) errs by at most (2 u, u) |y|^2 in (re, im), 2.24 u
# as a vector, and doubles the relative error it is handed: E_1 = 2.24, E_2 = 2 E_1 + 2.24, E_3 = 2 E_2 + 2.24
# (measured 1.9 / 4.5 / 8.8).
A_POW = {2: 2.5, 4: 7.0, 8: 16.0}
# The rotation exp(-2 pi i p / 2^32), absolute, as a vector: the table entry's rounding (u / 2 per part of a value below
# 1) and the final addition's (the same), 0.71 u each as vectors; the series' truncation (t^4 / 24 < 1e-5 u), the
# rounding of t and of the small fused term (below 2e-3 u each) are far below (measured 1.39).
A_ROT = 1.5
# demod_atan2_over_pi in u of a half turn: no closed bound; tdsa_demod_math.hpp states 0.12 u truncation + 0.53 u
# evaluated for the polynomial, the quotient and the reflections add one rounding each of values below 1 (u / 2 each):
# 1.65; the sweep here (every octant, the axes' and diagonals' neighbourhoods, |re| = |im|) measures 1.07.
A_ATAN = 1.75


def tree_depth(n: int) -> int:
    """Additions on the longest path of the kernel's sum over n elements: a thread's chain, then eight pairings."""
    return -(-int(n) // THREADS) + 8


def timing_bound(P: float, seg_len: int) -> float:
    """|C_dev - C| and |P_dev - P| per part: every term p_j w_j carries the rounding of |x|^2 (2 u), of the rotation
    (A_ROT u) and of its own fused step, and the sum the depth of its tree."""
    return (tree_depth(seg_len) + 3 + A_ROT) * U * P * 1.01


def delta_bound(C: complex, P: float, seg_len: int, step: int) -> int:
    """|delta_dev - delta| modulo step: arg C moves by at most asin(sqrt 2 bound / |C|), the arctangent adds A_ATAN u
    of a half turn, t takes float32 roundings of its own (3 u), and the floor and the 32-bit t add two counts."""
    e = math.sqrt(2.0) * timing_bound(P, seg_len) / abs(C)
    da = math.asin(min(1.0, e)) / math.pi + (A_ATAN + 3) * U
    return int(math.ceil(da / 2 * step)) + 2 + (step >> 32)


def resample_bound(mag):
    """|y_dev - y| per part for sum |c| |x| = mag: four roundings of the sum and the coefficients' own error."""
    return (4 + A_C) * U * mag


def transform_bound(z, M: int) -> float:
    """|Z_dev - Z| of any bin: z's own error (A_POW u |z|), and per pass one addition, the twiddle's error and the
    product's roundings, all relative to sum |z|, which bounds every intermediate value."""
    G = grid(len(z))
    return (A_POW[M] + math.log2(G) * (A_ROT + 3)) * U * float(np.sum(np.abs(z))) * 1.01


def power_bound(z, M: int) -> float:
    """| |Z_dev|^2 - |Z|^2 | of any bin, |Z| <= sum |z|; the square takes three roundings of its own."""
    e, s = transform_bound(z, M), float(np.sum(np.abs(z)))
    return 2 * s * e + e * e + 3 * U * s * s


def sum_bound(z, M: int) -> float:
    """|S_dev - S| of a rotated sum over z (S1, S2, the phase sum): z's error, the rotation's, the product's roundings
    and the tree's depth, relative to sum |z|."""
    return (A_POW[M] + A_ROT + 3 + tree_depth(len(z))) * U * float(np.sum(np.abs(z))) * 1.01


def _arg_err(e: float, mag: float) -> float:
    """How far, in half turns, the argument of a number of size mag can move under an error e per part."""
    return math.asin(min(1.0, math.sqrt(2.0) * e / mag)) / math.pi if mag > 0 else 1.0


def step_f_bound(c: dict, M: int) -> int:
    """|step_f_dev - step_f| given the same g: the arguments of S1 and S2, the product's and the arctangent's error,
    the float32 roundings of the fine term (three, relative to its size) and two integer roundings."""
    e = sum_bound(c["z"], M)
    dd = _arg_err(e, abs(c["S1"])) + _arg_err(e, abs(c["S2"])) + (A_ATAN + 4) * U
    fine = ONE / (2.0 * c["H"] * M)
    return int(math.ceil(dd * fine + 3 * U * fine)) + 2


def theta_bound(c: dict, M: int) -> int:
    """|theta_dev - theta| modulo 2^32 / M given the same step_f: the phase sum's argument, the arctangent, and the
    float32 roundings of (a - ref) / (2 M) 2^32 (three, of a value up to 2^32 / M)."""
    da = _arg_err(sum_bound(c["z"], M), abs(c["s"])) + (A_ATAN + 1) * U
    return int(math.ceil(da / (2 * M) * ONE + 3 * U * ONE / M)) + 2


def derotate_bound(y):
    """|sym_dev - sym| per symbol: the rotation's error and the product's roundings, relative to |y|."""
    return (A_ROT + 3) * U * np.abs(y) * 1.01


# ---- test signals -------------------------------------------------------------------------------------------------------
def points(name: str) -> np.ndarray:
    """Unit-rms reference points as complex128 (the tables of analytics.constellation_points)."""
    if name == "bpsk":
        return np.array([-1.0, 1.0], dtype=np.complex128)
    if name == "qpsk":
        return np.array([-1 - 1j, -1 + 1j, 1 - 1j, 1 + 1j]) / math.sqrt(2.0)
    if name == "8psk":
        return np.exp(2j * np.pi * np.arange(8) / 8)
    side = {"16qam": 4, "64qam": 8}[name]
    lv = np.arange(1 - side, side, 2, dtype=np.float64)
    g = (lv[:, None] + 1j * lv[None, :]).reshape(-1)
    return g / math.sqrt(np.mean(np.abs(g) ** 2))


ORDER = {"bpsk": 2, "qpsk": 4, "16qam": 4, "64qam": 4, "8psk": 8}


def raised_cosine(t, alpha: float):
    """The raised-cosine pulse at t symbols, float64."""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * alpha * t) ** 2
    sing = np.abs(den) < 1e-9
    out = np.sinc(t) * np.cos(np.pi * alpha * t) / np.where(sing, 1.0, den)
    return np.where(sing, np.pi / 4 * np.sinc(1.0 / (2.0 * alpha)), out)


def make_signal(mod: str, sps: float, n: int, seed: int = 1, offset: float = 0.37, w: float = 0.01, phase: float = 0.7,
                noise_db: float = -40.0, alpha: float = 0.35, span: int = 10):
    """n samples of a random symbol stream of `mod` through a raised-cosine pulse evaluated at the sample instants:
    symbol m sits at sample (m + offset) sps, the carrier turns w rad per sample from `phase`, white noise at noise_db
    relative to the symbols' unit power.  Returns (x complex128, the symbols, sps * offset in samples)."""
    rng = np.random.default_rng(seed)
    pts = points(mod)
    n_sym = int(n / sps) + 2 * span + 2
    sym = pts[rng.integers(0, pts.size, n_sym)]
    t = np.arange(n, dtype=np.float64) / sps - offset          # in symbols
    x = np.zeros(n, dtype=np.complex128)
    m0 = np.floor(t).astype(np.int64)
    for d in range(-span, span + 1):
        m = m0 + d
        x += sym[m + span] * raised_cosine(t - m, alpha)       # symbol m is stored at m + span
    x *= np.exp(1j * (w * np.arange(n) + phase))
    s = 10.0 ** (noise_db / 20.0) / math.sqrt(2.0)
    x += s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x, sym, offset * sps


def evm(symbols, mod: str) -> float:
    """Nearest-point EVM of symbols scaled to unit rms, as the constellation pass forms it."""
    y = np.asarray(symbols, dtype=np.complex128)
    y = y / math.sqrt(np.mean(np.abs(y) ** 2))
    d = np.min(np.abs(y[:, None] - points(mod)[None, :]), axis=1)
    return float(math.sqrt(np.mean(d ** 2)))
