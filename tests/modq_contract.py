"""The modulation quality stage's contract in numpy: what tdsa_modq_* computes from a row of
complex64 symbols y and a table of reference points, operation by operation in float32 and float64, summation trees
included, so that from the same y it gives the device's bits - the record, the indices and the error vectors.  The one
exception is phase_sumsq: the arctangent is the library's own polynomial, which this file does not restate; it takes
numpy's and phase_bound() says how far the device's sum may stand from it, counted from symsync_contract.A_ATAN."""
import math

import numpy as np

from symsync_contract import A_ATAN, THREADS, U

F32, F64 = np.float32, np.float64
MIN_SYMBOLS, MAX_SYMBOLS, MAX_POINTS = 2, 4096, 64
NONFINITE, DEGENERATE, ONE_POINT = 1, 2, 4
MODULATIONS = ("bpsk", "qpsk", "8psk", "16qam", "64qam")
ROTATIONS = {"bpsk": 2, "qpsk": 4, "8psk": 8, "16qam": 4, "64qam": 4}


# ---- the table -----------------------------------------------------------------------------------------------------------
def table(name: str) -> np.ndarray:
    """[T][2] float32: analytics.constellation_points(name) rounded to float32."""
    from topdogspectrumanalyser_amd.analytics import constellation_points
    return np.ascontiguousarray(constellation_points(name), dtype=F32)


def as_table(points) -> np.ndarray:
    p = np.asarray(points)
    if np.iscomplexobj(p):
        p = np.stack([p.real, p.imag], axis=1)
    return np.ascontiguousarray(p, dtype=F32)


def uploads(tab: np.ndarray):
    """(r_abs float32 [T], inv_rho float32): sqrtf(fl(fl(re^2) + fl(im^2))) and 1 / sqrt(sum |r|^2 / T), the sum in float64
    and in index order, rounded once."""
    re, im = tab[:, 0], tab[:, 1]
    with np.errstate(over="ignore"):
        r_abs = np.sqrt((re * re + im * im).astype(F32)).astype(F32)
    power = F64(0.0)
    for a, b in tab.astype(F64):
        power = power + (a * a + b * b)
    return r_abs, F32(1.0 / math.sqrt(float(power) / tab.shape[0]))


# ---- the tree ------------------------------------------------------------------------------------------------------------
def tree_sum(values) -> float:
    """The kernel's float64 sum: thread t of 256 folds elements t, t + 256, ... in order from 0.0; the 64 partial sums of
    each wave fold by the xor butterfly, v = v + v[lane ^ o] for o = 32 .. 1; the four wave sums as (W0 + W1) + (W2 + W3)."""
    a = np.asarray(values, dtype=F64)
    rows = -(-a.size // THREADS)
    pad = np.zeros(rows * THREADS, dtype=F64)
    pad[:a.size] = a
    pad = pad.reshape(rows, THREADS)
    p = np.zeros(THREADS, dtype=F64)
    with np.errstate(all="ignore"):
        for r in range(rows):
            n = min(THREADS, a.size - r * THREADS)
            p[:n] = p[:n] + pad[r, :n]
        p = p.reshape(THREADS // 64, 64)
        lane = np.arange(64)
        o = 32
        while o >= 1:
            p = p + p[:, lane ^ o]
            o //= 2
        w = p[:, 0]
        return float((w[0] + w[1]) + (w[2] + w[3]))


# ---- the stages ----------------------------------------------------------------------------------------------------------
def first_guess(K: int, s_y, s_yy, inv_rho, mean_guess: bool = True):
    """(flags, a0, c0): a and c as (re, im) pairs of float32."""
    zero = (F32(0), F32(0))
    if not (np.isfinite(s_y[0]) and np.isfinite(s_y[1]) and np.isfinite(s_yy)):
        return NONFINITE, zero, zero
    k = F64(K)
    with np.errstate(all="ignore"):
        mr, mi = F64(s_y[0]) / k, F64(s_y[1]) / k
        v = F64(s_yy) / k - (mr * mr + mi * mi)
        a_re = F32(np.sqrt(F32(v if v > 0 else 0.0)) * F32(inv_rho))
    c0 = (F32(mr), F32(mi)) if mean_guess else zero
    return (DEGENERATE if a_re == 0 else 0), (a_re, F32(0)), c0


def inverse(a):
    """q = conj(a) / (a_re^2 + a_im^2) in float64, each part rounded to float32 once."""
    ar, ai = F64(a[0]), F64(a[1])
    with np.errstate(all="ignore"):
        n = ar * ar + ai * ai
        return F32(ar / n), F32(-ai / n)


def normalise(y: np.ndarray, c, q):
    """w = (y - c) q in float32: (w_re, w_im)."""
    with np.errstate(all="ignore"):
        tr, ti = y.real - F32(c[0]), y.imag - F32(c[1])
        rr, ii, ri, ir = tr * F32(q[0]), ti * F32(q[1]), tr * F32(q[1]), ti * F32(q[0])
        return (rr - ii).astype(F32), (ri + ir).astype(F32)


def decide(w_re, w_im, tab):
    """The lowest index of the smallest d_i; a NaN never wins, every distance NaN gives 0."""
    with np.errstate(all="ignore"):
        dr, di = w_re[:, None] - tab[None, :, 0], w_im[:, None] - tab[None, :, 1]
        d = ((dr * dr).astype(F32) + (di * di).astype(F32)).astype(F32)
    key = d.astype(F64)
    key[np.isinf(d)] = 1e300            # an infinite distance still beats a NaN
    key[np.isnan(d)] = np.inf
    return np.argmin(key, axis=1).astype(np.int64)


def count_sums(tab, counts):
    """(S_r, S_rr, n_max) in float64 and in index order."""
    sr_re = sr_im = srr = F64(0.0)
    for (re, im), n in zip(tab.astype(F64), counts):
        nd = F64(n)
        sr_re = sr_re + nd * re
        sr_im = sr_im + nd * im
        srr = srr + nd * (re * re + im * im)
    return (sr_re, sr_im), srr, int(np.max(counts))


def cmul(x, y):
    return x[0] * y[0] - x[1] * y[1], x[0] * y[1] + x[1] * y[0]


def fit(K: int, s_r, s_rr, n_max: int, s_y, s_ry):
    """(a, c) as float32 pairs, or None when every symbol is on one index or D <= 0."""
    k = F64(K)
    with np.errstate(all="ignore"):
        D = k * s_rr - (s_r[0] * s_r[0] + s_r[1] * s_r[1])
        if n_max >= K or not D > 0:
            return None
        x = cmul((s_r[0], -s_r[1]), s_y)
        num = (k * s_ry[0] - x[0], k * s_ry[1] - x[1])
        a64 = (num[0] / D, num[1] / D)
        ar = cmul(a64, s_r)
        return (F32(a64[0]), F32(a64[1])), (F32((s_y[0] - ar[0]) / k), F32((s_y[1] - ar[1]) / k))


def analyse(y, tab, mean_guess: bool = True) -> dict:
    """One segment: dict(the record's fields, indices, indices_1 (round 1's), eps complex64, p (the phase errors in half
    turns, float64 from numpy's arctangent), deciders)."""
    y = np.ascontiguousarray(y, dtype=np.complex64)
    tab = as_table(tab)
    K, T = y.size, tab.shape[0]
    r_abs, inv_rho = uploads(tab)
    yr, yi = y.real.astype(F64), y.imag.astype(F64)
    s_y = (F64(tree_sum(yr)), F64(tree_sum(yi)))
    with np.errstate(all="ignore"):
        s_yy = F64(tree_sum(yr * yr + yi * yi))
    flags, a, c = first_guess(K, s_y, s_yy, inv_rho, mean_guess)
    out = dict(a=a, c=c, s_y=s_y, s_yy=s_yy, s_ry=(0.0, 0.0), s_cy=(0.0, 0.0), err_sumsq=0.0, ref_sumsq=0.0, mag_sumsq=0.0,
               phase_sumsq=0.0, err_peak=F32(0), err_peak_k=0, changed=0, flags=flags, indices=np.zeros(K, np.uint8),
               indices_1=np.zeros(K, np.uint8), p=np.zeros(K), deciders=[])
    if flags & NONFINITE:
        out.update(s_y=(0.0, 0.0), s_yy=0.0, eps=np.full(K, complex(np.nan, np.nan), dtype=np.complex64))
        return out
    if flags & DEGENERATE:
        with np.errstate(all="ignore"):
            er, ei = (y.real - c[0]).astype(F32), (y.imag - c[1]).astype(F32)
            e2 = ((er * er).astype(F32) + (ei * ei).astype(F32)).astype(F32)
        out.update(eps=_pair(er, ei), **_peak_and_sum(e2))
        return out
    s_ry = s_cy = (F64(0), F64(0))
    s_rr = F64(0)
    rounds = []
    for _ in range(2):
        out["deciders"].append((a, c))
        w_re, w_im = normalise(y, c, inverse(a))
        i = decide(w_re, w_im, tab)
        rounds.append(i)
        rr, ri = tab[i, 0].astype(F64), tab[i, 1].astype(F64)
        with np.errstate(all="ignore"):
            s_ry = (F64(tree_sum(rr * yr + ri * yi)), F64(tree_sum(rr * yi - ri * yr)))
            s_cy = (F64(tree_sum(rr * yr - ri * yi)), F64(tree_sum(rr * yi + ri * yr)))
        s_r, s_rr, n_max = count_sums(tab, np.bincount(i, minlength=T))
        got = fit(K, s_r, s_rr, n_max, s_y, s_ry)
        if got is None:
            flags |= ONE_POINT
        else:
            a, c = got
    i = rounds[1]
    w_re, w_im = normalise(y, c, inverse(a))
    r_re, r_im = tab[i, 0], tab[i, 1]
    with np.errstate(all="ignore"):
        er, ei = (w_re - r_re).astype(F32), (w_im - r_im).astype(F32)
        e2 = ((er * er).astype(F32) + (ei * ei).astype(F32)).astype(F32)
        m = (np.sqrt(((w_re * w_re).astype(F32) + (w_im * w_im).astype(F32)).astype(F32)).astype(F32) - r_abs[i]).astype(F32)
        pre = ((w_re * r_re).astype(F32) + (w_im * r_im).astype(F32)).astype(F32)
        pim = ((w_im * r_re).astype(F32) - (w_re * r_im).astype(F32)).astype(F32)
        p = np.arctan2(pim.astype(F64), pre.astype(F64)) / np.pi
        p = np.where((r_re == 0) & (r_im == 0), 0.0, p)
        m64 = m.astype(F64)
        out.update(a=a, c=c, s_ry=s_ry, s_cy=s_cy, ref_sumsq=float(s_rr), mag_sumsq=tree_sum(m64 * m64),
                   phase_sumsq=tree_sum(p * p), changed=int(np.sum(rounds[0] != rounds[1])), flags=flags,
                   indices=i.astype(np.uint8), indices_1=rounds[0].astype(np.uint8), p=p,
                   eps=_pair(er, ei), **_peak_and_sum(e2))
    return out


def _pair(re, im):
    z = np.empty(re.size, dtype=np.complex64)      # part by part: an infinity in one part leaves the other as it is
    z.real, z.imag = re, im
    return z


def _peak_and_sum(e2):
    cand = np.where(np.isnan(e2), F32(-1), e2)
    k = int(np.argmax(cand))
    peak, k = (e2[k], k) if cand[k] > 0 else (F32(0), 0)
    return dict(err_sumsq=tree_sum(e2.astype(F64)), err_peak=F32(peak), err_peak_k=k)


def phase_bound(p, K: int) -> float:
    """|phase_sumsq_dev - phase_sumsq|: every p_k of the device stands within A_ATAN u of a half turn of the arctangent
    of the same float32 quotient, so p^2 moves by at most 2 |p| d + d^2; the float64 trees differ by their own roundings,
    below 2^-48 of the sum at K <= 4096."""
    d = A_ATAN * U
    p = np.abs(np.asarray(p, dtype=F64))
    return float(np.sum(2 * p * d + d * d)) * 1.01 + 2.0 ** -48 * float(np.sum(p * p))


# ---- the figures an analyser shows, in float64 from the record --------------------------------------------------------------
def evm_rms(r: dict) -> float:
    return math.sqrt(r["err_sumsq"] / r["ref_sumsq"])


def best_rotation_errors(indices, sent, tab, rotations: int) -> int:
    """Symbol errors of the decided indices against the sent points under the best of `rotations` turns of the table."""
    pts = tab[:, 0].astype(F64) + 1j * tab[:, 1].astype(F64)
    best = len(indices)
    for r in range(rotations):
        turned = pts[indices] * np.exp(2j * np.pi * r / rotations)
        best = min(best, int(np.sum(np.abs(turned - sent) > 1e-3)))
    return best


# ---- a segment of the library, or of the host program, against analyse() ---------------------------------------------------
def same_bits(a, b):
    """Equal bit for bit, except that a NaN matches any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    fa, fb = a.view(np.float32 if a.dtype == np.complex64 else a.dtype), b.view(np.float32 if b.dtype == np.complex64 else b.dtype)
    if fa.dtype.kind != "f":
        return np.array_equal(fa, fb)
    nan = np.isnan(fa)
    return np.array_equal(nan, np.isnan(fb)) and fa[~nan].tobytes() == fb[~nan].tobytes()


def compare(rec, idx, eps, want, where=""):
    """One segment of the library (or the host program) against the contract: bit for bit, phase_sumsq within its bound."""
    for name, key in (("a_re", "a"), ("a_im", "a"), ("c_re", "c"), ("c_im", "c")):
        assert same_bits(np.float32(rec[name]), np.float32(want[key][name.endswith("im")])), (where, name, rec[name], want[key])
    for name in ("s_y", "s_ry", "s_cy"):
        assert same_bits(rec[name], np.array([want[name][0], want[name][1]], dtype=np.float64)), (where, name, rec[name], want[name])
    for name in ("s_yy", "err_sumsq", "ref_sumsq", "mag_sumsq"):
        assert same_bits(np.float64(rec[name]), np.float64(want[name])), (where, name, rec[name], want[name])
    assert same_bits(np.float32(rec["err_peak"]), np.float32(want["err_peak"])), (where, rec["err_peak"], want["err_peak"])
    for name in ("err_peak_k", "changed", "flags"):
        assert int(rec[name]) == int(want[name]), (where, name, rec[name], want[name])
    assert np.array_equal(idx, want["indices"]), (where, np.flatnonzero(idx != want["indices"])[:8])
    if eps is not None:
        assert same_bits(eps, want["eps"]), where
    got, ref = float(rec["phase_sumsq"]), float(want["phase_sumsq"])
    if math.isnan(ref):
        assert math.isnan(got), where
    else:
        assert abs(got - ref) <= phase_bound(want["p"], idx.size), (where, got, ref, phase_bound(want["p"], idx.size))
