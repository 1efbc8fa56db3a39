"""The contract of the correlation search (tdsa_corr_*) in numpy float64: what the device must
return, and how far its float32 sums may lie from it.

windows() is the arithmetic of every complete window in float64 with the bounds the header states; matches() is the
match rule on any array of metrics - the device's own float32 trace, or the float64 restatement; decide() classifies
every window of a float64 metric as a sure match, surely none, or undecided within a given slack, which is how the
device tests prove that their inputs leave the device no freedom; Stream is one stream's state across calls, flush and
capacity included."""
import numpy as np

from pstat_contract import C64, I8, U8, unpack  # noqa: F401  (the same samples)

RECORD = np.dtype([("index", np.int64), ("metric", np.float32), ("energy", np.float32), ("c1_re", np.float32),
                   ("c1_im", np.float32), ("c2_re", np.float32), ("c2_im", np.float32)])
COUNTS = ("n_total", "n_windows", "n_decided", "n_matches", "n_lost", "n_bad")
SUMMARY = np.dtype([(f, np.uint64) for f in COUNTS] + [("flushed", np.int32), ("reserved", np.int32)])
U = 2.0 ** -24                                   # the unit roundoff of float32
F32_MAX = float(np.finfo(np.float32).max)
YES, NO, OPEN = 1, 0, -1


def samples(x, fmt):
    """complex128 of one stream's samples as the device unpacks them."""
    re, im = unpack(x, fmt)
    out = np.empty(re.size, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def reference_energy(r):
    """E_r: the float64 sum of |r[k]|^2 of the complex64 reference, rounded once to float32."""
    r = np.asarray(r, dtype=np.complex64)
    return np.float32(np.sum(r.real.astype(np.float64) ** 2 + r.imag.astype(np.float64) ** 2))


def _slide(x, r):
    """sum_k x[n + k] r[k] for every complete window, real arrays, float64."""
    if x.size < r.size:
        return np.zeros(0)
    return np.correlate(x, r, mode="valid")


def _corr(x, r):
    """(c, A_re, A_im) of sum_k x[n + k] conj(r[k]): the sums in float64, and per component the sum of the absolute
    values of its real products."""
    xr, xi, rr, ri = x.real, x.imag, r.real, r.imag
    if r.size == 0:
        z = np.zeros(max(x.size, 0))
        return z.astype(np.complex128), z, z
    with np.errstate(all="ignore"):
        c = (_slide(xr, rr) + _slide(xi, ri)) + 1j * (_slide(xi, rr) - _slide(xr, ri))
        a_re = _slide(np.abs(xr), np.abs(rr)) + _slide(np.abs(xi), np.abs(ri))
        a_im = _slide(np.abs(xi), np.abs(rr)) + _slide(np.abs(xr), np.abs(ri))
    return c, a_re, a_im


class Windows:
    """Every complete window of x (complex128) against r (complex64) in float64: c1, c2, c, e, m, bad, and the distances
    the device's float32 values may keep: b_c1, b_c2, b_c (complex: a bound per component), b_e, b_m.

    The bounds.  A sum of t float32 products accumulated in any order, fused or not, differs from the exact sum by at
    most gamma_t A, gamma_t = t u / (1 - t u), A the sum of the absolute values of the terms; the header promises twice
    the first-order figure, 2 (L + 1) u A for a component of c1 or c2 (at most L products each: both halves' components
    have 2 ceil(L / 2) <= L + 1 terms) and 2 (2 L + 1) u e for e (2 L squares).
    c = fl(c1 + c2) is one more rounding of the sum of two values that are off by b_c1 and b_c2: with q = b_c1 + b_c2 a
    component of it lies within b_c = q + u (|c| + q) of the exact c - the header bounds c1 and c2, this follows.
    m = p / d with p = c_re^2 + c_im^2, d = E_r e.  With a component of c off by at most q before that rounding
    (the rounding itself, relative u in c and so 2 u in p, is part of the 8 u below),
        |dp| <= 2 |c_re| q_re + q_re^2 + 2 |c_im| q_im + q_im^2,      |dd| <= d eps,  eps = 2 (2 L + 1) u,
        |p' / d' - p / d| <= (|dp| / d + m eps) / (1 - eps),
    and the five roundings of m itself - two squares, their sum, E_r e, the quotient - and the two of c add at most
    (5 + 2) u m in first order: the header allows 8 u m for them."""

    def __init__(self, x, r):
        x = np.asarray(x, dtype=np.complex128)
        r = np.asarray(r, dtype=np.complex64).astype(np.complex128)
        L = self.L = r.size
        H = L // 2
        self.e_ref = float(reference_energy(r))
        n = self.n = max(0, x.size - L + 1)
        with np.errstate(all="ignore"):
            c1, a1r, a1i = _corr(x[:x.size - (L - H)] if n else x[:0], r[:H])
            c2, a2r, a2i = _corr(x[H:] if n else x[:0], r[H:])
            c1, c2 = c1[:n], c2[:n]
            e = _slide(x.real ** 2, np.ones(L))[:n] + _slide(x.imag ** 2, np.ones(L))[:n] if n else np.zeros(0)
            self.c1, self.c2, self.e = c1, c2, e
            self.c = c1 + c2
            k = 2.0 * (L + 1) * U
            self.b_c1 = k * a1r[:n] + 1j * k * a1i[:n]
            self.b_c2 = k * a2r[:n] + 1j * k * a2i[:n]
            q = self.b_c1 + self.b_c2
            self.b_c = (q.real + U * (np.abs(self.c.real) + q.real)) + 1j * (q.imag + U * (np.abs(self.c.imag) + q.imag))
            eps = 2.0 * (2 * L + 1) * U
            self.b_e = eps * e
            # what float32 cannot hold is not finite on the device
            big = lambda v: ~(np.abs(v) <= F32_MAX)
            self.bad = (e == 0) | big(c1.real) | big(c1.imag) | big(c2.real) | big(c2.imag) | big(e)
            p = self.c.real ** 2 + self.c.imag ** 2
            d = self.e_ref * e
            m = np.where(self.bad, 0.0, p / np.where(self.bad, 1.0, d))
            q_re, q_im = self.b_c1.real + self.b_c2.real, self.b_c1.imag + self.b_c2.imag
            dp = 2 * np.abs(self.c.real) * q_re + q_re ** 2 + 2 * np.abs(self.c.imag) * q_im + q_im ** 2
            b_m = (dp / np.where(self.bad, 1.0, d) + m * eps) / (1.0 - eps) + 8.0 * U * m
            self.m = m
            self.b_m = np.where(self.bad, 0.0, b_m)


def _bits(m):
    """The float32 bits of m as unsigned integers, a NaN as 0x7fc00000: the order the match rule compares in."""
    m = np.asarray(m, dtype=np.float32)
    b = m.view(np.uint32).astype(np.int64)
    return np.where(np.isnan(m), 0x7fc00000, b)


def matches(m, threshold, W, n_decided=None):
    """The indices of the matches among the windows 0 .. n_decided - 1 of the metric m (all complete windows; float32):
    m[n] >= threshold, above every m[j], j in [max(0, n - W), n), at or above every m[j], j in (n, n + W] clipped at the
    last window."""
    m = np.asarray(m, dtype=np.float32)
    k = _bits(m)
    n_decided = m.size if n_decided is None else int(n_decided)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(m[:n_decided] >= np.float32(threshold))
    out = []
    for n in cand:
        left = k[max(0, n - W):n]
        right = k[n + 1:n + W + 1]
        if (left.size == 0 or left.max() < k[n]) and (right.size == 0 or right.max() <= k[n]):
            out.append(n)
    return np.array(out, dtype=np.int64)


def decide(m, slack, threshold, W):
    """[n] of YES / NO / OPEN for float64 metrics m that the device's may miss by up to slack[n] each: YES when the
    window is a match for every such set of metrics, NO when for none, OPEN otherwise."""
    m, s = np.asarray(m, dtype=np.float64), np.asarray(slack, dtype=np.float64)
    thr = float(np.float32(threshold))
    lo, hi = m - s, m + s
    out = np.full(m.size, NO, dtype=np.int8)
    for n in np.flatnonzero(hi >= thr):
        a, b = max(0, n - W), min(m.size, n + W + 1)
        sure = lo[n] >= thr and (a == n or hi[a:n].max() < lo[n]) and (n + 1 == b or hi[n + 1:b].max() < lo[n])
        never = (a < n and lo[a:n].max() > hi[n]) or (n + 1 < b and lo[n + 1:b].max() > hi[n])
        out[n] = YES if sure else NO if never else OPEN
    return out


class Stream:
    """One stream's state across calls: feed() any number of times, flush() once.  Everything is recomputed from all the
    samples so far, so no split can matter by construction."""

    def __init__(self, reference, threshold, min_distance=None, capacity=1 << 22):
        self.r = np.asarray(reference, dtype=np.complex64)
        self.L = self.r.size
        self.threshold = np.float32(threshold)
        self.W = self.L if min_distance is None else int(min_distance)
        assert 2 <= self.L <= 1024 and 0 < self.threshold <= 1 and 1 <= self.W <= 65536 and capacity >= 1
        self.capacity = int(capacity)
        self.x = np.zeros(0, dtype=np.complex128)
        self.flushed = False

    def feed(self, x, fmt=C64):
        if self.flushed:
            raise RuntimeError("the stream was flushed: it takes no samples until a reset")
        self.x = np.concatenate([self.x, samples(x, fmt)])
        return self

    def flush(self):
        self.flushed = True
        return self

    def windows(self):
        return Windows(self.x, self.r)

    def n_decided(self, n_windows):
        return n_windows if self.flushed else max(0, n_windows - self.W)

    def result(self, m=None):
        """(records, summary) with the metric m of every complete window (default: the float64 one, rounded)."""
        w = self.windows()
        m = w.m.astype(np.float32) if m is None else np.asarray(m, dtype=np.float32)
        nd = self.n_decided(w.n)
        idx = matches(m, self.threshold, self.W, nd)
        rec = np.zeros(min(idx.size, self.capacity), dtype=RECORD)
        keep = idx[:self.capacity]
        rec["index"] = keep
        rec["metric"], rec["energy"] = m[keep], w.e[keep]
        rec["c1_re"], rec["c1_im"], rec["c2_re"], rec["c2_im"] = w.c1.real[keep], w.c1.imag[keep], w.c2.real[keep], w.c2.imag[keep]
        s = np.zeros((), dtype=SUMMARY)
        s["n_total"], s["n_windows"], s["n_decided"] = self.x.size, w.n, nd
        s["n_matches"], s["n_lost"], s["n_bad"] = idx.size, max(0, idx.size - self.capacity), int(w.bad.sum())
        s["flushed"] = int(self.flushed)
        return rec, s
