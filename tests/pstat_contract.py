"""The contract of the power statistics (tdsa_pstat_*) in numpy: what the device must return,
bit for bit.  Everything kept is an integer, so the state of a stream is the same for any split of its samples into
calls: accumulate() may be called once or many times."""
from fractions import Fraction

import numpy as np

I8, U8, C64 = 0, 1, 2
BINS, BINS_PER_OCTAVE, EXPONENTS = 2048, 32, 256
COUNTS = ("n_total", "n_nan", "n_gated", "n_inf", "n_zero", "n_under", "n_over")
RECORD = np.dtype([(f, np.uint64) for f in COUNTS] + [("max_bits", np.uint32), ("min_bits", np.uint32),
                                                       ("reserved", np.uint32, (2,))])
U8_TABLE = (np.arange(256, dtype=np.float64) / 127.5 - 1.0).astype(np.float32)     # pyrtlsdr's float64, then float32


def unpack(x, fmt):
    """(re, im) float32 of one stream: interleaved int8 / uint8 pairs, or complex64."""
    x = np.asarray(x)
    if fmt == I8:
        v = x.astype(np.int8).reshape(-1, 2).astype(np.float32) * np.float32(0.0078125)
        return v[:, 0], v[:, 1]
    if fmt == U8:
        v = U8_TABLE[x.astype(np.uint8).reshape(-1, 2)]
        return v[:, 0], v[:, 1]
    x = x.astype(np.complex64)
    return x.real.copy(), x.imag.copy()


def power(re, im):
    """float32(float32(re re) + float32(im im)): numpy's float32 arithmetic rounds each operation once."""
    with np.errstate(all="ignore"):
        return (re * re + im * im).astype(np.float32)


class State:
    """One stream's state."""

    def __init__(self):
        self.rec = np.zeros((), dtype=RECORD)
        self.rec["min_bits"] = 0xFFFFFFFF
        self.msum = np.zeros(EXPONENTS, dtype=np.uint64)
        self.hist = np.zeros(BINS, dtype=np.uint64)

    def accumulate(self, samples, fmt, exp_lo=-40, gate=0.0):
        return self.accumulate_power(power(*unpack(samples, fmt)), exp_lo, gate)

    def accumulate_power(self, p, exp_lo=-40, gate=0.0):
        """The classes, from the float32 powers themselves."""
        p = np.ascontiguousarray(p, dtype=np.float32)
        u = p.view(np.uint32)
        rec = self.rec
        rec["n_total"] += np.uint64(p.size)
        nan = np.isnan(p)
        with np.errstate(all="ignore"):
            gated = ~nan & (p < np.float32(gate))
        rest = ~nan & ~gated
        inf = rest & (u == 0x7F800000)
        finite = rest & ~inf
        zero = finite & (u == 0)
        c5 = finite & ~zero
        b = (u[c5] >> 18).astype(np.int64) - ((int(exp_lo) + 127) << 5)
        under, over = b < 0, b >= BINS
        for name, n in (("n_nan", nan), ("n_gated", gated), ("n_inf", inf), ("n_zero", zero), ("n_under", under),
                        ("n_over", over)):
            rec[name] += np.uint64(np.count_nonzero(n))
        self.hist += np.bincount(b[~under & ~over], minlength=BINS).astype(np.uint64)
        e, f = u[c5] >> 23, (u[c5] & 0x7FFFFF).astype(np.uint64)
        mant = np.where(e >= 1, f | np.uint64(1 << 23), f)
        for k in np.unique(e):
            self.msum[k] += mant[e == k].sum(dtype=np.uint64)
        if finite.any():
            rec["max_bits"] = max(int(rec["max_bits"]), int(u[finite].max()))
        if c5.any():
            rec["min_bits"] = min(int(rec["min_bits"]), int(u[c5].min()))
        return self


def run(streams, fmt, exp_lo=-40, gate=0.0):
    """(records [C], msum [C][256], hist [C][2048]) of C streams, each given whole."""
    st = [State().accumulate(s, fmt, exp_lo, gate) for s in streams]
    return stack(st)


def stack(states):
    rec = np.zeros(len(states), dtype=RECORD)
    for i, s in enumerate(states):
        rec[i] = s.rec[()]
    return rec, np.stack([s.msum for s in states]), np.stack([s.hist for s in states])


def edges(exp_lo):
    """The 2049 bin edges, float64 (every one but 2^128 is an exact float32): 2^(exp_lo + b // 32) (1 + (b % 32) / 32)."""
    b = np.arange(BINS + 1)
    return np.ldexp(1.0 + (b % BINS_PER_OCTAVE) / BINS_PER_OCTAVE, int(exp_lo) + b // BINS_PER_OCTAVE)


def total_power(msum):
    """The exact total power of the finite samples: a Fraction."""
    t = int(msum[0]) + sum(int(msum[e]) << (e - 1) for e in range(1, EXPONENTS))
    return Fraction(t, 1 << 149)


def mean_power(rec, msum):
    counted = int(rec["n_total"]) - int(rec["n_gated"]) - int(rec["n_nan"])
    if int(rec["n_inf"]) > 0:
        return float("inf")
    if counted == 0:
        return float("nan")
    return float(total_power(msum) / counted)


def ccdf_at_edges(rec, hist):
    """[2049] P(p >= edge_k) = (sum of hist[k:] + n_over + n_inf) / counted."""
    counted = int(rec["n_total"]) - int(rec["n_gated"]) - int(rec["n_nan"])
    tail = np.concatenate([np.cumsum(hist[::-1].astype(np.uint64))[::-1], [0]]).astype(np.uint64)
    tail = tail + np.uint64(int(rec["n_over"]) + int(rec["n_inf"]))
    return tail.astype(np.float64) / float(counted) if counted else np.full(BINS + 1, np.nan)


def scaled(state, reps):
    """The state after `reps` repetitions of the samples that made `state`: counts and sums scale, the bounds stay."""
    out = State()
    for f in COUNTS:
        out.rec[f] = state.rec[f] * np.uint64(reps)
    out.rec["max_bits"], out.rec["min_bits"] = state.rec["max_bits"], state.rec["min_bits"]
    out.msum, out.hist = state.msum * np.uint64(reps), state.hist * np.uint64(reps)
    return out


# ---- constructed inputs, shared by the CPU and the GPU tests -----------------------------------------------------
def edge_set(exp_lo=-40):
    """(complex64 samples, the bin each must fall in).  Per octave j of the window, with k = (exp_lo + j) / 2 where that
    is an integer: re = 2^k and im = 2^k {0, 1/4, 1/2, 3/4} give p = 2^2k {1, 17/16, 5/4, 25/16} exactly, the edges of bins
    32 j + {0, 2, 8, 18}; and re = 2^k (1 - 2^-24), im = 2^(k - 12) give fl(re re) = 4^k (1 - 2^-23), fl(im im) = 4^k 2^-24,
    p = 4^k (1 - 2^-24): the float32 just below the octave's first edge, which belongs to bin 32 j - 1."""
    xs, bins = [], []
    for j in range(64):
        if (exp_lo + j) % 2:
            continue
        k = (exp_lo + j) // 2
        if not -60 <= k <= 60:
            continue
        a = np.float32(2.0) ** np.float32(k)
        for q, b in ((0.0, 0), (0.25, 2), (0.5, 8), (0.75, 18)):
            xs.append(complex(a, a * np.float32(q)))
            bins.append(32 * j + b)
        if j > 0:
            xs.append(complex(a * np.float32(1.0 - 2.0 ** -24), a * np.float32(2.0 ** -12)))
            bins.append(32 * j - 1)
    return np.array(xs, dtype=np.complex64), np.array(bins)


def specials():
    """(complex64 samples, the class each falls in with exp_lo = -40 and no gate): NaN in either part, a NaN part next to an
    infinite one, +-inf, zero, a denormal power (2^-140), a power above the window (2^26), 1e19 whose square stays finite, 3e19
    whose square overflows, and two parts of 1e19 whose sum stays finite."""
    inf, nan = np.inf, np.nan
    x = [complex(nan, 0), complex(0, nan), complex(inf, nan), complex(inf, 0), complex(-inf, 1), complex(0, 0), complex(-0.0, 0),
         complex(2.0 ** -70, 0), complex(2.0 ** 13, 0), complex(1e19, 0), complex(3e19, 0), complex(1e19, -1e19)]
    cls = ["n_nan", "n_nan", "n_nan", "n_inf", "n_inf", "n_zero", "n_zero", "n_under", "n_over", "n_over", "n_inf", "n_over"]
    return np.array(x, dtype=np.complex64), cls
