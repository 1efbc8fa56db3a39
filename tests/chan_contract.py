"""The channelizer's contract, restated in numpy float64.

Inputs count from the last reset, across calls: n = 0, 1, ...
  x[n]    the existing unpack (zoom_contract.unpack), 0 for n < 0
  M, os   channels (a power of two) and oversampling; D = M / os
  y_c[m]  sum_{k < T} h[k] x[mD - k] exp(-2 pi j c (mD - k) / M), c = 0 .. M - 1: zoom_contract's down-converter at
          phase step c 2^32 / M with decimation D; output m is emitted by the call that delivers input m D, so n_total
          inputs give ceil(n_total / D) outputs per channel
and as the device evaluates it, with P = ceil(T / M):
  w_m[r]  sum_{q < P} h[qM + r] x[mD - qM - r]
  W_m[p]  w_m[r] at p = (r - mD) mod M
  y_c[m]  sum_p W_m[p] exp(+2 pi j c p / M)
Every array of outputs here is channel-major, [M][n_out], as the device stores it.

Non-finite samples: zoom_contract's rule with the padded window H = P M.  x[n*] reaches instant m through one branch,
and the transform spreads it over every channel of that instant: where h[mD - n*] != 0 all M channels are non-finite,
outside (mD - P M, mD] no channel of instant m changes a bit."""
import numpy as np

from zoom_contract import FMT_C64, FMT_I8, FMT_U8, hit_outputs, n_outputs, padded_window_outputs, unpack  # noqa: F401


def branch_taps(T: int, M: int) -> int:
    return -(-int(T) // int(M))


def _windows(x, T, M, D):
    """[n_out][P M]: x[mD - k] for k < P M (0 before the stream starts)."""
    PM = branch_taps(T, M) * M
    xp = np.concatenate([np.zeros(PM, dtype=x.dtype), x])
    m = np.arange(n_outputs(len(x), D))
    return xp[m[:, None] * D + PM - np.arange(PM)[None, :]]


def _pad(h, M):
    h = np.asarray(h)
    out = np.zeros(branch_taps(h.size, M) * M, dtype=h.dtype)
    out[:h.size] = h
    return out


def _shift(w, M, D):
    """[n_out][M] branch sums w_m[r] -> [M][n_out] W_m[p], p = (r - mD) mod M."""
    m = np.arange(w.shape[0])
    p = (np.arange(M)[None, :] - m[:, None] * D) % M
    W = np.empty_like(w)
    np.put_along_axis(W, p, w, axis=1)
    return W.T.copy()


def direct(x, h, M: int, os: int) -> np.ndarray:
    """y_c[m] as the defining sum: mix with channel c's phase, filter, keep every D-th (float64)."""
    D = M // os
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h, dtype=np.float64)
    n = np.arange(len(x), dtype=np.int64)
    out = np.empty((M, n_outputs(len(x), D)), dtype=np.complex128)
    for c in range(M):
        v = x * np.exp(-2j * np.pi * ((c * n) % M).astype(np.float64) / M)
        out[c] = np.convolve(v, h)[::D][:out.shape[1]]
    return out


def branches(x, h, M: int, os: int) -> np.ndarray:
    """W_m[p], [M][n_out] (float64)."""
    D = M // os
    hp = _pad(np.asarray(h, dtype=np.float64), M)
    g = _windows(np.asarray(x).astype(np.complex128), len(h), M, D) * hp[None, :]
    return _shift(g.reshape(g.shape[0], -1, M).sum(axis=1), M, D)


def transform(W) -> np.ndarray:
    """y_c[m] = sum_p W_m[p] exp(+2 pi j c p / M) of [M][n_out] branch sums."""
    M = W.shape[0]
    k = np.arange(M)
    E = np.exp(2j * np.pi * ((k[:, None] * k[None, :]) % M).astype(np.float64) / M)
    return E @ W


def restated(x, h, M: int, os: int) -> np.ndarray:
    return transform(branches(x, h, M, os))


def abs_branches(x, h, M: int, os: int) -> np.ndarray:
    """a_m[r] = sum_q |h[qM + r]| |x[mD - qM - r]|, [n_out][M] (what an fma chain's rounding error scales with)."""
    D = M // os
    hp = np.abs(_pad(np.asarray(h, dtype=np.float64), M))
    g = np.abs(_windows(np.asarray(x).astype(np.complex128), len(h), M, D)) * hp[None, :]
    return g.reshape(g.shape[0], -1, M).sum(axis=1)


def integer_branches(re, im, h, M: int, os: int):
    """W_m[p] of integer-valued x = re + j im and integer-valued taps, exactly, in int64: (real, imag), [M][n_out]."""
    D = M // os
    hi = np.asarray(h).astype(np.int64)
    assert np.array_equal(hi, np.asarray(h)), "taps must be integers"
    hp = _pad(hi, M)
    out = []
    for part in (re, im):
        g = _windows(np.asarray(part, dtype=np.int64), len(hi), M, D) * hp[None, :]
        out.append(_shift(g.reshape(g.shape[0], -1, M).sum(axis=1), M, D))
    return out[0], out[1]


def integer_channel(Wr, Wi, c: int):
    """Channel c of integer branch sums where every twiddle is 1, -1, j or -j (c M / 4 ... any c with 4 c p / M whole
    for all p: c = 0 and M / 2 always, every c at M = 4), exactly, in int64."""
    M = Wr.shape[0]
    yr = np.zeros(Wr.shape[1], np.int64)
    yi = np.zeros(Wr.shape[1], np.int64)
    for p in range(M):
        assert (4 * c * p) % M == 0, (c, p, M)
        q = (4 * c * p // M) % 4                      # twiddle j^q
        a, b = Wr[p], Wi[p]
        if q == 0:
            yr += a; yi += b
        elif q == 1:
            yr -= b; yi += a
        elif q == 2:
            yr -= a; yi -= b
        else:
            yr += b; yi -= a
    return yr, yi
