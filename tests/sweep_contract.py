"""The sweep assembler's contract, restated in numpy float64.

Geometry: S steps with centres c_s (float64 Hz, ascending), frame length N, bin width bin_hz, kept range [k0, k1) of
the fftshift-ed row.  Kept bin k of step s lies at x = c_s + (k - N/2) * bin_hz: one multiply, one add.
  detector   rows[f][k] float32 dB of one step -> T[k - k0] float32: the last frame, np.max / np.min over the frames,
             or 10 log10(max(mean_f(10^(d_f / 10)), 1e-30)) with the frames summed in frame order
  interp     np.interp(grid, xp, fp) with xp the concatenated frequencies of the steps present and fp their T as float64
             (HackRFSweepDataSource._parse), spelled out operation by operation in interp_spelled()
  peak       out[i] = max of fp over grid[i] - 0.5 h <= xp < grid[i] + 0.5 h, h = grid[1] - grid[0]; a NaN in the cell
             gives NaN, an empty cell takes the interp value
With no step present every output is NaN.
"""
import numpy as np

DETECTORS = ("sample", "max", "min", "avg")


def frequencies(centres, k0: int, k1: int, nfft: int, bin_hz: float) -> np.ndarray:
    """xp of all steps, [S * K] float64."""
    off = (np.arange(int(k0), int(k1)) - int(nfft) // 2).astype(np.float64) * np.float64(bin_hz)     # the multiply ...
    return (np.asarray(centres, dtype=np.float64).reshape(-1, 1) + off.reshape(1, -1)).reshape(-1)   # ... then the add


def detector(rows: np.ndarray, k0: int, k1: int, det: str) -> np.ndarray:
    """rows [F][N] float32 of one step -> T [K].  float32 (exact) for sample / max / min, float64 for avg."""
    r = np.asarray(rows, dtype=np.float32)[:, int(k0):int(k1)]
    if det == "sample":
        return r[-1].copy()
    if det == "max":
        return np.max(r, axis=0)
    if det == "min":
        return np.min(r, axis=0)
    if det == "avg":
        acc = np.zeros(r.shape[1], dtype=np.float64)
        with np.errstate(over="ignore", under="ignore"):
            for f in range(r.shape[0]):
                acc = acc + np.power(10.0, r[f].astype(np.float64) / 10.0)
            return 10.0 * np.log10(np.maximum(acc / r.shape[0], 1e-30))
    raise ValueError(det)


def interp_spelled(grid, xp, fp) -> np.ndarray:
    """np.interp written out: every operation its own float64 rounding."""
    xp = np.asarray(xp, dtype=np.float64)
    fp = np.asarray(fp, dtype=np.float64)
    out = np.empty(len(grid), dtype=np.float64)
    n = len(xp)
    with np.errstate(all="ignore"):
        for i, x in enumerate(np.asarray(grid, dtype=np.float64)):
            if x < xp[0]:
                out[i] = fp[0]
                continue
            if x > xp[-1]:
                out[i] = fp[-1]
                continue
            j = int(np.searchsorted(xp, x, side="right")) - 1      # the largest index with xp[j] <= x
            if j == n - 1 or xp[j] == x:
                out[i] = fp[j]
                continue
            slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
            r = slope * (x - xp[j]) + fp[j]
            if np.isnan(r):
                r = slope * (x - xp[j + 1]) + fp[j + 1]
                if np.isnan(r) and fp[j] == fp[j + 1]:
                    r = fp[j]
            out[i] = r
    return out


def stitch(grid, xp, fp, mode: str = "interp") -> np.ndarray:
    """The trace on the grid from the present steps' (xp, fp); fp float32 or float64."""
    grid = np.asarray(grid, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    fp = np.asarray(fp).astype(np.float64)
    if xp.size == 0:
        return np.full(grid.size, np.nan)
    out = np.interp(grid, xp, fp)
    if mode == "interp":
        return out
    if mode != "peak":
        raise ValueError(mode)
    h = grid[1] - grid[0]
    lo = np.searchsorted(xp, grid - 0.5 * h, side="left")          # first xp >= lower bound
    hi = np.searchsorted(xp, grid + 0.5 * h, side="left")          # first xp >= upper bound
    for i in range(grid.size):
        if hi[i] > lo[i]:
            out[i] = np.max(fp[lo[i]:hi[i]])                        # np.max keeps a NaN
    return out


def assemble(T, present, centres, k0, k1, nfft, bin_hz, grid, mode="interp") -> np.ndarray:
    """Stitch of the steps flagged in `present`; T [S][K]."""
    present = np.asarray(present, dtype=bool)
    K = int(k1) - int(k0)
    xp = frequencies(np.asarray(centres)[present], k0, k1, nfft, bin_hz) if present.any() else np.empty(0)
    fp = np.asarray(T).reshape(len(present), K)[present].reshape(-1)
    return stitch(grid, xp, fp, mode)
