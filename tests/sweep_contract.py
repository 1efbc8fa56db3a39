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
AVG_BOUND_DB = 1e-3          # the project's row allowance for the avg detector (DESIGN.md section 4.9 derives its room)


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


def interp_spelled(grid, xp, fp, locator=None) -> np.ndarray:
    """np.interp written out: every operation its own float64 rounding.  `locator(x)`, where given, stands in for the
    search of the largest j with xp[j] <= x (the mutants of the shapes suite)."""
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
            if locator is None:
                j = int(np.searchsorted(xp, x, side="right")) - 1  # the largest index with xp[j] <= x
            else:
                j = int(locator(x))
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


# ------------------------------------------------------------------------------------------------ the shapes suite
# Case builders and mutants shared by tests/test_sweep_host.py (which proves on the CPU that these very arrays tell a
# right kernel from a plausible wrong one) and tests/test_gpu_sweep_shapes.py (which feeds them to the device).
SENTINEL = 12345.0            # what lies between the rows of a padded buffer: it shows if it is ever folded in


def frame_counts(batch: int = 8):
    """F around the detector's frame loop (first frame, batches of `batch`, tail): no batch with an empty, a one-frame
    and a full tail, exactly one, two and three batches with and without a tail."""
    B = int(batch)
    return (1, 2, B - 1, B, B + 1, B + 2, 2 * B, 2 * B + 1, 3 * B + 1)


def detector_cases(block: int = 256, batch: int = 8):
    """(N, k0, k1, F, pad, byte_offset): the row length, the kept range, the frames per step, the floats between one
    step's rows and the next and the bytes the rows pointer lies past a 16-byte boundary.  A workgroup of `block` lanes
    owns 4 * block bins."""
    Fs = frame_counts(batch)
    wide, mid = 16 * block, 8 * block
    cases = []
    for k0 in range(4):                                    # every (k0 % 4, k1 % 4), the quad path, four workgroups in x
        for d in range(4):
            cases.append((wide, k0, wide - 3 + d, Fs[len(cases) % len(Fs)], 0, 0))
    # K = 1, 2, 3 inside one quad, K = 2 across a quad boundary, K = 4 as one whole quad, the whole row
    for (k0, k1), F in zip(((5, 6), (5, 7), (4, 7), (3, 5), (8, 12), (0, 64)), (Fs[4], Fs[5], Fs[7], Fs[3], Fs[1], Fs[8])):
        cases.append((64, k0, k1, F, 0, 0))
    # each cause of the bin-by-bin path on its own, two workgroups in x: the pointer, the stride, the row length
    for i, (pad, off) in enumerate(((0, 4), (0, 8), (0, 12), (1, 0), (2, 0), (3, 0))):
        cases.append((mid, 2, mid - 1, Fs[i], pad, off))
    for i in range(3):
        cases.append((mid + 2, 1, mid + 2 - i, Fs[6 + i], 0, 0))
    return cases


def case_steps(N: int) -> int:
    """Steps a detector case updates in one call: blockIdx.y of the launch."""
    return 3 if N <= 64 else 2


def takes_quads(N: int, F: int, pad: int, byte_offset: int) -> bool:
    """Whether launch_sweep_detector lets the kernel load 16 bytes at a time (for a buffer on a 16-byte boundary)."""
    return byte_offset % 16 == 0 and N % 4 == 0 and (F * N + pad) % 4 == 0


def spiky_rows(S: int, F: int, N: int, seed: int):
    """([S][F][N] float32, special [S][F][N] bool) for sample / max / min.  Outside `special` every value of a step's
    F x N block is distinct, bin b has its maximum in frame (b + s) % F and its minimum in frame (b + s + 1) % F, each
    unique, so a frame left out, taken twice or taken from a neighbouring bin changes the result.  `special` marks a
    sprinkling of NaN, -inf, +299 and -299.  No value is a zero: np.max does not fix which zero it returns where a bin
    holds zeros of both signs, so the contract does not either, and the suite keeps away from it."""
    rng = np.random.default_rng(seed)
    n = F * N
    rows = np.empty((S, F, N), dtype=np.float32)
    b = np.arange(N)
    for s in range(S):
        body = (-120.0 + 60.0 * (rng.permutation(n) + 0.5) / n).astype(np.float32)     # (-120, -60), 60 / n apart
        rows[s] = body.reshape(F, N)
        rows[s, (b + s) % F, b] = (10.0 + 1e-3 * b).astype(np.float32)
        if F > 1:
            rows[s, (b + s + 1) % F, b] = (-200.0 - 1e-3 * b).astype(np.float32)
    special = np.zeros(rows.shape, dtype=bool)
    for value in (np.nan, -np.inf, 299.0, -299.0):
        hit = rng.random(rows.shape) < 0.002
        rows[hit] = value
        special |= hit
    return rows, special


def level_rows(S: int, F: int, N: int, seed: int) -> np.ndarray:
    """[S][F][N] float32 for avg: every bin at a level of its own in [-140, 40) dB, its frames within 6 dB above it, so
    that every frame carries at least a quarter of the largest frame's power and none can go missing unnoticed."""
    rng = np.random.default_rng(seed)
    level = -140.0 + 180.0 * rng.random((S, 1, N))
    return (level + 6.0 * rng.random((S, F, N))).astype(np.float32)


def special_rows(S: int, F: int, N: int, seed: int) -> np.ndarray:
    """Level rows whose bin b carries pattern b % 16 of the special values: a NaN in the first, a middle or the last
    frame or in all, -inf in all frames (no power: avg gives -300), in all but one and in one, +-299 in all frames and
    in one, NaN beside -inf."""
    rows = level_rows(S, F, N, seed)
    b = np.arange(N)
    last, mid = F - 1, F // 2

    def put(pattern, frames, value):
        for f in frames:
            rows[:, f, b[b % 16 == pattern]] = value

    put(0, [0], np.nan)
    put(1, [last], np.nan)
    put(2, [mid], np.nan)
    put(3, range(F), np.nan)
    put(4, range(F), -np.inf)
    put(5, range(1, F), -np.inf)
    put(6, [0], -np.inf)
    put(7, range(F), 299.0)
    put(8, range(F), -299.0)
    put(9, [mid], 299.0)
    put(10, [last], -299.0)
    put(11, range(F), -np.inf)
    put(11, [mid], np.nan)
    return rows


def lay_out(rows: np.ndarray, pad: int, byte_offset: int):
    """(buf float32 1-D, step_stride_floats): the rows [S][F][N] at byte_offset into a buffer, pad floats between the
    steps, SENTINEL wherever no row lies."""
    S, F, N = rows.shape
    stride, lead = F * N + int(pad), int(byte_offset) // 4
    buf = np.full(lead + S * stride, SENTINEL, dtype=np.float32)
    body = buf[lead:].reshape(S, stride)
    body[:, :F * N] = rows.reshape(S, F * N)
    return buf, stride


# ---- stitch geometries
STITCH_GEOMETRIES = ("inexact", "k1", "k2", "k3", "steps4096")


def stitch_geometry(name: str):
    """(N, k0, k1, bin_hz, centres): fs = 1e6 throughout and bin_hz = 1.0 / (N * (1.0 / fs)) as Python passes it; the
    first kept bin of the first step lies at 0 Hz, where the products are small against their own rounding and a fused
    multiply-add shows.  `inexact` has a gap of 37.3 bins after step 4, the others have abutting steps."""
    fs = 1e6
    N, k0, k1, S, gap = {"inexact": (768, 96, 672, 9, 37.3), "k1": (768, 383, 384, 300, 0.0), "k2": (768, 383, 385, 40, 0.0),
                         "k3": (768, 382, 385, 40, 0.0), "steps4096": (8, 2, 6, 4096, 0.0)}[name]
    bin_hz = 1.0 / (N * (1.0 / fs))
    K = k1 - k0
    bins = (N // 2 - k0) + np.arange(S, dtype=np.float64) * K
    bins[5:] += gap
    return N, k0, k1, bin_hz, bins * bin_hz


def stitch_T(S: int, K: int, seed: int, gap_after: int = 4) -> np.ndarray:
    """[S][K] float32 noise with NaN and infinities sprinkled, and placed next to step boundaries and next to the gap."""
    rng = np.random.default_rng(seed)
    T = (-95 + 12 * rng.standard_normal((S, K))).astype(np.float32)
    T[rng.random(T.shape) < 0.003] = np.nan
    T[rng.random(T.shape) < 0.003] = np.inf
    T[rng.random(T.shape) < 0.003] = -np.inf
    T[1, K - 1] = np.nan
    T[2, 0] = np.inf
    T[gap_after, K - 1] = -np.inf
    T[gap_after + 2, 0] = np.nan
    T[gap_after + 3, K - 1] = np.inf
    return T


def ramp_T(S: int, K: int, gap_after: int = 4) -> np.ndarray:
    """[S][K] float32 for cells of many bins, where noise with NaN sprinkled would leave NaN in every cell: rising over
    the first half of the bins, falling over the second, all values distinct, so the maximum of a cell is the bin at
    its upper edge in one half and at its lower edge in the other; one NaN and two -inf next to step boundaries."""
    n = S * K
    j = np.arange(n, dtype=np.float64)
    T = (-100.0 + 100.0 * np.minimum(j, n - 0.5 - j) / n).astype(np.float32).reshape(S, K)
    T[1, K - 1] = np.nan
    T[gap_after, K - 1] = -np.inf
    T[gap_after + 2, 0] = -np.inf
    return T


def present_sets(name: str, S: int, block: int = 256):
    """{tag: present[S] bool}; for k1 also sets of block - 1, block and block + 1 steps, a run missing in the middle."""
    sets = {"all": np.ones(S, dtype=bool), "ends_missing": np.ones(S, dtype=bool), "every_other": np.zeros(S, dtype=bool)}
    sets["ends_missing"][[0, S - 1]] = False
    sets["every_other"][::2] = True
    if name == "k1":
        for n in (block - 1, block, block + 1):
            p = np.ones(S, dtype=bool)
            p[100:100 + S - n] = False
            sets[f"n{n}"] = p
    return sets


def ulp_grid(xp: np.ndarray, K: int, bin_hz: float, cap: int = 60000) -> np.ndarray:
    """Every xp, its neighbours one ulp below and above and the midpoint of every gap between steps, ascending, with two
    points below the first bin (one bin apart: they fix the peak cell) and two above the last.  Beyond `cap` points the
    bins inside the steps are thinned, the first and last bin of every step stay."""
    xp = np.asarray(xp, dtype=np.float64)
    idx = np.arange(xp.size)
    room = (cap - 4 - xp.size // K) // 3                   # bins the cap admits, each with its two neighbours
    if xp.size > room:
        inner = np.linspace(0, xp.size - 1, max(room - 2 * (xp.size // K), 2)).astype(np.int64)
        idx = np.unique(np.concatenate([inner, idx[::K], idx[K - 1::K]]))
    x = xp[idx]
    mids = 0.5 * (xp[K - 1:-1:K] + xp[K::K])
    body = np.unique(np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), mids]))
    below = [xp[0] - 2.5 * bin_hz, xp[0] - 1.5 * bin_hz]
    above = [xp[-1] + 0.5 * bin_hz, xp[-1] + 7.25 * bin_hz]
    return np.concatenate([below, body, above])


def long_grid(xp: np.ndarray, bin_hz: float, n: int) -> np.ndarray:
    return np.linspace(xp[0] - 5.0 * bin_hz, xp[-1] + 5.0 * bin_hz, int(n))


def cells_grid(xp: np.ndarray, bins_per_cell: float, bin_hz: float) -> np.ndarray:
    """A grid for peak mode.  grid[0] and grid[1], below every cell that holds a bin, fix h; the other points are
    xp[j] - h / 2 and xp[j] + h / 2 with their neighbours one ulp either side, ascending, so that cell edges fall on a
    bin, one ulp below it and one ulp above it: the lower edge belongs to the cell, the upper edge does not."""
    xp = np.asarray(xp, dtype=np.float64)
    g0 = xp[0] - 3.0 * bins_per_cell * bin_hz
    g1 = g0 + bins_per_cell * bin_hz
    half = 0.5 * (g1 - g0)
    mid = np.concatenate([xp - half, xp + half])
    body = np.unique(np.concatenate([mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)]))
    assert body[0] > g1
    return np.concatenate([[g0, g1], body])


def stitch_cases(block: int = 256):
    """(geometry, present set, grid) of every stitch case.  Grids: `ulp`, `cells8` (cells of about 8 bins), `cellswide`
    (about 3.5 K bins, a cell spans whole steps), `long` (a second round of the grid-stride loop), `lin3000`."""
    cases = []
    for name in STITCH_GEOMETRIES[:-1]:
        for tag in present_sets(name, len(stitch_geometry(name)[4]), block):
            cases += [(name, tag, grid) for grid in ("ulp", "cells8", "cellswide")]
    cases += [("inexact", "all", "long"), ("k1", f"n{block + 1}", "long")]
    cases += [("steps4096", "all", "ulp"), ("steps4096", "all", "lin3000")]    # loaded with one call: all present
    return cases


def stitch_inputs(name: str, present_tag: str, grid_tag: str, block: int = 256, max_blocks: int = 2048):
    """(N, k0, k1, bin_hz, centres, T, present, grid) of one stitch case.  T is stitch_T's noise with NaN and infinities,
    except on `cellswide`, where it is ramp_T (see there)."""
    N, k0, k1, bin_hz, centres = stitch_geometry(name)
    S, K = len(centres), k1 - k0
    present = present_sets(name, S, block)[present_tag]
    xp = frequencies(centres[present], k0, k1, N, bin_hz)
    T = ramp_T(S, K) if grid_tag == "cellswide" else stitch_T(S, K, seed=S + K)
    if grid_tag == "ulp":
        grid = ulp_grid(xp, K, bin_hz)
    elif grid_tag == "cells8":
        grid = cells_grid(xp, 8.0, bin_hz)
    elif grid_tag == "cellswide":
        grid = cells_grid(xp, 3.5 * K, bin_hz)
    elif grid_tag == "long":
        grid = long_grid(xp, bin_hz, block * max_blocks + block + 1)
    elif grid_tag == "lin3000":
        grid = np.linspace(xp[0] - 2.0 * bin_hz, xp[-1] + 2.0 * bin_hz, 3000)
    else:
        raise ValueError(grid_tag)
    return N, k0, k1, bin_hz, centres, T, present, grid


# ---- mutants: plain numpy restatements of plausible wrong kernels, for the CPU half only
def frequencies_fused(centres, k0: int, k1: int, nfft: int, bin_hz: float) -> np.ndarray:
    """xp with one rounding per bin, as fma(k - N/2, bin_hz, centre) gives it (exact rationals, rounded once)."""
    from fractions import Fraction
    b = Fraction(float(bin_hz))
    return np.array([float(Fraction(float(c)) + (k - int(nfft) // 2) * b)
                     for c in np.asarray(centres, dtype=np.float64) for k in range(int(k0), int(k1))])


def locate(x, xp) -> np.ndarray:
    """The contract's locator: the largest linear index j with xp[j] <= x (x >= xp[0])."""
    return np.searchsorted(xp, x, side="right") - 1


def locate_by_guess(x, xp, K: int, bin_hz: float) -> np.ndarray:
    """The step by exact comparison, the bin by int((x - x_first) * (1 / bin_hz)) and no correction."""
    x = np.asarray(x, dtype=np.float64)
    first = xp[::K]
    p = np.searchsorted(first, x, side="right") - 1
    t = (x - first[p]) * (1.0 / bin_hz)
    k = np.where(t >= K - 1, K - 1, t.astype(np.int64))
    return p * K + k


def detector_skipping(rows, k0: int, k1: int, det: str, f: int) -> np.ndarray:
    """The detector of a frame loop that never takes frame f (and still divides by F).  For sample only the last frame
    can go missing: the one before it is taken."""
    r = np.asarray(rows, dtype=np.float32)
    F = r.shape[0]
    if det == "sample":
        return r[max(F - 2, 0), int(k0):int(k1)].copy() if f == F - 1 else detector(r, k0, k1, det)
    rest = np.delete(r, f, axis=0)[:, int(k0):int(k1)]
    if det in ("max", "min"):
        fill = -np.inf if det == "max" else np.inf
        return (np.max if det == "max" else np.min)(rest, axis=0, initial=fill).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        acc = np.sum(np.power(10.0, rest.astype(np.float64) / 10.0), axis=0)
        return 10.0 * np.log10(np.maximum(acc / F, 1e-30))


def detector_quad_shifted(rows, k0: int, k1: int, det: str, block_bins: int = 1024) -> np.ndarray:
    """The detector whose workgroups after the first look one quad too far: bins at block_bins past the first quad and
    beyond take the fold of the bin four further on (the last four stay)."""
    T = detector(rows, k0, k1, det)
    out = T.copy()
    j = block_bins - int(k0) % 4
    if len(T) > j + 4:
        out[j:-4] = T[j + 4:]
    return out


def stitch_upper_closed(grid, xp, fp) -> np.ndarray:
    """peak with the cell [g - h / 2, g + h / 2]: the upper edge closed."""
    grid = np.asarray(grid, dtype=np.float64)
    fp = np.asarray(fp).astype(np.float64)
    out = np.interp(grid, xp, fp)
    h = grid[1] - grid[0]
    lo = np.searchsorted(xp, grid - 0.5 * h, side="left")
    hi = np.searchsorted(xp, grid + 0.5 * h, side="right")
    for i in range(grid.size):
        if hi[i] > lo[i]:
            out[i] = np.max(fp[lo[i]:hi[i]])
    return out


def assemble_table_cut(T, present, centres, k0, k1, nfft, bin_hz, grid, mode="interp", n_tab: int = 256) -> np.ndarray:
    """The stitch of a step table that holds only its first n_tab entries: later present steps do not exist."""
    present = np.asarray(present, dtype=bool).copy()
    present[np.nonzero(present)[0][n_tab:]] = False
    return assemble(T, present, centres, k0, k1, nfft, bin_hz, grid, mode)
