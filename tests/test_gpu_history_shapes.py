"""The 3-D history views on the MI355X at the shapes their kernels branch on (tests/history_cases.py builds the rows,
tests/test_history_host.py proves what the rows claim): batches that give a workgroup several rows, bin counts that take
one-bin lanes over several waves and workgroups, rows whose maximum lies below zero, column counts next to the widths at
which the reduction changes its group, heights on integers, hues on sextant boundaries, levels on the limits of the
surface - and what one NaN bin leaves alone.  HistoryModel of tests/history_contract.py is the reference; every
comparison is np.array_equal on arrays of the same dtype and shape."""
import numpy as np
import pytest

import history_cases as cases
import history_contract as hc
from topdogspectrumanalyser_amd import DeviceBuffer, TraceHistory

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same_but(a, b, at=()):
    """_same outside the elements `at` (indices of the leading axes), which the contract leaves unspecified."""
    a, b = np.array(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    for i in at:
        a[i] = b[i]
    return np.array_equal(a, b)


def _peak_same(a, b):
    return int(a[0]) == int(b[0]) and _same(np.float32(a[1]), np.float32(b[1]))


class Open:
    """What a NaN leaves unspecified in one comparison: (view row, column) elements, columns of the hold and min rows,
    the two peaks.  Nothing by default."""

    def __init__(self, cells=(), hold=(), min=(), live_peak=False, hold_peak=False):
        self.cells, self.hold, self.min = list(cells), [(c,) for c in hold], [(c,) for c in min]
        self.live_peak, self.hold_peak = live_peak, hold_peak

    def view(self, first, count):
        """The open elements of lines first .. first + count - 1."""
        return [(r - first, c) for r, c in self.cells if first <= r < first + count]


NOTHING = Open()


def _check_ribbon(h, m, x, columns=None, what="", open_=NOTHING):
    v, w = h.ribbon(x, columns), m.ribbon(x, columns)
    print(f"ribbon {what} n={h.n_bins} depth={h.depth} columns={columns}: verts {v['verts'].shape}, "
          f"differing verts {(v['verts'] != w['verts']).sum()}, colours {(v['colours'] != w['colours']).sum()}")
    at = [(r, slice(2 * c, 2 * c + 2)) for r, c in open_.view(0, v["verts"].shape[0])]
    assert _same_but(v["verts"], w["verts"], at) and _same_but(v["colours"], w["colours"], at)
    if columns is not None:
        assert _same_but(v["bins"], w["bins"], open_.view(0, v["bins"].shape[0]))
    return v


def _check_lines(h, m, columns=None, first=0, count=None, what="", open_=NOTHING):
    for mode in ("index", "rgba"):
        v, w = h.lines(first, count, mode, columns), m.lines(first, count, columns)
        print(f"lines {what} n={h.n_bins} depth={h.depth} columns={columns} {first}+{count} {mode}: z {v['z'].shape}, "
              f"differing z {(v['z'] != w['z']).sum()}, colours {(v[mode] != w[mode]).sum()}, "
              f"hold {(v['hold'] != w['hold']).sum()}, peaks {v['live_peak']} / {w['live_peak']}, "
              f"{v['hold_peak']} / {w['hold_peak']}")
        at = open_.view(first, v["z"].shape[0])
        assert _same_but(v["z"], w["z"], at) and _same_but(v[mode], w[mode], at)
        assert _same_but(v["hold"], w["hold"], open_.hold)
        assert open_.live_peak or _peak_same(v["live_peak"], w["live_peak"])
        assert open_.hold_peak or _peak_same(v["hold_peak"], w["hold_peak"])
        assert (v["min"] is None) == (w["min"] is None)
        if w["min"] is not None:
            assert _same_but(v["min"], w["min"], open_.min)
        if columns is not None:
            assert _same_but(v["bins"], w["bins"], at) and _same_but(v["hold_bins"], w["hold_bins"], open_.hold)
            if w["min"] is not None:
                assert _same_but(v["min_bins"], w["min_bins"], open_.min)
    return v


def _check_surface(h, m, columns=None, what="", open_=NOTHING):
    v, w = h.surface(columns), m.surface(columns)
    print(f"surface {what} n={h.n_bins} depth={h.depth} columns={columns}: z {v['z'].shape}, differing z "
          f"{(v['z'] != w['z']).sum()}, colours {(v['colours'] != w['colours']).sum()}, peak {v['live_peak']} / "
          f"{w['live_peak']}, norm {v['peak_norm']!r} / {w['peak_norm']!r}")
    at = open_.view(0, v["z"].shape[0])
    assert _same_but(v["z"], w["z"], at) and _same_but(v["colours"], w["colours"], at)
    assert open_.live_peak or (_peak_same(v["live_peak"], w["live_peak"]) and v["peak_norm"] == w["peak_norm"])
    if columns is not None:
        assert _same_but(v["bins"], w["bins"], at)
    return v


def _x(n):
    return np.linspace(-10, 10, n, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- row chunks
@pytest.mark.parametrize("depth", cases.CHUNK_DEPTHS)
@pytest.mark.parametrize("n,n_rows", cases.CHUNK_SHAPES)
def test_a_batch_that_gives_a_workgroup_several_rows(n, n_rows, depth):
    """Catches: rows older than the ring stored into it (or kept out of the hold), a hold that starts afresh with every
    row of a chunk, a ring wrap or the first stored row inside a chunk going to the wrong slot, a short last chunk
    reading past the batch, a hold that one chunk overwrites instead of raising."""
    case = cases.chunk_case(n, n_rows, depth)
    gx, gy, rows_per_wg, last = case["geometry"]
    print(f"n={n} rows={n_rows} depth={depth}: grid ({gx}, {gy}), {rows_per_wg} rows a workgroup, {last} in the last, "
          f"skip {case['skip']}")
    assert rows_per_wg >= 2 and last < rows_per_wg and case["skip"] > 0
    first, batch, P = case["first"], case["batch"], cases.CHUNK_COLUMNS
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s, DeviceBuffer(batch.nbytes) as d:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for t in (h, m, s, ms):
            t.set_amplitude(*cases.CHUNK_AMPLITUDE)
            t.push(first)                          # head = 1: the ring wraps inside a chunk
        d.put(batch)
        h.push_rows(None, d.ptr, n_rows)
        s.push_rows(None, d.ptr, n_rows)
        m.push_rows(batch)
        ms.push_rows(batch)
        v = _check_lines(h, m, what="chunks")
        assert v["pushed"] == n_rows + 1 and v["valid"] == depth
        _check_lines(h, m, P, what="chunks")
        _check_ribbon(h, m, _x(n), what="chunks")
        _check_ribbon(h, m, _x(n), P, what="chunks")
        _check_surface(s, ms, what="chunks")
        _check_surface(s, ms, P, what="chunks")
        # a maximum from a skipped row is in the hold row and in no line
        cols = case["classes"]["skipped"]
        held = hc.heights(batch[[case["planted"][int(c)] for c in cols], cols], *cases.CHUNK_AMPLITUDE)
        assert _same(v["hold"][cols], held) and (v["z"][:, cols] < held).all()
        for name in ("chunk_end", "chunk_start"):
            cols = case["classes"][name]
            held = hc.heights(batch[[case["planted"][int(c)] for c in cols], cols], *cases.CHUNK_AMPLITUDE)
            assert _same(v["hold"][cols], held)


# ---------------------------------------------------------------------------------------------------- one-bin lanes
@pytest.mark.parametrize("n", cases.ONE_BIN_N)
def test_one_bin_lanes_over_waves_and_workgroups(n):
    """Catches: a scalar instantiation that indexes rows, lanes or records as the 16-byte one does (gid / per_row, the
    strides of the interleaved stores), a dead lane of the last wave that stores or wins the row maximum."""
    depth, P = cases.ONE_BIN_DEPTH, cases.one_bin_columns(n)
    rows = cases.generic_rows(np.random.default_rng(n), depth + 4, n)
    assert cases.lane_width(n) == 1 and P % 4 != 0
    with TraceHistory(depth, n) as a, TraceHistory(depth, n) as b, TraceHistory(depth, n, "levels") as sa, \
            TraceHistory(depth, n, "levels") as sb, DeviceBuffer(rows.nbytes) as d:
        ma, mb, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for t in (a, b, ma, mb, sa, sb, ms):
            t.set_amplitude(-5.0, 85.0)
        for i, r in enumerate(rows):               # host pushes, with a min trace
            mn = np.minimum.reduce(rows[:i + 1])
            for t in (a, ma):
                t.push(r, None, mn)
            for t in (sa, ms):
                t.push(r)
        d.put(rows)
        b.push(rows[0])                            # one host row, the others as a batch
        b.push_rows(None, d.at(4 * n), depth + 3)
        sb.push_rows(None, d.ptr, depth + 4)
        mb.push_rows(rows)
        for columns in (None, P):
            _check_lines(a, ma, columns, what="host")
            _check_lines(b, mb, columns, what="batch")
            _check_lines(a, ma, columns, first=1, count=3, what="host")
            _check_ribbon(a, ma, _x(n), columns, what="host")
            _check_ribbon(b, mb, _x(n), columns, what="batch")
            _check_surface(sa, ms, columns, what="host")
            _check_surface(sb, ms, columns, what="batch")


@pytest.mark.parametrize("n", cases.MISALIGNED_N)
def test_a_batch_from_a_pointer_off_the_16_byte_grid(n):
    """A bin count that is a multiple of 4 behind a pointer that is not: one-bin lanes, the bits of the aligned push, and
    nothing read before or after the rows (+inf there would show as z = 8 and in the hold)."""
    depth, n_rows = 5, 9
    rows = cases.generic_rows(np.random.default_rng(n + 1), n_rows, n)
    m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
    m.push_rows(rows)
    ms.push_rows(rows)
    for offset in (0,) + cases.MISALIGNED_OFFSETS:
        buf, at = cases.misaligned_buffer(rows, offset)
        with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s, DeviceBuffer(buf.nbytes) as d:
            assert d.ptr % 16 == 0 and (d.ptr + at) % 16 == offset
            d.put(buf)
            h.push_rows(None, d.at(at, rows.nbytes), n_rows)
            s.push_rows(None, d.at(at, rows.nbytes), n_rows)
            v = _check_lines(h, m, what=f"offset {offset}")
            _check_lines(h, m, 129, what=f"offset {offset}")
            _check_ribbon(h, m, _x(n), what=f"offset {offset}")
            _check_surface(s, ms, what=f"offset {offset}")
            assert v["pushed"] == n_rows


# ---------------------------------------------------------------------------------------------------- maxima below zero
@pytest.mark.parametrize("n", cases.NEGATIVE_N)
def test_maxima_below_zero(n):
    """Catches: a key that orders negative floats by their bits (b instead of ~b), -inf rows reported as untouched
    slots, a zero whose sign decides, a tie between workgroups settled by their order instead of the bin."""
    named = cases.negative_rows(n)
    depth = len(named)
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for t in (h, m, s, ms):
            t.set_amplitude(*cases.NEGATIVE_AMPLITUDE)
        for name, row, at, _ in named:
            for t in (h, m, s, ms):
                t.push(row)
            v = _check_lines(h, m, first=0, count=1, what=name)
            w = _check_surface(s, ms, what=name)
            assert v["live_peak"][0] == at and w["live_peak"][0] == at, name
            assert _same(w["live_peak"][1], np.float32(row[at])), name
        for columns in (1, 7, n):
            _check_lines(h, m, columns)
            _check_surface(s, ms, columns)
            _check_ribbon(h, m, _x(n), columns)


# ---------------------------------------------------------------------------------------------------- cell widths
@pytest.mark.parametrize("n,columns", [(n, c) for n, by in cases.WIDTH_CASES.items() for c in by])
def test_cell_widths_next_to_the_group_thresholds(n, columns):
    """Catches: a group chosen from n / columns that misses the last bin of the cells one bin wider, a tie between the
    lanes of a group settled without the bin (oi < bi), lanes without a bin winning a cell of -inf, cells of a partly
    filled last workgroup."""
    rows, mn, plateaus, dead = cases.width_rows(n, columns)
    depth, last = cases.WIDTH_DEPTH, cases.WIDTH_ROWS - 1
    assert cases.reduce_group(n, columns) == cases.WIDTH_CASES[n][columns]
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for i, r in enumerate(rows):
            for t in (h, m):
                t.push(r, None, mn)
            for t in (s, ms):
                t.push(r)
            if i == 3:                             # lines 4 .. 6 were never pushed
                _check_lines(h, m, columns, what="four rows")
                _check_lines(h, m, columns, first=2, count=5, what="four rows")
                _check_lines(h, m, columns, first=5, count=2, what="four rows")
        _check_lines(h, m, columns)
        _check_lines(h, m, columns, first=1, count=3)
        _check_ribbon(h, m, _x(n), columns)
        v = _check_surface(s, ms, columns)
        cells = hc.cells(n, columns)
        for r, c, first, end in plateaus:
            if last - r < depth:
                assert v["bins"][last - r, c] == first, (r, c, first, end)
        assert v["bins"][last - dead[0], dead[1]] == cells[dead[1]][0] and v["z"][last - dead[0], dead[1]] == 0


# ---------------------------------------------------------------------------------------------------- arithmetic edges
@pytest.mark.parametrize("n", [54, 56])
def test_heights_on_and_next_to_integers(n):
    """Catches: int(8 - z) rounded instead of truncated, 8 - z or the clip evaluated in another precision."""
    row = cases.integer_edge_row(n)
    with TraceHistory(3, n) as h:
        m = hc.HistoryModel(3, n, "heights")
        for t in (h, m):
            t.set_amplitude(*cases.EXACT_AMPLITUDE)
            t.push(row)
            t.push(row[::-1])
        v = _check_lines(h, m)
        normal = (row == 0) | (np.abs(row) > 1e-30)                               # x / 8 * 8 == x unless x / 8 underflows
        assert _same(v["z"][1][normal], np.clip(row, np.float32(0), np.float32(8))[normal])   # z is the level itself
        _check_lines(h, m, 7)
        _check_ribbon(h, m, _x(n))


@pytest.mark.parametrize("n", [112, 113])
def test_ribbon_hues_on_sextant_boundaries(n):
    """Catches: a hue taken to float64 too early or too late, hue * 6 contracted or rounded, a sextant chosen by a
    comparison that differs from int() on the boundary."""
    row = cases.sextant_row(n)
    pairs = cases.sextant_pairs()
    assert len(pairs) == 7
    with TraceHistory(30, n) as h:
        m = hc.HistoryModel(30, n, "heights")
        for t in (h, m):
            t.set_amplitude(*cases.EXACT_AMPLITUDE)
            for _ in range(30):
                t.push(row)
        v = _check_ribbon(h, m, _x(n))
        assert _same(v["verts"][0, 0::2, 2], row)                                 # the heights are the levels themselves


@pytest.mark.parametrize("n", [24, 25])
def test_surface_levels_on_its_limits(n):
    """Catches: the normalisation in float32, a clip that lets a level one step outside through, inf - zmin or
    inf / span going to NaN."""
    rows = cases.surface_edge_rows(n)
    with TraceHistory(2, n, "levels") as s:
        ms = hc.HistoryModel(2, n, "levels")
        for r in (rows[0], rows[1], rows[0]):
            for t in (s, ms):
                t.push(r)
            for amp in cases.SURFACE_AMPLITUDES:
                for t in (s, ms):
                    t.set_amplitude(*amp)
                v = _check_surface(s, ms, what=f"{amp}")
                assert not np.isnan(v["z"]).any()
                _check_surface(s, ms, 5, what=f"{amp}")


# ---------------------------------------------------------------------------------------------------- NaN
def _with(row, j, value):
    row = np.array(row, dtype=np.float32)
    row[j] = value
    return row


@pytest.mark.parametrize("mode", ["live", "max", "min"])
def test_a_nan_bin_of_a_host_push_stays_where_it_is(mode):
    """history_contract's NaN paragraph: the device with a NaN at bin j against the contract with -inf there, everything
    compared but what the paragraph leaves open."""
    n, depth = cases.NAN_N, 5
    rows = cases.generic_rows(np.random.default_rng(9), 5, n)
    for j in cases.NAN_BINS:
        for columns in (None, 7):
            c = j if columns is None else cases.cell_of(n, columns, j)
            with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s:
                m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
                levels = (s, ms) if mode == "live" else ()

                def push(i, dirty):
                    mx = np.maximum.reduce(rows[:i + 1]) if mode == "max" else None
                    mn = np.minimum.reduce(rows[:i + 1]) if mode == "min" else None
                    for t, bad in ((h, np.nan), (m, -np.inf)):
                        live = _with(rows[i], j, bad) if dirty and mode == "live" else rows[i]
                        t.push(live, _with(mx, j, bad) if dirty and mode == "max" else mx,
                               _with(mn, j, bad) if dirty and mode == "min" else mn)
                    for t, bad in zip(levels, (np.nan, -np.inf)):
                        t.push(_with(rows[i], j, bad) if dirty else rows[i])

                def check(open_, what):
                    _check_lines(h, m, columns, what=what, open_=open_)
                    _check_ribbon(h, m, _x(n), columns, what=what, open_=open_)
                    if levels:
                        _check_surface(s, ms, columns, what=what, open_=open_)

                push(0, False)
                push(1, False)
                push(2, True)
                what = f"{mode} j={j}"
                if mode == "live":
                    check(Open(cells=[(0, c)], hold=[c], live_peak=True, hold_peak=True), what + " dirty")
                elif mode == "max":
                    check(Open(hold=[c], hold_peak=True), what + " dirty")
                else:
                    check(Open(min=[c]), what + " dirty")
                push(3, False)                     # the live peak is the contract's again
                if mode == "live":
                    check(Open(cells=[(1, c)], hold=[c], hold_peak=True), what + " then clean")
                elif mode == "max":
                    check(Open(hold=[c], hold_peak=True), what + " then clean")
                else:
                    check(NOTHING, what + " then clean")
                for t in (h, m):
                    t.reset_hold()
                push(4, False)                     # and so is the hold
                check(Open(cells=[(2, c)]) if mode == "live" else NOTHING, what + " after reset_hold")


def test_nan_bins_of_a_chunked_batch_stay_where_they_are():
    n, n_rows, depth = cases.NAN_CHUNK
    case = cases.chunk_case(n, n_rows, depth)
    assert case["geometry"][2] >= 2
    j = (496, 498, n - 1)
    at = [(100, j[0]), (n_rows - 10, j[1]), (n_rows - 1, j[2])]          # a skipped row, a line, the newest line
    assert at[0][0] < case["skip"] <= at[1][0]
    dirty, clean = case["batch"].copy(), case["batch"].copy()
    for k, b in at:
        dirty[k, b], clean[k, b] = np.nan, -np.inf
    extra = cases.generic_rows(np.random.default_rng(3), 2, n)
    with TraceHistory(depth, n) as h, TraceHistory(depth, n, "levels") as s, DeviceBuffer(dirty.nbytes) as d:
        m, ms = hc.HistoryModel(depth, n, "heights"), hc.HistoryModel(depth, n, "levels")
        for t in (h, m, s, ms):
            t.set_amplitude(*cases.CHUNK_AMPLITUDE)
            t.push(case["first"])
        d.put(dirty)
        h.push_rows(None, d.ptr, n_rows)
        s.push_rows(None, d.ptr, n_rows)
        m.push_rows(clean)
        ms.push_rows(clean)
        for step in range(3):
            for columns in (None, 7):
                c = [b if columns is None else cases.cell_of(n, columns, b) for b in j]
                open_ = Open(cells=[(step + 9, c[1]), (step, c[2])], hold=c if step < 2 else (), live_peak=step == 0,
                             hold_peak=step < 2)
                _check_lines(h, m, columns, what=f"step {step}", open_=open_)
                _check_ribbon(h, m, _x(n), columns, what=f"step {step}", open_=open_)
                _check_surface(s, ms, columns, what=f"step {step}", open_=open_)
            if step == 1:
                for t in (h, m):
                    t.reset_hold()
            if step < 2:
                for t in (h, m, s, ms):
                    t.push(extra[step])
