"""The contract of the two peak searches of tdsa_analytics.hip (top_peaks_kernel, marker_peaks_kernel) and the rows that
pin them.  TEST INFRASTRUCTURE ONLY.

Top peaks: oracle.analytics_oracle.find_top_peaks with the candidate order made deterministic (a stable sort walked
backwards: between equal values the larger index first, the device's documented rule) and the excursion taken as the
float32 value the C-ABI receives.  A NaN between two peaks makes the reference's np.min NaN and both of its comparisons
false: such a valley never rejects.

Markers: oracle.analytics_oracle.marker_find_peaks / snap_to_peak_bin / snap_to_next_peak_bin as they are (scipy's
find_peaks(height, prominence, distance) restated; tests/test_peaks_host.py holds the rows against the real scipy).

Every builder returns cases = dicts with the rows [R][n] float32, the call's parameters and the contract's answer; with
check=True it also asserts that its rows discriminate (the notch changes the answer, the decoy does not but would with a
valley one block wider, the two sides of a threshold differ ...).  Everything is compared bit for bit."""
import functools
import itertools

import numpy as np

from oracle import analytics_oracle as ao

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
MAX_N = 16384
LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4097, 8193, 16383, 16384)
LANES = (0, 1, 15, 30, 31)                       # `& 31` of the bins the top-peaks families put their peaks at


def top_threads(n):
    """threads per row of top_peaks_kernel (launch_top_peaks)"""
    return 64 if n <= 1024 else 128 if n <= 2048 else 256 if n <= 4096 else 512 if n <= 8192 else 1024


# The first length that selects each width (for 64 threads the first that holds the families: 13 whole blocks and a ragged
# one) and the last: 16 bins per thread, so only there do blocks of 32 bins reach the upper half of the waves.
TOP_FIRST = (417, 1025, 2049, 4097, 8193)
TOP_LAST = (1024, 2048, 4096, 8192, 16384)


def up(x, k=1):
    """x moved by k float32 steps (k < 0: down)"""
    x = F32(x)
    with np.errstate(all="ignore"):
        for _ in range(abs(int(k))):
            x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return x


# ---- top peaks -------------------------------------------------------------------------------------------------------
def top_peaks(row, n_peaks, min_sep, exc):
    """Bins of the contract, strongest first."""
    row = np.asarray(row, dtype=F32)
    with np.errstate(all="ignore"):
        got = ao.find_top_peaks(np.arange(len(row), dtype=np.float64), row, int(n_peaks), int(min_sep),
                                float(F32(exc)), kind="stable")
    return [int(f) for f, _ in got]


def top_peaks_variant(row, n_peaks, min_sep, exc, wide=False, small_first=False):
    """The same selection restated, with the two mistakes the families are built against: a valley taken a block of 32
    bins wider than the span on both sides (wide), equal candidates visited smaller index first (small_first)."""
    row = np.asarray(row, dtype=F32)
    e, n = float(F32(exc)), len(row)
    if n < 3:
        return []
    mid = row[1:-1]
    cands = np.flatnonzero((mid > row[:-2]) & (mid > row[2:])) + 1
    order = cands[np.argsort(row[cands], kind="stable")[::-1]]
    if small_first:
        order = cands[np.argsort(-row[cands], kind="stable")]
    chosen = []
    with np.errstate(all="ignore"):
        for c in order:
            if len(chosen) >= n_peaks:
                break
            ok = True
            for o in chosen:
                if abs(int(c) - o) < min_sep:
                    ok = False
                    break
                a, b = min(int(c), o), max(int(c), o)
                if wide:
                    a, b = max(0, (a & ~31) - 32), min(n - 1, (b | 31) + 32)
                floor = float(row[a:b + 1].min())
                if row[c] - floor < e or float(row[o]) - floor < e:
                    ok = False
                    break
            if ok:
                chosen.append(int(c))
    return chosen


def top_expected(rows, n_peaks, min_sep, exc):
    """(bins [R][n_peaks] int32 padded with -1, dB [R][n_peaks] float32 padded with NaN) of the contract."""
    rows = np.asarray(rows, dtype=F32)
    bins = np.full((len(rows), n_peaks), -1, dtype=np.int32)
    db = np.full((len(rows), n_peaks), np.nan, dtype=F32)
    for r, row in enumerate(rows):
        got = top_peaks(row, n_peaks, min_sep, exc)
        bins[r, :len(got)] = got
        db[r, :len(got)] = row[got]
    return bins, db


def _top_case(name, rows, n_peaks, min_sep, exc, **extra):
    rows = np.ascontiguousarray(np.stack(rows), dtype=F32)
    assert rows.shape[1] <= MAX_N
    # the separation as the contract sees it: none below 1 (tdsa_hip.h)
    bins, db = top_expected(rows, n_peaks, min_sep, exc)
    return dict(name=name, rows=rows, n=rows.shape[1], n_peaks=n_peaks, min_sep=min_sep, exc=exc, bins=bins, db=db, **extra)


def _found(case, r):
    return [int(b) for b in case["bins"][r] if b >= 0]


def _interior_pick(a, b):
    ia, ib = (a >> 5) + 1, (b >> 5) - 1
    if ia > ib:
        return []
    blocks = {ia, ib, (ia + ib) // 2} | {k for k in (63, 64, 127, 128, 255, 256, 383, 384) if ia <= k <= ib}
    return [32 * k + lane for k in sorted(blocks) for lane in (0, 13, 31)]


def _pairs(n):
    """(placement, a, b): two peaks in one block of 32 bins, in adjacent blocks, many blocks apart."""
    combos = [(LANES[i], LANES[(i + s) % 5]) for s in (0, 2) for i in range(5)]
    out = [("same", 96 + la, 96 + lb) for la, lb in ((0, 15), (1, 30), (15, 31), (0, 31), (1, 15), (15, 30), (0, 2))]
    out += [("adjacent", 96 + la, 128 + lb) for la, lb in combos + [(31, 1), (30, 0), (31, 15)]]
    out += [("far", 32 + la, 32 * (n // 32 - 2) + lb) for la, lb in combos]
    return out


def top_valley_cases(n, check=False):
    """Two strong peaks a < b over a floor that is too shallow; ONE deep notch somewhere in the span makes the valley
    pass, the same notch just outside the span must not."""
    hi, lo, floor, notch = F32(0.0), F32(-1.0), F32(-5.0), F32(-50.0)
    rows, meta = [], []
    for placement, a, b in _pairs(n):
        for mirror in (0, 1):                              # 0: the accepted (stronger) peak on the left, 1: on the right
            base = np.full(n, floor, dtype=F32)
            base[a], base[b] = (lo, hi) if mirror else (hi, lo)
            i0 = len(rows)
            rows.append(base)
            meta.append(("none", placement, a, b, -1, i0))
            inside = {a + 1, min(b - 1, a | 31), min(b - 1, max(a + 1, b & ~31)), b - 1} | set(_interior_pick(a, b))
            if placement == "same":
                inside |= set(range(a + 1, b))
            inside = {q for q in inside if a < q < b}              # (a peak in lane 31 / lane 0 has no bin of its block on that side)
            outside = {a - 1, a & ~31, b + 1, min(n - 1, b | 31)} - {a, b}
            for kind, where in (("notch", inside), ("decoy", outside)):
                for pos in sorted(where):
                    row = base.copy()
                    row[pos] = notch
                    rows.append(row)
                    meta.append((kind, placement, a, b, pos, i0))
    case = _top_case(f"valley n={n}", rows, 5, 2, 10.0, meta=meta)
    if check:
        regions = set()
        for r, (kind, placement, a, b, pos, i0) in enumerate(meta):
            got, plain = _found(case, r), _found(case, i0)
            strong = b if case["rows"][r][b] > case["rows"][r][a] else a
            assert plain == [strong], (n, meta[r])
            if kind == "notch":
                assert a < pos < b and got == [strong, a + b - strong], (n, meta[r], got)
                region = "between" if placement == "same" else ("a" if pos >> 5 == a >> 5 else "b" if pos >> 5 == b >> 5 else "in")
                regions.add((placement, region))
            elif kind == "decoy":
                assert (pos < a or pos > b) and got == plain, (n, meta[r], got)
                assert top_peaks_variant(case["rows"][r], 5, 2, 10.0, wide=True) == [strong, a + b - strong], (n, meta[r])
            assert top_peaks_variant(case["rows"][r], 5, 2, 10.0) == got
        assert regions == {("same", "between"), ("adjacent", "a"), ("adjacent", "b"), ("far", "a"), ("far", "b"), ("far", "in")}
        assert {m[2] & 31 for m in meta} == set(LANES) and {m[3] & 31 for m in meta} >= set(LANES)
    return [case]


def top_many_cases(n, check=False):
    """One to seven accepted peaks and a weaker candidate next to the accepted peak of rank k (the k-th accepted), for
    every k: every other valley of the candidate holds a deep notch, the one against rank k only with `opt`.  Then
    twelve qualifying candidates for n_peaks = 1 ... 8."""
    floor, notch, cand = F32(-8.0), F32(-60.0), F32(-4.5)
    rows, meta = [], []
    centre = (n // 2) & ~31
    for gap, dc, dn, dopt, start in ((6, 2, 4, 1, centre - 63), (40, 13, 26, 6, centre - 151)):
        for K in range(1, 8):
            pos = [start + gap * j for j in range(K)]
            for perm in ([j for j in range(K)], [K - 1 - j for j in range(K)], [(3 * j + 1) % K for j in range(K)] if K in (4, 5, 7) else None):
                if perm is None:
                    continue
                for k, side, opt in itertools.product(range(K), (1, -1), (False, True)):
                    row = np.full(n, floor, dtype=F32)
                    for j, p in enumerate(pos):
                        row[p] = F32(-0.5 * perm[j])
                        row[p + gap // 2] = notch
                    row[start - gap // 2] = notch
                    j = perm.index(k)
                    p = pos[j]
                    row[p + side * (gap // 2)] = floor
                    c = p + side * dc
                    row[c] = cand
                    row[p + side * dn] = notch
                    if opt:
                        row[p + side * dopt] = notch
                    rows.append(row)
                    meta.append((K, tuple(pos), tuple(perm), k, c, opt))
    case = _top_case(f"many n={n}", rows, 8, 2, 6.0, meta=meta)
    cases = [case]
    if check:
        for r, (K, pos, perm, k, c, opt) in enumerate(meta):
            got, row = _found(case, r), case["rows"][r]
            accepted = [pos[perm.index(q)] for q in range(K)]
            assert got == accepted + ([c] if opt else []), (n, meta[r], got)
            shallow = [q for q in range(K) if row[min(c, accepted[q]):max(c, accepted[q]) + 1].min() > notch]
            assert shallow == ([] if opt else [k]), (n, meta[r], shallow)
    # more qualifying candidates than any n_peaks: 12 peaks, a notch between neighbours
    rows = []
    for levels in ([-0.25 * j for j in range(12)], [-0.25 * (11 - j) for j in range(12)], [-0.25 * ((5 * j + 3) % 12) for j in range(12)]):
        for gap, start in ((6, centre - 40), (33, max(5, centre - 200))):
            row = np.full(n, floor, dtype=F32)
            for j, lv in enumerate(levels):
                row[start + gap * j] = F32(lv)
                row[start + gap * j + gap // 2] = notch
            rows.append(row)
    for n_peaks in range(1, 9):
        cs = _top_case(f"twelve candidates n={n} n_peaks={n_peaks}", rows, n_peaks, 2, 6.0)
        if check:
            assert all(len(_found(cs, r)) == n_peaks for r in range(len(rows)))
            assert all(len(top_peaks(row, 12, 2, 6.0)) == 12 for row in rows)
        cases.append(cs)
    return cases


EXCURSIONS = (3.0, 6.0, 10.0, 0.0, 6.3, 0.7)


def top_threshold_cases(n, check=False):
    """A row that is ONE level `valley` but for two peaks: the candidate's float32 difference and the accepted peak's
    float64 difference sit on, one float32 step above and below the excursion, and on opposite sides of it."""
    cases, classes = [], set()
    a, b = 40, 75
    for exc in EXCURSIONS:
        e32 = F32(exc)
        rows, meta = [], []
        for valley in (F32(0.0), F32(-73.3), F32(-0.1), F32(1.5e-7), F32(-100.7), F32(33.3), F32(-299.9)):
            centre = F32(valley + e32)
            for k in range(-3, 4):
                vc = up(centre, k) if exc > 0 else up(valley, k + 4)
                if not vc > valley:
                    continue
                for tie, mirror in ((True, 0), (False, 0), (False, 1)):
                    vs = vc if tie else F32(vc + F32(50.0))
                    row = np.full(n, valley, dtype=F32)
                    # equal peaks: the larger index is visited (and accepted) first, the candidate is the one at a
                    row[a], row[b] = (vs, vc) if mirror else (vc, vs)
                    rows.append(row)
                    with np.errstate(all="ignore"):
                        meta.append((valley, k, tie, mirror, bool(F32(vc - valley) < e32),
                                     bool(float(vs) - float(valley) < float(e32)), bool(float(vc) - float(valley) < float(e32))))
        case = _top_case(f"threshold exc={exc} n={n}", rows, 5, 2, exc, meta=meta)
        if check:
            for r, (valley, k, tie, mirror, rej32, rej64, own64) in enumerate(meta):
                assert len(_found(case, r)) == (1 if rej32 or rej64 else 2), (exc, meta[r])
                classes.add((rej32, rej64, tie, own64))
            if exc > 0:
                on = [m for m in meta if m[0] == 0.0 and m[2]]
                assert [(m[1], m[4] or m[5]) for m in on if abs(m[1]) <= 1] == [(-1, True), (0, False), (1, False)], exc
            else:
                assert not any(m[4] or m[5] for m in meta)
        cases.append(case)
    if check:
        # opposite sides: the float32 difference passes (rounded up onto the excursion) where the float64 difference of the SAME
        # numbers fails - only the accepted peak's comparison turns the candidate down; the reverse cannot happen with equal
        # numbers (rounding is monotone and the excursion is a float32), only with a stronger accepted peak
        assert any(not r32 and r64 and tie for r32, r64, tie, own in classes)
        assert any(r32 and not r64 and not tie for r32, r64, tie, own in classes)
        assert not any(r32 and not own for r32, r64, tie, own in classes)
    return cases


def excursion_63_row(n=417):
    """The constructed 6.3 case: two equal peaks float32(6.3) over a floor of 1.5e-7.  The float64 difference lies
    between 6.3 and float32(6.3): the contract (the excursion IS a float32) turns the second peak down, the unrounded
    Python float would let it in."""
    row = np.full(n, F32(1.5e-7), dtype=F32)
    row[40] = row[75] = F32(6.3)
    return row


def top_separation_cases(n, check=False):
    """An accepted peak at p, candidates exactly min_sep - 1 and min_sep away on both sides; min_sep on both sides of
    the `2 min_sep - 1 <= threads` switch, beyond the row, below 1 (= no rule), and wider than a thread's stride."""
    T = top_threads(n)
    floor = F32(-100.0)
    cases = []
    spots = sorted({p for p in (T, T + 1, 2 * T - 1, T + T // 2, n // 2, n - T - 3) if T // 2 + 3 <= p <= n - T // 2 - 4})
    for ms in (1, 2, T // 2, T // 2 + 1, n, n + 5, 2 ** 31 - 1, 0, -3):
        rows, meta = [], []
        near = (2, 3) if ms <= 3 else (ms - 1, ms) if ms < n else (0,)
        for p in spots:
            for dl, dr, swap in itertools.product(near, near, (0, 1)):
                row = np.full(n, floor, dtype=F32)
                row[p] = F32(0.0)
                l, r = (p - dl, p + dr) if ms < n else (1, n - 2)
                if not (1 <= l < p - 1 and p + 1 < r <= n - 2):
                    continue
                row[l], row[r] = (F32(-2.0), F32(-3.0)) if swap else (F32(-3.0), F32(-2.0))
                rows.append(row)
                meta.append((p, l, r))
        if not rows:
            continue
        case = _top_case(f"separation min_sep={ms} n={n}", rows, 5, ms, 6.0, meta=meta)
        if check:
            for r, (p, l, rr) in enumerate(meta):
                keep = [q for q in (l, rr) if abs(q - p) >= ms]
                got = _found(case, r)
                assert got[0] == p and sorted(got[1:]) == sorted(keep), (ms, meta[r], got)   # (two kept ones are 2 min_sep apart)
            if 3 < ms < n:
                assert {len(_found(case, r)) for r in range(len(rows))} >= {1, 2}
        cases.append(case)
    # wider than the stride: the accepted peak sweeps away two candidates of ONE thread (p + T, p + 2T), keeps the one exactly
    # min_sep away and the thread's next
    if n >= 4 * T + 16:
        for ms in (2 * T, 2 * T + 3):
            rows = []
            for p in (T + 5, T + 63, 2 * T - 1):
                row = np.full(n, floor, dtype=F32)
                row[p] = F32(0.0)
                for q, lv in ((p + T, -1.0), (p + 2 * T, -2.0), (p + ms, -3.0), (p + 3 * T, -4.0), (p - T, -5.0), (p + ms - 1, -6.0)):
                    if row[q - 1] == floor and row[q + 1] == floor:
                        row[q] = F32(lv)
                rows.append(row)
            case = _top_case(f"sweep min_sep={ms} n={n}", rows, 8, ms, 6.0)
            if check:
                for r, p in enumerate((T + 5, T + 63, 2 * T - 1)):
                    assert _found(case, r) == [p, p + ms], (ms, _found(case, r))   # p + 3T is within min_sep of p + ms
                    assert len(top_peaks(case["rows"][r], 8, 2, 6.0)) >= 5
            cases.append(case)
    return cases


def top_tie_cases(n, check=False):
    """Equal candidates in one thread, one row of 16 lanes, one wave, two waves: larger index first, also where that
    decides which of two conflicting peaks stays."""
    T = top_threads(n)
    floor, v = F32(-100.0), F32(-10.0)
    s = T + 3
    groups = {"thread": (s, s + T), "lanes": (s, s + 5), "rows16": (s, s + 20), "wave": (s, s + 40),
              "all": (s, s + 5, s + 20, s + 40, s + T, s + 2 * T + 7)}
    if T >= 128:
        groups["waves"] = (s, s + 70)
        groups["all"] += (s + 70,)
    cases = []

    def rows_of(between=None):
        out = []
        for name, pos in groups.items():
            row = np.full(n, floor, dtype=F32)
            if between is not None:
                row[min(pos):max(pos) + 1] = between
            row[list(pos)] = v
            out.append(row)
        return out
    for n_peaks, ms in ((1, 1), (2, 1), (8, 1), (8, 6), (8, 21), (8, T + 1)):
        case = _top_case(f"ties n={n} n_peaks={n_peaks} min_sep={ms}", rows_of(), n_peaks, ms, 6.0)
        if check:
            for r, pos in enumerate(groups.values()):
                got = _found(case, r)
                assert got[0] == max(pos) and got == sorted(got, reverse=True), (n, ms, got)
                other = top_peaks_variant(case["rows"][r], n_peaks, ms, 6.0, small_first=True)
                assert other != got, (n, ms, got)
        cases.append(case)
    case = _top_case(f"ties n={n} shallow valley", rows_of(F32(-11.0)), 8, 1, 6.0)
    if check:
        for r, pos in enumerate(groups.values()):
            assert _found(case, r) == [max(pos)]
            assert top_peaks_variant(case["rows"][r], 8, 1, 6.0, small_first=True) == [min(pos)]
    cases.append(case)
    return cases


def top_nonfinite_cases(n, check=False):
    """NaN at and next to a candidate, in every region of a valley (never rejects) and just outside it (no effect),
    -inf valleys, +inf peaks, rows without any candidate.

    No row forms inf - inf, and none can: a candidate is a STRICT maximum, so the valley of a +inf peak holds a bin below
    +inf and its floor is finite or -inf (inf - finite, inf - (-inf) = +inf: never below an excursion); a peak is never
    -inf.  What +inf can do is here: a +inf peak against a finite one on either side, two +inf peaks (a tie: larger index
    first), +inf over a -inf floor, and the all-+inf / all--inf rows, which have no candidate."""
    hi, lo, floor = F32(0.0), F32(-1.0), F32(-5.0)
    rows, meta = [], []
    picks = [("same", 96 + 1, 96 + 30), ("same", 96 + 0, 96 + 4), ("adjacent", 96 + 15, 128 + 15), ("adjacent", 96 + 28, 128 + 3),
             ("far", 32 + 1, 32 * (n // 32 - 2) + 30), ("far", 32 + 15, 32 * (n // 32 - 2) + 0 + 3)]
    for placement, a, b in picks:
        for mirror, (pa, pb) in enumerate(((hi, lo), (lo, hi), (INF, lo), (lo, INF), (INF, INF))):
            base = np.full(n, floor, dtype=F32)
            base[a], base[b] = pa, pb
            i0 = len(rows)
            rows.append(base)
            meta.append(("none", a, b, -1, i0))
            inside = {a + 2, min(b - 2, a | 31), max(a + 2, b & ~31), b - 2} | set(_interior_pick(a, b))
            inside = {q for q in inside if a + 2 <= q <= b - 2}
            for kind, where, value in (("nan", inside, NAN), ("ninf", inside | {a + 1, b - 1}, -INF),
                                       ("decoy", {a - 2, (a & ~31) - 1, b + 2, b + 33}, NAN), ("decoy", {a - 1, b + 1}, -INF),
                                       ("kill", {a - 1, a, a + 1, b - 1, b, b + 1}, NAN)):
                for pos in sorted(where):
                    if kind == "decoy" and value != value and (abs(pos - a) <= 1 or abs(pos - b) <= 1):
                        continue                              # (a NaN next to a peak takes the peak away: that is `kill`)
                    row = base.copy()
                    row[pos] = value
                    rows.append(row)
                    meta.append((kind, a, b, pos, i0))
    ramp = np.arange(n, dtype=F32)
    for row in (np.full(n, NAN), np.full(n, F32(-3.0)), ramp, -ramp, np.where(np.arange(n) % 7 == 3, NAN, F32(1.0)),
                np.full(n, INF), np.full(n, -INF)):
        rows.append(np.asarray(row, dtype=F32))
        meta.append(("empty", 0, 0, -1, len(rows) - 1))
    case = _top_case(f"non-finite n={n}", rows, 5, 2, 10.0, meta=meta)
    if check:
        for r, (kind, a, b, pos, i0) in enumerate(meta):
            got, plain, row = _found(case, r), _found(case, i0), case["rows"][r]
            if kind == "empty":
                assert got == []
            elif kind in ("nan", "ninf"):
                assert sorted(got) == [a, b], (n, meta[r], got)
            elif kind == "decoy":
                assert got == plain, (n, meta[r], got)
            elif kind == "kill":
                gone = a if abs(pos - a) <= 1 else b
                assert got == [a + b - gone], (n, meta[r], got)
            elif np.isinf(row[a]) and np.isinf(row[b]):
                assert got == [b, a]                     # +inf - floor is below no excursion; equal: the larger index first
            else:
                assert len(got) == 1                      # the floor alone is too shallow
    return [case]


def top_length_cases(n, check=False):
    """Every row of a batch different: a peak at bin 1, one at bin n - 2, a third that moves with the row."""
    cases = []
    for count in (1, 2, 257):
        rows = []
        for r in range(count):
            row = np.full(n, F32(-100.0 - 0.5 * r), dtype=F32)
            if n >= 3:
                row[1] = F32(-0.25 * r)
                row[n - 2] = F32(-10.0 - 0.125 * r)
                q = 3 + (7 * r) % max(n - 6, 1)
                if 3 <= q <= n - 4:
                    row[q] = F32(-20.0 + 0.0625 * r)
            rows.append(row)
        case = _top_case(f"lengths n={n} rows={count}", rows, 5, 2, 6.0)
        if check:
            for r in range(count):
                got = _found(case, r)
                if n >= 5:
                    assert 1 in got and n - 2 in got, (n, r, got)
                elif n == 3:
                    assert got == [1]
                elif n < 3:
                    assert got == []
            assert len({row.tobytes() for row in case["rows"]}) == count
            if count > 1 and n >= 9:
                assert len({tuple(b) for b in case["bins"]}) > 1
        cases.append(case)
    return cases


def all_top_cases(check=False):
    out = []
    for n in TOP_FIRST + TOP_LAST:
        out += top_valley_cases(n, check)
    for n in TOP_FIRST + (16384,):
        out += top_many_cases(n, check) + top_nonfinite_cases(n, check)
    for n in TOP_FIRST + TOP_LAST:
        out += top_separation_cases(n, check) + top_tie_cases(n, check)
    for n in TOP_FIRST + TOP_LAST:
        out += top_threshold_cases(n, check)
    for n in LENGTHS:
        out += top_length_cases(n, check)
    return out


# ---- markers ---------------------------------------------------------------------------------------------------------
DEFAULTS = dict(height=-200.0, prominence=6.0, distance=3, current_idx=-1, max_list=8)


def marker_expected(rows, height, prominence, distance, current_idx, max_list):
    """What tdsa_rows_marker_peaks reports, from the oracle's three functions as they are."""
    rows = np.asarray(rows, dtype=F32)
    R = len(rows)
    out = dict(n_peaks=np.zeros(R, np.int32), snap_bin=np.zeros(R, np.int32), next_bin=np.zeros(R, np.int32),
               peaks=np.full((R, max_list), -1, np.int32), prominences=np.full((R, max_list), np.nan, np.float64))
    # The two snap functions call marker_find_peaks again with the row's same arguments; its Python walk over a long row is
    # what a batch costs, so one row's search is done once and handed to all three (the functions themselves are untouched).
    search, memo = ao.marker_find_peaks, {}

    def once(levels, *args):
        key = (id(levels),) + args
        if key not in memo:
            memo.clear()
            memo[key] = search(levels, *args)
        return memo[key]
    ao.marker_find_peaks = once
    try:
        with np.errstate(all="ignore"):
            for r, row in enumerate(rows):
                memo.clear()                               # (a row's id may be the last row's)
                pk, _, prom = ao.marker_find_peaks(row, height, prominence, distance)
                out["n_peaks"][r] = len(pk)
                out["snap_bin"][r] = ao.snap_to_peak_bin(row, height, prominence, distance)
                out["next_bin"][r] = ao.snap_to_next_peak_bin(row, current_idx, height, prominence, distance)
                m = min(len(pk), max_list)
                out["peaks"][r, :m] = pk[:m]
                out["prominences"][r, :m] = prom[:m]
    finally:
        ao.marker_find_peaks = search
    return out


def close_ties(row, height, distance):
    """Two equal-height peaks within `distance` of each other: scipy's order between them is not defined."""
    x = np.asarray(row, dtype=np.float64)
    # every peak, flat or not, starts with a rising edge onto its own value: no two equal values among those, no tie
    # (decided without the oracle's Python walk, which is most of a long row's cost)
    rising = x[1:][x[1:] > x[:-1]]
    if len(np.unique(rising)) == len(rising):
        return False
    pk = ao._local_maxima(x)
    pk = pk[x[pk] >= height]
    d = int(np.ceil(distance))
    for i in range(len(pk)):
        j = i + 1
        while j < len(pk) and pk[j] - pk[i] < d:
            if x[pk[j]] == x[pk[i]]:
                return True
            j += 1
    return False


def _mark_case(name, rows, tie_family=False, want=None, meta=None, **params):
    rows = np.ascontiguousarray(np.stack(rows), dtype=F32)
    assert rows.shape[1] <= MAX_N
    kw = dict(DEFAULTS, **params)
    ties = np.array([close_ties(row, kw["height"], kw["distance"]) for row in rows]) if want is None else np.zeros(len(rows), bool)
    assert tie_family or not ties.any(), name
    return dict(name=name, rows=rows, n=rows.shape[1], params=kw, ties=ties, meta=meta,
                want=marker_expected(rows, **kw) if want is None else want)


def _peaks_of(case, r):
    return [int(b) for b in case["want"]["peaks"][r] if b >= 0]


FLAT_WIDTHS = (2, 3, 31, 32, 33, 64, 65, 1025)


def marker_flat_cases(check=False):
    """Flat tops of every width over the seams of the blocks of 32 bins: the peak is the middle (left + right) // 2."""
    floor, top = F32(-100.0), F32(-20.0)
    cases = []
    for n in (1300, 1301):                                 # n % 4 == 0: the 16-byte loads; else one float per lane
        rows, meta = [], []
        for W in FLAT_WIDTHS:
            starts = {0, 1, 31, 32, 33} | {s for s in range(64, 96) if (s + W) % 32 in (0, 1, 31)}
            for s in sorted(starts):
                for tail in ("fall", "rise", "nan", "inf", "infnan"):
                    row = np.full(n, floor, dtype=F32)
                    row[s:s + W] = INF if tail.startswith("inf") else top
                    if tail == "rise":
                        row[s + W] = F32(-10.0)
                    if tail in ("nan", "infnan"):
                        if W < 3:
                            continue
                        row[s + W // 2 if W < 96 else 96 + 32 * 3 + 7] = NAN   # (the widest: inside a block the plateau fills)
                    rows.append(row)
                    meta.append((W, s, tail))
        for s in (n - 1, n - 2, n - 33, n - 64, n - 1026):   # a plateau that reaches the last bin is no peak
            row = np.full(n, floor, dtype=F32)
            row[s:] = top
            rows.append(row)
            meta.append((n - s, s, "end"))
        case = _mark_case(f"flat tops n={n}", rows, meta=meta)
        if check:
            for r, (W, s, tail) in enumerate(meta):
                want = [] if tail in ("nan", "infnan", "end") or (s == 0 and tail != "rise") else [s + W] if tail == "rise" else [(2 * s + W - 1) // 2]
                assert _peaks_of(case, r) == want, (n, meta[r], _peaks_of(case, r))
            whole = [(W, s) for W, s, t in meta if s % 32 == 0 and W % 32 == 0]
            assert whole and {(s % 32, (s + W) % 32) for W, s, t in meta} >= {(0, 0), (31, 1), (1, 0), (0, 31)}
        cases.append(case)
    return cases


def marker_height_cases(check=False):
    """Peaks exactly at `height`, one float32 step below and above, a +inf peak; heights of +-inf."""
    v = F32(-20.3)
    cases, counts = [], []
    for n in (64, 65):
        row = np.full(n, F32(-100.0), dtype=F32)
        row[[5, 15, 25, 35, 45]] = [v, up(v, -1), up(v, 1), INF, F32(-90.0)]
        for height in (float(v), float(np.nextafter(np.float64(v), np.inf)), float(up(v, -1)), -np.inf, np.inf, -90.0):
            case = _mark_case(f"height {height!r} n={n}", [row, row[::-1].copy()], height=height)
            counts.append(int(case["want"]["n_peaks"][0]))
            cases.append(case)
    if check:
        assert counts[:6] == [3, 2, 4, 5, 1, 5], counts
    return cases


DISTANCES = (1, 2, 3, 4, 32, 33, 34, 64, 1000)


def _chains(n, gaps, starts=(33, 62, 63, 64)):
    patterns = ((0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0), (1, 3, 2, 4, 3, 5), (3, 1, 4, 0, 5, 2), (2, 2, 2, 2, 2, 2), (1, 2, 2, 1, 2, 2), (0, 1))
    rows = []
    for g, s0, pat in itertools.product(gaps, starts, patterns):
        if s0 + g * (len(pat) - 1) > n - 2:
            continue
        row = np.full(n, F32(-100.0), dtype=F32)
        for j, h in enumerate(pat):
            row[s0 + g * j] = F32(-20.0 + h)
        rows.append(row)
    return rows


def marker_distance_cases(check=False):
    """Chains of peaks exactly distance - 1 and distance apart (rising, falling, equal, mixed heights) across the 32-bit
    words of the bit set, on both sides of the `reach < 32` pre-pass; distances beyond the row."""
    cases = []
    for D in DISTANCES:
        for n in ((5120, 5121) if D == 1000 else (512, 513)):
            gaps = (2, 3) if D <= 3 else (D - 1, D)
            case = _mark_case(f"distance {D} n={n}", _chains(n, gaps, (63, 64) if D == 1000 else (33, 62, 63, 64)), tie_family=True,
                              distance=D, max_list=8)
            if check:
                kept = {int(c) for c in case["want"]["n_peaks"]}
                assert kept >= ({6} if D <= 2 else {3, 6}), (D, kept)        # a gap of distance - 1 halves the chain
                assert case["ties"].any() == (D > 2)
            cases.append(case)
    for n in (300, 301):
        for D in (n, n + 7, 2 ** 31 - 1):
            case = _mark_case(f"distance {D} n={n}", _chains(n, (2, 3, 40)), tie_family=True, distance=D, max_list=8)
            if check:
                assert set(case["want"]["n_peaks"]) == {1}
            cases.append(case)
    return cases


def marker_staircase_case(n, mirror=False):
    """[0, 1, 0, 2, 0, 3, ...] with distance 3: from the top down every other peak goes - the fixed point settles one peak
    per round, thousands of rounds at 16384 bins.  The expected answer is the closed form (the oracle's Python walk of
    every prominence is quadratic here); tests/test_peaks_host.py holds it against scipy at full length and against the
    oracle at 1024 bins."""
    x = np.zeros(n, dtype=F32)
    odd = np.arange(1, n, 2)
    x[odd] = (odd + 1) // 2
    peaks = odd[odd <= n - 2]
    kept = peaks[::-1][::2][::-1]                          # the highest, then every second one below it
    if mirror:
        x = x[::-1].copy()
        kept = (n - 1 - kept)[::-1]
    prom = x[kept].astype(np.float64)                      # both bases are 0
    params = dict(DEFAULTS, prominence=0.5, current_idx=n // 2, max_list=len(kept) + 4)
    right = kept[kept > params["current_idx"]]
    want = dict(n_peaks=np.array([len(kept)], np.int32), snap_bin=np.array([kept[np.argmax(x[kept])]], np.int32),
                next_bin=np.array([right[0] if len(right) else kept[0]], np.int32),
                peaks=np.full((1, params["max_list"]), -1, np.int32), prominences=np.full((1, params["max_list"]), np.nan))
    want["peaks"][0, :len(kept)] = kept
    want["prominences"][0, :len(kept)] = prom
    return _mark_case(f"staircase n={n} mirror={mirror}", [x], want=want, **params)


WALK_N = (2600, 2601, 3072)                                # ragged last blocks of 32 and of 1024 bins, and whole ones


def marker_walk_cases(check=False):
    """One peak (-20) whose higher base (-30) lies on the tested side: within the first six bins, at the seventh, in a
    skipped block of 32 / of 1024, behind a sample equal to the peak, NOT behind a sample one step above it, at the last bin
    of the row, before a NaN.  Every row has the prominence 10.0 exactly: the filter runs on it and one float64 step either
    side."""
    xp, fill, base, other, wall, decoy = F32(-20.0), F32(-22.0), F32(-30.0), F32(-40.0), F32(-10.0), F32(-90.0)
    cases = []
    for n in WALK_N:
        rows, meta = [], []
        for d in (-1, 1):
            p = 2300 if d < 0 else 300
            end = p if d < 0 else n - 1 - p                  # steps to the end of the row
            specs = [(f"near {k}", {k: base, 40: wall, 45: decoy}) for k in range(1, 9)]
            specs += [("block 32", {100: base, 300: wall, 310: decoy}), ("block 1024", {1000: base, 1800: wall, 1810: decoy}),
                      ("equal 32", {100: xp, 200: base, 300: wall}), ("above 32", {50: base, 100: up(xp), 200: decoy}),
                      ("equal 1024", {1000: xp, 1500: base, 1800: wall}), ("above 1024", {500: base, 1000: up(xp), 1500: decoy}),
                      ("end", {end: base}), ("end far", {50: base}), ("end near", {end - 1: base}),
                      ("nan", {149: base, 150: NAN, 160: decoy}), ("nan block", {700: base, 1000: NAN, 1500: decoy}),
                      ("nan first", {33: base, 34: NAN, 35: decoy})]
            for name, spec in specs:
                row = np.full(n, fill, dtype=F32)
                row[p] = xp
                row[p - 2 * d] = other
                for k, v in spec.items():
                    row[p + d * k] = v
                rows.append(row)
                meta.append((name, d, p))
        for prom in (10.0, float(np.nextafter(10.0, 0.0)), float(np.nextafter(10.0, 11.0))):
            case = _mark_case(f"walk n={n} prominence={prom!r}", rows, prominence=prom, max_list=12, meta=meta)
            if check:
                for r, (name, d, p) in enumerate(meta):
                    assert (p in _peaks_of(case, r)) == (prom <= 10.0), (n, prom, meta[r])
                    if prom <= 10.0:
                        assert case["want"]["prominences"][r][_peaks_of(case, r).index(p)] == 10.0, (n, meta[r])
            cases.append(case)
    return cases


def _okey(f):
    u = int(F32(f).view(np.int32))
    return u if u >= 0 else -(u & 0x7fffffff)


def _unkey(k):
    return np.array([k if k >= 0 else (-k) | 0x80000000], dtype=np.uint32).view(F32)[0]


def largest_passing(xp, prominence):
    """The largest float32 v below the peak with float64(xp) - float64(v) >= prominence (None: not even -inf), by bisection
    over the float32 values in their order: the difference is monotone in v."""
    with np.errstate(all="ignore"):
        ok = lambda k: bool(np.float64(xp) - np.float64(_unkey(k)) >= prominence)
        lo, hi = _okey(-np.inf), _okey(xp)
        if not ok(lo):
            return None
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return _unkey(lo)


PROMINENCES = (0.0, -1.0, np.inf, 6.3, 2.5000001, 1e-3, 6.0)
THR_PEAKS = (1e-3, 1e-30, 0.0, -80.25, -79.99999, 299.7, -299.7, 6.0, 6.3, 2.5, np.inf)


def marker_threshold_cases(check=False):
    """The float threshold of the prominence filter: for every peak level and prominence the base exactly on the pass
    boundary (largest_passing), one float32 step above (out) and below (in), next to the peak, behind the first six bins and
    in a skipped block; denormal and -inf bases."""
    cases = []
    for n in (300, 301):
        for prom in PROMINENCES:
            rows, meta = [], []
            for xp in THR_PEAKS:
                xp = F32(xp)
                edge = largest_passing(xp, prom)
                bases = [] if edge is None else [(edge, "on"), (up(edge), "above"), (up(edge, -1), "below")]
                bases += [(F32(1e-40), "denormal"), (F32(-1e-40), "denormal"), (F32(1.4e-45), "denormal"), (-INF, "ninf")]
                for b, kind in bases:
                    if not b < xp or (kind == "below" and edge == -INF):
                        continue
                    for k in (1, 9, 100):
                        row = np.full(n, up(xp, -1), dtype=F32)
                        row[150] = xp
                        row[150 - k] = row[150 + k] = b
                        rows.append(row)
                        meta.append((float(xp), kind, k, float(b)))
            case = _mark_case(f"threshold prominence={prom!r} n={n}", rows, prominence=prom, height=-np.inf, meta=meta)
            if check:
                verdicts = {}
                for r, (xp, kind, k, b) in enumerate(meta):
                    verdicts.setdefault((xp, kind), set()).add(150 in _peaks_of(case, r))
                for (xp, kind), v in verdicts.items():
                    if kind in ("on", "below", "ninf"):
                        assert v == {True}, (prom, xp, kind)
                    if kind == "above" and prom > 0:
                        # (behind the first bin the fill - one step below the peak - is met first: it passes only a prominence of one step)
                        assert False in v, (prom, xp, kind)
                if prom == 6.0:
                    assert largest_passing(F32(6.0), 6.0) == F32(2.0 ** -51)     # far above the floats next to float(6.0 - 6.0)
            cases.append(case)
    return cases


def marker_nopeak_cases(check=False):
    """Rows without a peak: snap_bin is np.argmax (the first NaN, the first of equal maxima), next_bin -1, the list padded."""
    cases = []
    for n in (1, 2, 3, 64, 65):
        k = np.arange(n, dtype=F32)
        rows = [k, -k, np.full(n, F32(7.0)), np.full(n, NAN), np.where(np.arange(n) == n // 2, NAN, F32(7.0)),
                np.where(np.arange(n) % 3 == 1, F32(9.0), F32(7.0)) if n < 3 else np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), F32(9.0), F32(7.0)),
                np.where(np.arange(n) >= n - 2, NAN, k), np.full(n, INF), np.full(n, -INF)]
        case = _mark_case(f"no peak n={n}", [np.asarray(r, dtype=F32) for r in rows], max_list=3, current_idx=0)
        if check:
            assert not case["want"]["n_peaks"].any() and set(case["want"]["next_bin"]) == {-1}
            assert [int(b) for b in case["want"]["snap_bin"]] == [int(np.argmax(r)) for r in case["rows"]]
            assert np.all(case["want"]["peaks"] == -1) and np.all(np.isnan(case["want"]["prominences"]))
        cases.append(case)
    return cases


def marker_rows_with_peaks(n=200):
    rows = []
    for shift, heights in ((0, (-20, -30, -25, -35)), (1, (-30, -20, -20, -25)), (2, (-40, -41, -42, -19))):
        row = np.full(n, F32(-100.0), dtype=F32)
        for p, h in zip((10, 50, 120, n - 2 - shift), heights):
            row[p + shift if p < 150 else p] = F32(h)
        rows.append(row)
    return rows


def marker_current_cases(check=False):
    """current_idx at -1, on, before and after every peak and at n: next_bin is the first peak right of it, wrapping."""
    cases = []
    for n in (200, 201):
        rows = marker_rows_with_peaks(n)
        seen = set()
        for cur in sorted({-1, n} | {p + o for p in (10, 11, 12, 50, 51, 52, 120, 121, 122, n - 2, n - 3, n - 4) for o in (-1, 0, 1)}):
            case = _mark_case(f"current_idx={cur} n={n}", rows, current_idx=cur, max_list=6)
            seen |= {(cur, int(b)) for b in case["want"]["next_bin"]}
            cases.append(case)
        if check:
            assert (n, 10) in seen and (-1, 10) in seen and (10, 50) in seen and (9, 10) in seen and (n - 2, 10) in seen and (n - 3, n - 2) in seen
    return cases


def marker_list_cases(check=False):
    cases = []
    for n in (200, 201):
        for max_list in (0, 1, 4, 7):
            case = _mark_case(f"max_list={max_list} n={n}", marker_rows_with_peaks(n), max_list=max_list)
            if check:
                assert set(case["want"]["n_peaks"]) == {4}
            cases.append(case)
    return cases


def marker_length_cases(n, check=False):
    """A peak at bin 1 and one at bin n - 2; every row of a batch different."""
    cases = []
    for count in (1, 2, 257):
        rows = []
        for r in range(count):
            row = np.full(n, F32(-100.0 - 0.5 * r), dtype=F32)
            if n >= 3:
                row[1] = F32(-0.25 * r)
                row[n - 2] = F32(-10.03125 - 0.125 * r)          # (never equal to the peak at bin 1)
                q = 3 + (7 * r) % max(n - 6, 1)
                if 4 <= q <= n - 5:                        # (three bins from either: distance 3 takes none of them)
                    row[q] = F32(-20.0 + 0.0625 * r)
            rows.append(row)
        case = _mark_case(f"lengths n={n} rows={count}", rows, current_idx=n // 2, max_list=4)
        if check:
            for r in range(count):
                got = _peaks_of(case, r)
                assert (1 in got and n - 2 in got) if n >= 6 else len(got) == (1 if n >= 3 else 0), (n, r, got)   # (n = 5: two bins apart, distance 3)
            assert len({row.tobytes() for row in case["rows"]}) == count
        cases.append(case)
    return cases


def all_marker_cases(check=False):
    out = marker_flat_cases(check) + marker_height_cases(check) + marker_distance_cases(check) + marker_walk_cases(check)
    out += marker_threshold_cases(check) + marker_nopeak_cases(check) + marker_current_cases(check) + marker_list_cases(check)
    for n in LENGTHS:
        out += marker_length_cases(n, check)
    return out
