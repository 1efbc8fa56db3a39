"""The two peak searches (top_peaks_kernel, marker_peaks_kernel in tdsa_analytics.hip) pinned against
tests/peaks_contract.py where they can go wrong: a valley's deciding bin in every region of its span (the accepted peak's
block, an interior block, the candidate's block, one shared block) and just outside it, one to eight accepted peaks, the
excursion on and a float32 step beside the threshold, the separation on both sides of the kernel's two sweeps, ties in
every unit of the argmax, NaN / inf rows; flat tops over every seam of the blocks of 32 bins, the distance rule's fixed
point down an 8191-peak staircase, the prominence walk into every kind of block, the filter's float threshold at the
pass boundary, every length from 1 to 16384, batches of 1, 2 and 257 different rows, rows at every 4-byte alignment, and
the C-ABI's argument checks.

No tolerance anywhere: bins and counts are integers, the dB values float32 copied from the row (compared as bit
patterns), the prominences float64 (bit patterns); padding is -1 / NaN.  Every family asserts on the CPU that its rows
discriminate (tests/test_peaks_host.py)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import peaks_contract as pc
from topdogspectrumanalyser_amd import DeviceBuffer

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]        # every test under a time limit of its own

F32 = np.float32
ERR_ARG = -1


def _nat():
    from topdogspectrumanalyser_amd import _native as nat
    return nat


@pytest.fixture(scope="module")
def an():
    from topdogspectrumanalyser_amd import analytics
    return analytics


@pytest.fixture(scope="module")
def eng():
    from topdogspectrumanalyser_amd import SpectrumEngine
    with SpectrumEngine(64, max_frames=1) as e:
        yield e


@contextlib.contextmanager
def _on_device(rows, offset=0):
    """The address of the rows on the device, `offset` bytes into a buffer whose base is aligned to 256 bytes."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    with DeviceBuffer(rows.nbytes + 64) as buf:
        assert buf.ptr % 256 == 0
        buf.put(rows, offset)
        yield buf.at(offset, rows.nbytes)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def _top_wrong(case, bins, db):
    """Rows of a call that differ from the contract."""
    rows, want = case["rows"], case["bins"]
    bad = []
    for r in range(len(rows)):
        k = int((want[r] >= 0).sum())
        ok = np.array_equal(bins[r], want[r]) and np.array_equal(_bits(db[r][:k]), _bits(rows[r][want[r][:k]])) \
            and np.all(np.isnan(db[r][k:]))
        if not ok:
            bad.append((r, bins[r].tolist(), want[r].tolist()))
    return bad


def _run_top(an, eng, cases, offset=0):
    bad = []
    for case in cases:
        with _on_device(case["rows"], offset) as d:
            bins, db = an.rows_top_peaks(eng, d, len(case["rows"]), n_bins=case["n"], n=case["n_peaks"],
                                         min_sep_bins=case["min_sep"], min_excursion_db=case["exc"])
        wrong = _top_wrong(case, bins, db)
        if wrong:
            bad.append((case["name"], len(wrong), wrong[:3], [case["meta"][r] for r, _, _ in wrong[:3]] if case.get("meta") else None))
    assert not bad, bad


def _mark_wrong(case, got):
    want, cap = case["want"], case["params"]["max_list"]
    bad = []
    for r in range(len(case["rows"])):
        ok = got["n_peaks"][r] == want["n_peaks"][r] and got["snap_bin"][r] == want["snap_bin"][r] \
            and got["next_bin"][r] == want["next_bin"][r]
        if cap > 0:
            k = int((want["peaks"][r] >= 0).sum())
            ok = ok and np.array_equal(got["peaks"][r], want["peaks"][r]) \
                and np.array_equal(_bits(got["prominences"][r][:k]), _bits(want["prominences"][r][:k])) \
                and np.all(np.isnan(got["prominences"][r][k:]))
        if not ok:
            bad.append((r, {k: np.asarray(v[r]).tolist() for k, v in got.items() if k != "prominences"},
                        {k: np.asarray(v[r]).tolist() for k, v in want.items() if k != "prominences"}))
    return bad


def _run_mark(an, eng, cases, offset=0):
    bad = []
    for case in cases:
        kw = case["params"]
        with _on_device(case["rows"], offset) as d:
            got = an.rows_marker_peaks(eng, d, len(case["rows"]), n_bins=case["n"], peak_threshold=kw["height"],
                                       peak_excursion=kw["prominence"], distance=kw["distance"], current_idx=kw["current_idx"],
                                       max_list=kw["max_list"])
        wrong = _mark_wrong(case, got)
        if wrong:
            bad.append((case["name"], len(wrong), wrong[:2], [case["meta"][r] for r, _, _ in wrong[:4]] if case.get("meta") else None))
    assert not bad, bad


# ---- top peaks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_valley_regions(an, eng, n):
    _run_top(an, eng, pc.top_valley_cases(n))


@pytest.mark.parametrize("n", pc.TOP_FIRST + (16384,))
def test_top_three_to_eight_accepted(an, eng, n):
    _run_top(an, eng, pc.top_many_cases(n))


@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_threshold(an, eng, n):
    _run_top(an, eng, pc.top_threshold_cases(n))


def test_top_excursion_is_a_float32(an, eng):
    """The constructed 6.3 case: the device agrees with the contract called with float32(6.3) - one peak - where the
    unrounded Python float would give two."""
    row = pc.excursion_63_row()
    with _on_device(row[None, :]) as d:
        bins, _ = an.rows_top_peaks(eng, d, 1, n_bins=len(row), n=5, min_sep_bins=2, min_excursion_db=6.3)
    assert bins[0].tolist() == [75, -1, -1, -1, -1] == pc.top_expected(row[None, :], 5, 2, float(F32(6.3)))[0][0].tolist()


@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_separation(an, eng, n):
    _run_top(an, eng, pc.top_separation_cases(n))


@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_ties(an, eng, n):
    _run_top(an, eng, pc.top_tie_cases(n))


@pytest.mark.parametrize("n", pc.TOP_FIRST + (16384,))
def test_top_nonfinite(an, eng, n):
    _run_top(an, eng, pc.top_nonfinite_cases(n))


@pytest.mark.parametrize("n", pc.LENGTHS)
def test_top_lengths_and_batches(an, eng, n):
    _run_top(an, eng, pc.top_length_cases(n))


@pytest.mark.parametrize("offset", (4, 8, 12))
def test_top_rows_at_every_alignment(an, eng, offset):
    _run_top(an, eng, pc.top_nonfinite_cases(1025) + pc.top_length_cases(1024)[:2] + pc.top_length_cases(33), offset)


def test_top_abi_arguments(eng):
    nat = _nat()
    rows = pc.top_length_cases(64)[1]["rows"]
    bins = np.full((2, 8), 77, dtype=np.int32)
    db = np.zeros((2, 8), dtype=F32)

    def call(ptr, n_rows=2, n_bins=64, n_peaks=5, sep=2, exc=6.0, bins_p=None, db_p=None):
        return nat.lib.tdsa_rows_top_peaks(eng._h, C.c_void_p(ptr), n_rows, n_bins, n_peaks, sep, exc,
                                           bins.ctypes.data_as(C.c_void_p) if bins_p is None else bins_p,
                                           db.ctypes.data_as(C.c_void_p) if db_p is None else db_p)
    with _on_device(rows) as d:
        assert call(d, exc=float("nan")) == ERR_ARG
        assert call(d, n_peaks=0) == ERR_ARG and call(d, n_peaks=9) == ERR_ARG
        assert call(d, n_bins=0) == ERR_ARG and call(d, n_bins=16385) == ERR_ARG
        assert call(d + 1) == ERR_ARG and call(d + 2) == ERR_ARG            # rows are floats: 4-byte aligned
        assert np.all(bins == 77)
        assert call(d, n_rows=0) == 0 and np.all(bins == 77)
        assert call(d, db_p=C.c_void_p()) == 0                              # a null peak_db_host is accepted
        want = pc.top_expected(rows, 5, 2, 6.0)[0]
        assert np.array_equal(bins.reshape(-1)[:10].reshape(2, 5), want)
        # min_sep_bins < 1 is "no separation rule" (tdsa_hip.h): the contract's `abs(a - b) < min_sep` never holds
        for sep in (0, -1, -2 ** 31):
            assert call(d, sep=sep) == 0
            assert np.array_equal(bins.reshape(-1)[:10].reshape(2, 5), pc.top_expected(rows, 5, sep, 6.0)[0])


# ---- markers ---------------------------------------------------------------------------------------------------------
def test_marker_flat_tops(an, eng):
    _run_mark(an, eng, pc.marker_flat_cases())


def test_marker_height(an, eng):
    _run_mark(an, eng, pc.marker_height_cases())


def test_marker_distance(an, eng):
    _run_mark(an, eng, pc.marker_distance_cases())


@pytest.mark.parametrize("n,mirror", ((16384, False), (16384, True), (16383, False), (16383, True)))
def test_marker_distance_staircase(an, eng, n, mirror):
    _run_mark(an, eng, [pc.marker_staircase_case(n, mirror)])


def test_marker_prominence_walk(an, eng):
    _run_mark(an, eng, pc.marker_walk_cases())


def test_marker_threshold_float(an, eng):
    _run_mark(an, eng, pc.marker_threshold_cases())


def test_marker_rows_without_a_peak(an, eng):
    _run_mark(an, eng, pc.marker_nopeak_cases())


def test_marker_current_idx(an, eng):
    _run_mark(an, eng, pc.marker_current_cases())


def test_marker_max_list(an, eng):
    _run_mark(an, eng, pc.marker_list_cases())


@pytest.mark.parametrize("n", pc.LENGTHS)
def test_marker_lengths_and_batches(an, eng, n):
    _run_mark(an, eng, pc.marker_length_cases(n))


@pytest.mark.parametrize("offset", (4, 8, 12))
def test_marker_rows_at_every_alignment(an, eng, offset):
    """Rows that start 4, 8 and 12 bytes into a buffer give the contract's answer, with n % 4 == 0 and without.  This pins
    the RESULT at every offset; it cannot tell which load path ran (the hardware tolerates a misaligned 16-byte load).  The
    path choice itself - 16-byte loads only where every row starts on 16 bytes - is pinned on the host, where
    tests/peaks_align_host.cpp enumerates the launcher's predicate (tests/test_peaks_host.py)."""
    cases = pc.marker_list_cases() + pc.marker_nopeak_cases() + pc.marker_length_cases(1024)[:2] + pc.marker_length_cases(64)
    assert any(c["n"] % 4 == 0 for c in cases) and any(c["n"] % 4 for c in cases)
    _run_mark(an, eng, cases, offset)


def test_marker_abi_arguments(eng):
    nat = _nat()
    case = pc.marker_list_cases()[2]
    rows, want, n = case["rows"], case["want"], case["n"]
    R, cap = len(rows), case["params"]["max_list"]
    cnt, snap, nxt = (np.full(R, 77, dtype=np.int32) for _ in range(3))
    lst = np.full((R, cap), 77, dtype=np.int32)

    def call(ptr, n_rows=R, n_bins=n, distance=3, max_list=cap, prominence=6.0, lst_p=lst.ctypes.data_as(C.c_void_p)):
        return nat.lib.tdsa_rows_marker_peaks(eng._h, C.c_void_p(ptr), n_rows, n_bins, -200.0, prominence, distance, -1, max_list,
                                              cnt.ctypes.data_as(C.c_void_p), snap.ctypes.data_as(C.c_void_p),
                                              nxt.ctypes.data_as(C.c_void_p), lst_p, None)
    with _on_device(rows) as d:
        assert call(d + 1) == ERR_ARG and call(d + 2) == ERR_ARG and call(d + 3) == ERR_ARG
        assert call(d, n_bins=0) == ERR_ARG and call(d, n_bins=16385) == ERR_ARG and call(d, distance=0) == ERR_ARG
        assert call(d, prominence=float("nan")) == ERR_ARG and call(d, lst_p=None) == ERR_ARG
        assert np.all(cnt == 77) and np.all(lst == 77)
        assert call(d, n_rows=0) == 0 and np.all(cnt == 77)
        assert call(d) == 0                                                 # a null peak_prom_host: the list alone
        assert np.array_equal(lst, want["peaks"]) and np.array_equal(cnt, want["n_peaks"])
        assert np.array_equal(snap, want["snap_bin"]) and np.array_equal(nxt, want["next_bin"])
        assert call(d, max_list=0, lst_p=None) == 0 and np.array_equal(cnt, want["n_peaks"])
