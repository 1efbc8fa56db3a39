"""The peak searches, host side (no GPU): every row family of tests/peaks_contract.py discriminates (its builders assert it
with check=True: a notch changes the answer, a decoy does not but would with a valley one block wider, the two sides of
every threshold differ ...), the marker rows agree with the real scipy.signal.find_peaks, the stable-order top-peaks
contract reproduces the vectors recorded from the reference, and the float32-excursion decision is what the constructed
6.3 case says it is."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import peaks_contract as pc
from oracle import analytics_oracle as ao

F32 = np.float32
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- top peaks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_valley_rows_discriminate(n):
    (case,) = pc.top_valley_cases(n, check=True)
    kinds = [m[0] for m in case["meta"]]
    assert kinds.count("notch") > 100 and kinds.count("decoy") > 100
    assert pc.top_threads(n) == {417: 64, 1024: 64, 1025: 128, 2048: 128, 2049: 256, 4096: 256, 4097: 512, 8192: 512}.get(n, 1024)


@pytest.mark.parametrize("n", pc.TOP_FIRST + (16384,))
def test_top_many_and_nonfinite_rows_discriminate(n):
    cases = pc.top_many_cases(n, check=True)
    assert {m[0] for m in cases[0]["meta"]} == set(range(1, 8)) and [c["n_peaks"] for c in cases[1:]] == list(range(1, 9))
    (case,) = pc.top_nonfinite_cases(n, check=True)
    assert {m[0] for m in case["meta"]} == {"none", "nan", "ninf", "decoy", "kill", "empty"}


@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_separation_and_tie_rows_discriminate(n):
    T = pc.top_threads(n)
    seps = {c["min_sep"] for c in pc.top_separation_cases(n, check=True)}
    assert seps >= {1, 2, T // 2, T // 2 + 1, n, n + 5, 0} and (n < 4 * T + 16 or 2 * T + 3 in seps)
    assert len(pc.top_tie_cases(n, check=True)) == 7


@pytest.mark.parametrize("n", pc.TOP_FIRST + pc.TOP_LAST)
def test_top_threshold_rows_discriminate_at_every_width(n):
    assert [c["exc"] for c in pc.top_threshold_cases(n, check=True)] == list(pc.EXCURSIONS)


def test_the_excursion_is_a_float32():
    # the constructed case of the float32 decision: contract (rounded) one peak, the unrounded Python float two
    row = pc.excursion_63_row()
    assert float(F32(6.3)) > float(row[75]) - float(row[41]) > 6.3          # the float64 difference lies between the two
    assert pc.top_peaks(row, 5, 2, 6.3) == pc.top_peaks(row, 5, 2, float(F32(6.3))) == [75]
    raw = ao.find_top_peaks(np.arange(len(row), dtype=np.float64), row, 5, 2, 6.3, kind="stable")
    assert [int(f) for f, _ in raw] == [75, 40]


def test_top_length_rows_discriminate():
    for n in pc.LENGTHS:
        assert [len(c["rows"]) for c in pc.top_length_cases(n, check=True)] == [1, 2, 257]
    assert {pc.top_threads(n) for n in pc.TOP_FIRST} == {pc.top_threads(n) for n in pc.TOP_LAST} == {64, 128, 256, 512, 1024}


def test_restated_variant_without_its_mistakes_is_the_contract():
    for case in pc.top_many_cases(417) + pc.top_nonfinite_cases(1025) + pc.top_tie_cases(2049) + pc.top_threshold_cases(417):
        for r, row in enumerate(case["rows"]):
            got = pc.top_peaks_variant(row, case["n_peaks"], case["min_sep"], case["exc"])
            assert got == [int(b) for b in case["bins"][r] if b >= 0], (case["name"], r)


def test_stable_order_contract_reproduces_the_recorded_peak_cases(golden_dir):
    gold = np.load(os.path.join(golden_dir, "analytics.npz"))
    keys = [str(k) for k in gold["peak_cases"]]
    assert len(keys) >= 8
    for key in keys:
        n, _, exc = key.split("_")[1:]
        tr = gold[key + "_trace"]
        sep = max(10, int(n) // 50)
        ours = ao.find_top_peaks(np.arange(int(n), dtype=np.float64), tr, 5, sep, float(exc), kind="stable")
        assert [int(f) for f, _ in ours] == list(gold[key + "_bins"]), key
        assert pc.top_peaks(tr, 5, sep, float(exc)) == list(gold[key + "_bins"]), key
        assert np.array_equal(np.array([p for _, p in ours]), gold[key + "_pwr"]), key


# ---- markers ---------------------------------------------------------------------------------------------------------
FAMILIES = {"flat": pc.marker_flat_cases, "height": pc.marker_height_cases, "distance": pc.marker_distance_cases,
            "walk": pc.marker_walk_cases, "threshold": pc.marker_threshold_cases, "nopeak": pc.marker_nopeak_cases,
            "current": pc.marker_current_cases, "list": pc.marker_list_cases}


def _against_scipy(case):
    find_peaks = pytest.importorskip("scipy.signal").find_peaks
    kw, want = case["params"], case["want"]
    compared = 0
    for r, row in enumerate(case["rows"]):
        if case["ties"][r]:
            continue                                       # scipy's order between equal peaks within `distance` is undefined
        with np.errstate(all="ignore"):
            pk, props = find_peaks(row.astype(np.float64), height=kw["height"], prominence=kw["prominence"], distance=kw["distance"])
        m = min(len(pk), kw["max_list"])
        assert len(pk) == want["n_peaks"][r], (case["name"], r)
        assert np.array_equal(pk[:m], want["peaks"][r][:m]) and np.all(want["peaks"][r][m:] == -1), (case["name"], r)
        assert np.array_equal(props["prominences"][:m], want["prominences"][r][:m]), (case["name"], r)
        if len(pk):
            assert want["snap_bin"][r] == pk[int(np.argmax(props["peak_heights"]))], (case["name"], r)
            right = pk[pk > kw["current_idx"]]
            assert want["next_bin"][r] == (right[0] if len(right) else pk[0]), (case["name"], r)
        compared += 1
    return compared


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_marker_rows_discriminate_and_agree_with_scipy(family):
    cases = FAMILIES[family](True)
    compared = sum(_against_scipy(case) for case in cases)
    ties = sum(int(case["ties"].sum()) for case in cases)
    assert compared > 0 and (ties > 0) == (family == "distance")           # only the family built for ties holds any
    assert {case["n"] % 4 == 0 for case in cases} == {True, False}          # both load paths of the kernel


@pytest.mark.parametrize("n", pc.LENGTHS)
def test_marker_length_rows_discriminate_and_agree_with_scipy(n):
    cases = pc.marker_length_cases(n, True)
    assert [len(c["rows"]) for c in cases] == [1, 2, 257] and not any(c["ties"].any() for c in cases)
    assert sum(_against_scipy(case) for case in cases) == 260


def test_flat_tops_cover_every_width_and_both_load_paths():
    cases = pc.marker_flat_cases()
    assert [c["n"] % 4 for c in cases] == [0, 1]
    assert {m[0] for m in cases[0]["meta"] if m[2] == "fall"} == set(pc.FLAT_WIDTHS)


def test_staircase_closed_form_is_the_oracle_and_scipy():
    for n, mirror in ((1024, False), (1024, True), (1023, False), (1023, True), (64, True), (9, False)):
        case = pc.marker_staircase_case(n, mirror)
        want = pc.marker_expected(case["rows"], **case["params"])
        for k in want:
            assert np.array_equal(want[k], case["want"][k], equal_nan=True), (n, mirror, k)
    for n, mirror in ((16384, False), (16384, True), (16383, False), (16383, True)):
        case = pc.marker_staircase_case(n, mirror)
        assert case["want"]["n_peaks"][0] == 4096 and not pc.close_ties(case["rows"][0], -200.0, 3)
        assert _against_scipy(case) == 1


def test_pass_boundary_of_the_prominence_filter():
    """largest_passing is the boundary the threshold rows are built on: it passes, the next float32 does not."""
    for xp in pc.THR_PEAKS:
        for prom in pc.PROMINENCES:
            edge = pc.largest_passing(F32(xp), prom)
            if edge is None:
                continue
            with np.errstate(all="ignore"):
                assert edge < F32(xp) and np.float64(F32(xp)) - np.float64(edge) >= prom
                nxt = pc.up(edge)
                assert not nxt < F32(xp) or not np.float64(F32(xp)) - np.float64(nxt) >= prom
    # peak and prominence cancel: the boundary is half a float64 step of the PEAK, thousands of float32 steps above zero
    assert pc.largest_passing(F32(6.0), 6.0) == F32(2.0 ** -51) and pc.largest_passing(F32(6.0), np.inf) == -np.inf


def test_marker_load_path_is_chosen_by_the_alignment_of_every_row(tmp_path):
    """launch_marker_peaks takes the 16-byte loads where tdsa_rows_align.hpp says so; tests/peaks_align_host.cpp enumerates
    that predicate over every byte offset of a base and every n against "every row of the batch starts on 16 bytes"."""
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm's host compiler not available")
    exe = str(tmp_path / "peaks_align_host")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "peaks_align_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    src = open(os.path.join(CSRC, "tdsa_analytics.hip")).read()
    launcher = src[src.index("hipError_t launch_marker_peaks"):src.index("hipError_t launch_density")]
    assert "const int vec = rows_take_vec16(rows, n) ? 1 : 0;" in launcher and "max_list, vec," in launcher
    kernel = src[src.index("void __launch_bounds__(kMarkThreads) marker_peaks_kernel"):src.index("// ---- density histogram")]
    assert "if (vec) {" in kernel and "(n & 3) == 0" not in kernel            # the kernel follows the launcher's flag alone
