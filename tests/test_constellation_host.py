"""Constellation analysis, host side (no GPU): the numpy restatement of Constellation2D.update_iq_data in
tests/constellation_contract.py is bit-exact against the vectors captured from the imported reference
(tests/golden/constellation.npz), the package builds the reference's point tables, and the new translation unit compiles
scratch-free for gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import constellation_contract as cc
from topdogspectrumanalyser_amd.analytics import constellation_points

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "constellation.npz"))


def _case(g, k):
    fmt, r, mp, scatter = g[f"c{k}_meta"]
    return int(fmt), float(r), int(mp), bool(scatter), str(g[f"c{k}_mod"])


def test_restatement_matches_reference_vectors(g):
    n_cases = int(g["n_cases"])
    assert n_cases >= 20
    for k in range(n_cases):
        fmt, r, mp, scatter, mod = _case(g, k)
        iq = cc.to_complex(g[f"c{k}_raw"], fmt)
        out = cc.evaluate(iq, mod, r)
        if g[f"c{k}_evm_none"]:
            assert out["evm"] is None, k
        else:
            want = float(g[f"c{k}_evm"])
            assert out["evm"] == want or (np.isnan(want) and np.isnan(out["evm"])), (k, out["evm"], want)
        assert cc.readout(out["evm"], mod) == str(g[f"c{k}_text"]), k
        if scatter:
            start = slice(-min(mp, len(iq)), None).indices(len(iq))[0]
            assert np.array_equal(out["i"][start:], g[f"c{k}_sx"], equal_nan=True), k
            assert np.array_equal(out["q"][start:], g[f"c{k}_sy"], equal_nan=True), k
        else:
            assert np.array_equal(out["counts"], g[f"c{k}_counts"]), k


def test_fixture_covers_the_contract(g):
    n_cases = int(g["n_cases"])
    lens = {len(cc.to_complex(g[f"c{k}_raw"], _case(g, k)[0])) for k in range(n_cases)}
    assert {5, 127, 8191, 8192, 8193, 16384, 100003} <= lens
    mods = {_case(g, k)[4] for k in range(n_cases)}
    assert {"bpsk", "qpsk", "8psk", "16qam", "64qam"} < mods
    assert {0, 1, 2} == {_case(g, k)[0] for k in range(n_cases)}
    assert {0.7, 1.5, 2.0} <= {_case(g, k)[1] for k in range(n_cases)}
    assert any(_case(g, k)[3] for k in range(n_cases)) and not all(_case(g, k)[3] for k in range(n_cases))


def test_package_tables_are_the_reference_tables(g):
    for name in ("bpsk", "qpsk", "8psk", "16qam", "64qam"):
        want = g[f"ref_{name}"]
        for got in (constellation_points(name), cc.reference_points(name)):
            assert got.dtype == want.dtype and np.array_equal(got, want), name
    assert constellation_points("ofdm") is None and cc.reference_points("ofdm") is None


@pytest.mark.parametrize("n", [1, 7, 8, 127, 128, 129, 200, 1000, 8191, 8192, 8193, 16384, 24577, 100003])
def test_summation_order_is_numpys(n):
    rng = np.random.default_rng(n)
    for dt in (np.float32, np.float64):
        x = (rng.random(n) * rng.random(n) * 10).astype(dt)
        assert cc.np_sum(x) == np.add.reduce(x), (n, dt)


def test_cabs_matches_numpy_absolute():
    rng = np.random.default_rng(5)
    z = (rng.standard_normal(1 << 18) + 1j * rng.standard_normal(1 << 18)).astype(np.complex64)
    z[:4] = [0, complex(np.inf, np.nan), complex(np.nan, 1), complex(3e-39, 0)]
    assert np.array_equal(cc.cabs(z), np.abs(z), equal_nan=True)


def test_constellation_kernels_compile_scratch_free():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "tdsa_constellation.hip", "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)\s+\[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = [k for k in kernels if "cst_" in k]
    assert len(names) >= 6, sorted(kernels)
    for k in names:
        assert kernels[k]["ScratchSize [bytes/lane]"] == "0", (k, kernels[k])
        assert int(kernels[k]["LDS Size [bytes/block]"]) <= 64 * 1024, (k, kernels[k])


def test_split_rule_stays_within_the_kernel_constants():
    """numpy's split rule walked for every partial-block length: the partial-block path of tdsa_constellation.hip
    lists the leaves in kMaxLeaves LDS slots and keeps one stack frame per recursion level in kStack."""
    src = open(os.path.join(CSRC, "tdsa_constellation.hip")).read()
    max_leaves = int(re.search(r"constexpr\s+int\s+kMaxLeaves\s*=\s*(\d+)\s*;", src).group(1))
    stack = int(re.search(r"constexpr\s+int\s+kStack\s*=\s*(\d+)\s*;", src).group(1))
    most_leaves = deepest = 0
    for n in range(1, 8193):
        leaves, depth = cc.split_leaves(n)
        assert sum(leaves) == n and all(1 <= k <= 128 for k in leaves), n
        if n > 128:
            assert min(leaves) >= 64, (n, min(leaves))
        most_leaves, deepest = max(most_leaves, len(leaves)), max(deepest, depth)
    assert most_leaves <= 65 and deepest <= 7, (most_leaves, deepest)
    # a frame per level: the deepest leaf's frame is stack slot `deepest`
    assert most_leaves <= max_leaves and deepest + 1 <= stack, (most_leaves, max_leaves, deepest, stack)
    # the walk is the one _pairwise sums by: leaf by leaf, combined in the same tree
    x = (np.random.default_rng(1).random(5000) * 100).astype(np.float32)
    leaves, _ = cc.split_leaves(len(x))
    at = np.concatenate([[0], np.cumsum(leaves)])
    sums = [cc._pairwise(x[a:b].reshape(1, -1))[0] for a, b in zip(at[:-1], at[1:])]

    def combine(n, it):
        if n <= 128:
            return next(it)
        n2 = n // 2 - (n // 2) % 8
        left = combine(n2, it)
        return np.float32(left + combine(n - n2, it))

    assert combine(len(x), iter(sums)) == np.add.reduce(x)


def test_explicit_table_overrides_the_modulation():
    rng = np.random.default_rng(6)
    iq = ((rng.standard_normal(9000) + 1j * rng.standard_normal(9000)) * 0.4).astype(np.complex64)
    for name in ("qpsk", "8psk", "64qam"):
        a = cc.evaluate(iq, name, 1.5)
        b = cc.evaluate(iq, "ofdm", 1.5, pts=cc.reference_points(name))
        assert a["evm"] == b["evm"] and np.array_equal(a["counts"], b["counts"]), name
    assert cc.evaluate(iq, "qpsk", 1.5, pts=np.zeros((0, 2), np.float32))["evm"] is None
    one = cc.evaluate(iq, pts=np.array([[0.25, -0.5]]))
    d = (one["i"].astype(np.float64) - 0.25) ** 2 + (one["q"].astype(np.float64) + 0.5) ** 2
    assert one["evm"] == float(np.sqrt(cc.np_mean(d)))


def test_float64_edges_are_decisive_at_range_0_7():
    """At range 0.7 most float64 edges are no float32 number: float32(edge) lies strictly on one side of its edge and
    a float32 compare would put it in the wrong bin.  At range 1.5 every edge is exact and neither compare bites."""
    e = cc.edges(0.7, 128)
    ef = e.astype(np.float32).astype(np.float64)
    assert (int((ef < e).sum()), int((ef > e).sum()), int((ef == e).sum())) == (52, 52, 25)
    e = cc.edges(1.5, 128)
    assert np.array_equal(e.astype(np.float32).astype(np.float64), e)


def test_sequential_fold_differs_from_numpys_tree():
    """The yardstick of the length sweep: a plain left-to-right float32 fold is another number than numpy's sum."""
    x = (np.random.default_rng(3).standard_normal(3000) ** 2 * 100).astype(np.float32)
    x[::50] *= np.float32(1e6)
    seq = np.float32(0)
    for v in x:
        seq = np.float32(seq + v)
    assert cc.sequential_sum(x) == seq and seq != cc.np_sum(x)


def test_rows_at_once_equal_row_by_row():
    """evaluate_rows (what the segment tests compare with) is evaluate of each row, bit for bit."""
    rng = np.random.default_rng(21)
    for n, table in ((1, "qpsk"), (7, "8psk"), (129, "16qam"), (8193, "qpsk"), (20011, "64qam")):
        rows = ((rng.standard_normal((6, n)) + 1j * rng.standard_normal((6, n))) * 0.4).astype(np.complex64)
        rows[1] = 0
        rows[2] *= np.float32(1e-11)                          # below the AGC threshold
        rows[3, n // 2] = complex(np.nan, 0.5)
        rows[4, 0] = complex(0.1, -np.inf)
        for r, bins in ((0.7, 127), (1.5, 128)):
            got = cc.evaluate_rows(rows, table, r, bins)
            for k in range(len(rows)):
                want = cc.evaluate(rows[k], table, r, bins)
                assert np.array_equal(got["rms"][k], want["rms"], equal_nan=True), (n, k)
                assert np.array_equal(got["evm"][k], want["evm"], equal_nan=True), (n, k)
                assert np.array_equal(got["counts"][k], want["counts"]), (n, k)
    none = cc.evaluate_rows(rows, "ofdm")
    assert np.isnan(none["evm"]).all() and np.array_equal(none["counts"], cc.evaluate_rows(rows, "qpsk")["counts"])
