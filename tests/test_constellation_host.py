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
