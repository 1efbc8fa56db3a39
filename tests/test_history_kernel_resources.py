"""tdsa_history.hip cross-compiled for gfx950 (no GPU): every kernel of the 3-D history views is free of scratch and of
spilled registers, the translation unit is built with -ffp-contract=off, its divisions are the IEEE sequences, and its
wide stores are the global stores the compiler pads on gfx950, not buffer stores with a register offset."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"hist_push_kernel": 2, "hist_reduce_kernel": 1, "hist_ribbon_kernel": 2, "hist_lines_kernel": 2,
           "hist_surface_kernel": 2}      # name -> instantiations (16-byte and one-bin lanes)


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/tdsa_history.o" in mk and re.search(r"^CAPI\s*=.*\bhistory\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_history\.hpp\b", mk, re.M)
    assert re.search(r"^\$\(B\)/tdsa_history\.o:\s*EXTRA\s*\+=\s*-ffp-contract=off\s*$", mk, re.M), \
        "the history views restate numpy operation by operation: no contraction into FMA"
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    return [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + ["-ffp-contract=off", "--cuda-device-only"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    asm = str(tmp_path_factory.mktemp("history") / "tdsa_history.s")
    r = subprocess.run(_flags() + ["-Rpass-analysis=kernel-resource-usage", "-S", "tdsa_history.hip", "-o", asm],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr, open(asm).read()


def test_history_kernels_have_no_scratch_and_no_spills(compiled):
    remarks, _ = compiled
    kernels, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)\s+\[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    for name, count in KERNELS.items():
        found = [k for k in kernels if name in k]
        assert len(found) == count, (name, sorted(kernels))
        for k in found:
            print(k, kernels[k])
            assert kernels[k]["ScratchSize [bytes/lane]"] == "0", (k, kernels[k])
            assert kernels[k].get("VGPRs Spill", "0") == "0", (k, kernels[k])
            assert kernels[k].get("SGPRs Spill", "0") == "0", (k, kernels[k])
            assert kernels[k]["LDS Size [bytes/block]"] == "0", (k, kernels[k])      # streaming passes and shuffles
            assert int(kernels[k]["VGPRs"]) <= 64, (k, kernels[k])                     # eight waves per SIMD stay possible


def test_history_divisions_are_ieee_and_stores_are_global(compiled):
    """(The fused multiply-adds that remain belong to the correctly rounded division sequences; that nothing else is
    contracted is what the bit-for-bit GPU tests show.)"""
    _, asm = compiled
    body = "\n".join(ln for ln in asm.splitlines() if not ln.lstrip().startswith((";", "//", ".")))
    assert "v_div_fixup_f32" in body and "v_div_fixup_f64" in body               # not the reciprocal approximation
    assert "global_store_dwordx4" in body and "global_load_dwordx4" in body      # 16-byte lanes
    assert "buffer_store" not in body
    assert "scratch_" not in body
