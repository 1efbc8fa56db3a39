"""tdsa_history.hip cross-compiled for gfx950 (no GPU): every kernel of the 3-D history views is free of scratch and of
spilled registers, the translation unit is built with -ffp-contract=off, its divisions are the IEEE sequences, and its
wide stores are the global stores the compiler pads on gfx950, not buffer stores with a register offset."""
import re
import shutil

import pytest

from kernel_build import HIPCC, compile_kernels, flags, makefile

KERNELS = {"hist_push_kernel": 2, "hist_reduce_kernel": 1, "hist_ribbon_kernel": 2, "hist_lines_kernel": 2,
           "hist_surface_kernel": 2}      # name -> instantiations (16-byte and one-bin lanes)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = makefile()
    assert "$(B)/tdsa_history.o" in mk and re.search(r"^CAPI\s*=.*\bhistory\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_history\.hpp\b", mk, re.M)
    assert re.search(r"^\$\(B\)/tdsa_history\.o:\s*EXTRA\s*\+=\s*-ffp-contract=off\s*$", mk, re.M), \
        "the history views restate numpy operation by operation: no contraction into FMA"
    assert "-ffp-contract=off" in flags("tdsa_history.hip")
    asm = str(tmp_path_factory.mktemp("history") / "tdsa_history.s")
    return compile_kernels("tdsa_history.hip", asm), open(asm).read()


def test_history_kernels_have_no_scratch_and_no_spills(compiled):
    kernels, _ = compiled
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
