"""tdsa_history.hip cross-compiled for gfx950 (no GPU): every kernel of the 3-D history views is free of scratch and of
spilled registers, the translation unit is built with -ffp-contract=off, its divisions are the IEEE sequences, and its
wide stores are the global stores the compiler pads on gfx950, not buffer stores with a register offset."""
import pytest

from kernel_build import cross_compiled, in_makefile, no_scratch_no_spills

KERNELS = {"hist_push_kernel": 2, "hist_reduce_kernel": 1, "hist_ribbon_kernel": 2, "hist_lines_kernel": 2,
           "hist_surface_kernel": 2}      # name -> instantiations (16-byte and one-bin lanes)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    # the history views restate numpy operation by operation: no contraction into FMA
    in_makefile("history", ["tdsa_history.hpp"], own_flags="-ffp-contract=off")
    return cross_compiled(tmp_path_factory, "tdsa_history.hip", listing=True)


def test_history_kernels_have_no_scratch_and_no_spills(compiled):
    kernels, _ = compiled
    for name, count in KERNELS.items():
        found = [k for k in kernels if name in k]
        assert len(found) == count, (name, sorted(kernels))
        for k in found:
            print(k, kernels[k])
            no_scratch_no_spills(kernels[k])
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
