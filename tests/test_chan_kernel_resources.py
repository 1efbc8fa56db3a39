"""tdsa_chan.hip cross-compiled for gfx950 (no GPU): every kernel of the channelizer is free of scratch and of spilled
registers, its static LDS is what the launcher budgets for, and the dynamic LDS the launcher asks for stays within a
CU's 160 KiB for every shape the library accepts."""
import functools
import os

import pytest

from kernel_build import CSRC, cross_compiled, header_const, in_makefile, no_scratch_no_spills

KERNELS = {"chan_bank_kernel": 2, "chan_history_kernel": 1}      # name -> instantiations (oversampling 1 and 2)


_const = functools.partial(header_const, "tdsa_chan.hpp")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    in_makefile("chan", ["tdsa_chan.hpp"])
    return cross_compiled(tmp_path_factory, "tdsa_chan.hip", listing=True)


def test_chan_kernels_have_no_scratch_no_spills_and_the_budgeted_static_lds(compiled):
    kernels, _ = compiled
    assert sorted(k for k in kernels if "chan_" in k) == sorted(k for k in kernels), sorted(kernels)
    for name, count in KERNELS.items():
        found = [k for k in kernels if name in k]
        assert len(found) == count, (name, sorted(kernels))
        for k in found:
            print(k, kernels[k])
            no_scratch_no_spills(kernels[k])
            assert int(kernels[k]["LDS Size [bytes/block]"]) <= _const("kChanStaticLdsBytes"), (k, kernels[k])
            assert int(kernels[k]["VGPRs"]) <= 128, (k, kernels[k])      # 256 threads: four workgroups fit a CU's registers


def test_chan_fir_is_packed_and_nothing_goes_through_scratch(compiled):
    _, asm = compiled
    body = "\n".join(ln for ln in asm.splitlines() if not ln.lstrip().startswith((";", "//", ".")))
    assert "v_pk_fma_f32" in body                      # the branch FIR over (re, im)
    assert "ds_read_b64" in body or "ds_read2_b64" in body or "ds_read_b128" in body
    assert "scratch_" not in body


def _lds_samples(M, os_, P):
    """chan_lds_samples of tdsa_chan.hpp."""
    D, F, blk = M // os_, _const("kChanTilePoints") // M, _const("kChanBlock")
    staged = (F + P * os_ - 1) * D
    padded = staged + staged // (blk * D) * (M if M < 64 else 0)
    return max(padded, F * (M + (M // 64 if M > 64 else 1)))


def test_dynamic_lds_fits_a_cu_for_every_accepted_shape():
    hpp = open(os.path.join(CSRC, "tdsa_chan.hpp")).read()
    assert "(F + P * os - 1) * D" in hpp and "chan_stage_pad(int M) { return M < 64 ? M : 0; }" in hpp
    assert "chan_row(int M) { return M + (M > 64 ? M / 64 : 1); }" in hpp
    limit, static, worst = _const("kChanMaxLdsBytes"), _const("kChanStaticLdsBytes"), 0
    assert limit == 160 * 1024
    M = _const("kChanMinChannels")
    while M <= _const("kChanMaxChannels"):
        for os_ in (1, 2):
            for P in range(1, _const("kChanMaxTapsPerBranch") + 1):
                worst = max(worst, 8 * _lds_samples(M, os_, P) + static)
        M *= 2
    print("worst LDS per workgroup", worst)
    assert worst <= limit
    # at 32 taps per branch two workgroups share a CU even at 256 channels
    assert 2 * (8 * _lds_samples(256, 1, 32) + static) <= limit
