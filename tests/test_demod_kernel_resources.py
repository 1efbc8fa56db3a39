"""tdsa_demod.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the expected
kernel instantiations exist, none uses scratch or spills a register, VGPRs stay within 128, the static LDS is what the
header budgets for, and the dynamic LDS the launcher asks for stays within a CU's 160 KiB for every (R, T) the library
accepts."""
import functools
import os

import pytest

from kernel_build import CSRC, cross_compiled, header_const, in_makefile, no_scratch_no_spills

KERNELS = {"demod_audio_kernel": 2, "demod_history_kernel": 2, "demod_post_kernel": 1}     # name -> instantiations (FM, AM)


_const = functools.partial(header_const, "tdsa_demod.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    in_makefile("demod", ["tdsa_demod.hpp", "tdsa_demod_math.hpp"])
    return cross_compiled(tmp_path_factory, "tdsa_demod.hip")


def test_demod_kernels_have_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    assert sorted(k for k in kernels if "demod_" in k) == sorted(k for k in kernels), sorted(kernels)
    for name, count in KERNELS.items():
        found = [k for k in kernels if name in k]
        assert len(found) == count, (name, sorted(kernels))
        for k in found:
            print(k, kernels[k])
            no_scratch_no_spills(kernels[k])
            assert int(kernels[k]["LDS Size [bytes/block]"]) <= _const("kDemodStaticLdsBytes"), (k, kernels[k])
            assert int(kernels[k]["VGPRs"]) <= 128, (k, kernels[k])      # 256 threads: four workgroups fit a CU's registers


def _lds_floats(R, Q):
    """demod_lds_floats of tdsa_demod.hpp."""
    blk, tile = _const("kDemodBlock"), _const("kDemodTile")
    last = tile + Q - 2
    rows = (last + last // blk + 1) | 1
    return -(-R // blk) * rows * blk


def test_dynamic_lds_fits_a_cu_for_every_accepted_shape():
    hpp = open(os.path.join(CSRC, "tdsa_demod.hpp")).read()
    assert "demod_prow(int j) { return j + j / kDemodBlock; }" in hpp
    assert "demod_stage_rows(int Q) { return (demod_prow(kDemodTile + Q - 2) + 1) | 1; }" in hpp
    assert "return (R + kDemodBlock - 1) / kDemodBlock * demod_stage_rows(Q) * kDemodBlock;" in hpp
    assert (_const("kDemodMaxChannels"), _const("kDemodMaxDecimation"), _const("kDemodMaxTapsPerPhase")) == (256, 64, 64)
    assert _const("kDemodTile") % (256 // _const("kDemodBlock") * _const("kDemodBlock")) == 0 and _const("kDemodPoleBlock") == 64
    limit, worst = _const("kDemodMaxLdsBytes"), 0
    assert limit == 160 * 1024
    for R in range(1, _const("kDemodMaxDecimation") + 1):
        for Q in range(1, _const("kDemodMaxTapsPerPhase") + 1):      # every T with ceil(T / R) = Q
            worst = max(worst, 4 * _lds_floats(R, Q))
    print("worst dynamic LDS per workgroup", worst)
    assert worst + _const("kDemodStaticLdsBytes") <= limit
    # the default filter (34 phases) at the bench's R = 6 leaves room for eight workgroups per CU
    assert 8 * 4 * _lds_floats(6, 34) <= limit
