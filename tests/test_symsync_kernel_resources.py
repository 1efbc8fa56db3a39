"""tdsa_symsync.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the one kernel
exists, uses no scratch and spills no register, VGPRs stay within 128, the static LDS is what the header budgets for,
and the dynamic LDS the launcher asks for stays within ~100 KiB of a CU's 160 for every K the library accepts."""
import functools

import pytest

from kernel_build import cross_compiled, header_const, in_makefile, no_scratch_no_spills
from topdogspectrumanalyser_amd import symbols as sy

_const = functools.partial(header_const, "tdsa_symsync.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    # contraction is off for the file
    in_makefile("symsync", ["tdsa_symsync.hpp", "tdsa_symsync_math.hpp", "tdsa_seg.hpp", "tdsa_seg_block.hpp"], own_flags="-ffp-contract=off")
    return cross_compiled(tmp_path_factory, "tdsa_symsync.hip")


def test_symsync_kernel_has_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    found = [k for k in kernels if "symsync_kernel" in k]
    assert len(found) == 1 and len(kernels) == 1, sorted(kernels)
    k = kernels[found[0]]
    print(found[0], k)
    no_scratch_no_spills(k)
    assert int(k["LDS Size [bytes/block]"]) <= _const("kSymStaticLdsBytes"), k
    assert int(k["VGPRs"]) <= 128, k


def test_dynamic_lds_stays_within_the_budget_for_every_accepted_k():
    assert (_const("kSegThreads"), _const("kSegMaxSymbols"), _const("kSymMaxGrid")) == (256, sy.MAX_SYMBOLS, 8192)
    limit = _const("kSymMaxLdsBytes")
    assert limit <= 101 * 1024                                   # y at most 32 KiB, the transform at most 64 KiB, scratch
    worst = 0
    for K in range(2, sy.MAX_SYMBOLS + 1):
        G = 2 * (1 << (K - 1).bit_length())
        assert G >= 2 * K and G <= _const("kSymMaxGrid")
        worst = max(worst, 8 * (K + G))
    print("worst dynamic LDS per workgroup", worst)
    assert worst + _const("kSymStaticLdsBytes") <= limit
