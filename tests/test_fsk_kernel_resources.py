"""tdsa_fsk.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the two kernels
(complex64 and float32 input) exist, use no scratch and spill no register, VGPRs stay within 128, the static LDS is what
the header budgets for, and static plus dynamic LDS at K = 4096 stays inside what tdsa_fsk.hpp declares."""
import functools

import pytest

from kernel_build import cross_compiled, header_const, in_makefile, no_scratch_no_spills
from topdogspectrumanalyser_amd import fsk as fk

_const = functools.partial(header_const, "tdsa_fsk.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    # contraction is off for the file
    in_makefile("fsk", ["tdsa_fsk.hpp", "tdsa_fsk_math.hpp", "tdsa_symsync_math.hpp", "tdsa_demod_math.hpp", "tdsa_seg.hpp",
                        "tdsa_seg_block.hpp"],
                own_flags="-ffp-contract=off")
    return cross_compiled(tmp_path_factory, "tdsa_fsk.hip")


def test_fsk_kernels_have_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    found = sorted(k for k in kernels if "fsk_kernel" in k)
    assert len(found) == 2 and len(kernels) == 2, sorted(kernels)
    for name in found:
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["LDS Size [bytes/block]"]) <= _const("kFskStaticLdsBytes"), k
        assert int(k["VGPRs"]) <= 128, k


def test_lds_at_the_largest_k_stays_inside_the_declared_budget():
    assert (_const("kSegThreads"), _const("kSegMaxSymbols")) == (256, fk.MAX_SYMBOLS)
    assert (_const("kFskMaxBoxcar"), _const("kFskMaxLag")) == (fk.MAX_BOXCAR, fk.MAX_LAG)
    # a tile of e is whole rounds of the workgroup, and its b and d fit their arrays at the largest B and L
    assert _const("kFskTile") % _const("kSegThreads") == 0
    assert _const("kFskTileB") >= _const("kFskTile") + fk.MAX_LAG
    assert _const("kFskTileD") >= _const("kFskTileB") + fk.MAX_BOXCAR - 1
    limit = _const("kFskMaxLdsBytes")
    assert limit <= 48 * 1024                                     # no opt-in for large dynamic LDS is needed
    assert 4 * fk.MAX_SYMBOLS + _const("kFskStaticLdsBytes") <= limit
