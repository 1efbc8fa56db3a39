"""tdsa_eye.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the three kernels
(IQ, FM, REAL) exist and nothing else does - the merge is the kernels' own tail -, they use no scratch and spill no
register, VGPRs stay within 128, the static LDS is what the header budgets for, and two uint32 images of the largest size
beside it stay inside what tdsa_eye.hpp declares."""
import functools

import pytest

from kernel_build import cross_compiled, header_const, in_makefile, no_scratch_no_spills, public_define
from topdogspectrumanalyser_amd import eye as ey

_const = functools.partial(header_const, "tdsa_eye.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    # contraction is off for the file
    in_makefile("eye", ["tdsa_eye.hpp", "tdsa_fsk.hpp", "tdsa_fsk_math.hpp", "tdsa_symsync.hpp", "tdsa_symsync_math.hpp",
                        "tdsa_demod_math.hpp", "tdsa_seg.hpp", "tdsa_seg_block.hpp"],
                own_flags="-ffp-contract=off")
    return cross_compiled(tmp_path_factory, "tdsa_eye.hip")


def test_eye_kernels_have_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    found = sorted(k for k in kernels if "eye_kernel" in k)
    assert len(found) == 3 and len(kernels) == 3, sorted(kernels)
    for name in found:
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["LDS Size [bytes/block]"]) <= _const("kEyeStaticLdsBytes"), k
        assert int(k["VGPRs"]) <= 128, k


def test_lds_at_the_largest_image_stays_inside_the_declared_budget():
    assert (_const("kEyeThreads"), _const("kSegMaxSymbols")) == (256, ey.MAX_SYMBOLS)
    assert (_const("kEyeMaxBins"), _const("kEyeMaxBoxcar")) == (ey.MAX_BINS, ey.MAX_BOXCAR) == (public_define("TDSA_EYE_MAX_BINS"), 64)
    assert (_const("kEyeMinRows"), _const("kEyeMaxRows")) == (ey.MIN_ROWS, ey.MAX_ROWS)
    assert (_const("kEyeMinPoints"), _const("kEyeMaxPoints")) == (ey.POINTS[0], ey.POINTS[-1])
    assert _const("kEyeMinSymbols") == ey.MIN_SYMBOLS and _const("kEyeTotals") == public_define("TDSA_EYE_TOTALS")
    # the tile holds complex64 samples in the room of its b and d, and the d its b need at the largest boxcar
    tile = _const("kEyeTile")
    assert _const("kEyeTileD") >= tile + ey.MAX_BOXCAR - 1
    assert (tile + _const("kEyeTileD")) * 4 >= tile * 8
    # a work item's symbols fit the tile at both ends of the rate, and it has at least one
    for step in (4 << 32, 64 << 32):
        spi = ((tile - 5) << 32) // step
        assert spi >= 1 and spi * step <= (tile - 5) << 32
    # a workgroup's uint32 bins cannot wrap: its items times the most points of one
    assert _const("kEyeItemsPerGroup") * (tile // 4) * ey.POINTS[-1] <= 1 << 31
    limit = _const("kEyeMaxLdsBytes")
    assert limit <= 160 * 1024
    assert 2 * ey.MAX_BINS * 4 + _const("kEyeStaticLdsBytes") <= limit
