"""tdsa_modq.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the one kernel
exists, uses no scratch and spills no register, VGPRs stay within 128, the static LDS is the header's constant, and
static plus dynamic LDS at K = 4096 stays inside what tdsa_modq.hpp declares."""
import functools

import pytest

from kernel_build import cross_compiled, header_const, in_makefile, no_scratch_no_spills
from topdogspectrumanalyser_amd import modquality as mq

_const = functools.partial(header_const, "tdsa_modq.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    # contraction is off for the file
    in_makefile("modq", ["tdsa_modq.hpp", "tdsa_modq_math.hpp", "tdsa_demod_math.hpp", "tdsa_wave.hpp"], own_flags="-ffp-contract=off")
    return cross_compiled(tmp_path_factory, "tdsa_modq.hip")


def test_modq_kernel_has_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    found = sorted(k for k in kernels if "modq_kernel" in k)
    assert len(found) == 1 and len(kernels) == 1, sorted(kernels)
    k = kernels[found[0]]
    print(found[0], k)
    no_scratch_no_spills(k)
    assert int(k["LDS Size [bytes/block]"]) == _const("kModqStaticLdsBytes"), k
    assert int(k["VGPRs"]) <= 128, k


def test_lds_at_the_largest_k_stays_inside_the_declared_budget():
    assert (_const("kModqThreads"), _const("kModqWaves")) == (256, 4)
    assert (_const("kModqMinSymbols"), _const("kModqMaxSymbols"), _const("kModqMaxPoints")) == (mq.MIN_SYMBOLS, mq.MAX_SYMBOLS, mq.MAX_POINTS)
    limit = _const("kModqMaxLdsBytes")
    assert limit <= 48 * 1024                                     # no opt-in for large dynamic LDS is needed
    assert 9 * mq.MAX_SYMBOLS + _const("kModqStaticLdsBytes") == limit
    assert _const("kModqMaxPoints") <= 256                        # an index is one byte
