"""tdsa_detect.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the kernel's
two load paths exist, use no scratch and spill no register, VGPRs stay within 128, and the LDS of a workgroup - the
static part the compiler reports plus the row the launcher asks for - stays within 80 KiB, so that two workgroups fit a
CU's 160 KiB."""
import functools

import pytest

from kernel_build import cross_compiled, header_const, in_makefile, no_scratch_no_spills
from topdogspectrumanalyser_amd import detect as dt


_const = functools.partial(header_const, "tdsa_detect.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    in_makefile("detect", ["tdsa_detect.hpp", "tdsa_rows_align.hpp"])      # no flags of its own: the Makefile's
    return cross_compiled(tmp_path_factory, "tdsa_detect.hip")


def test_detect_kernel_has_no_scratch_no_spills_and_fits_two_workgroups_per_cu(kernels):
    found = [k for k in kernels if "detect_kernel" in k]
    assert len(found) == 2 and len(kernels) == 2, sorted(kernels)          # 16-byte loads and float loads
    row_bytes = 4 * _const("kDetMaxBins")
    for name in found:
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= 128, k
        assert int(k["LDS Size [bytes/block]"]) <= _const("kDetStaticLdsBytes"), k
        assert int(k["LDS Size [bytes/block]"]) + row_bytes <= 80 * 1024, k


def test_the_header_budgets_what_the_python_layer_promises():
    assert (_const("kDetThreads"), _const("kDetMaxBins"), _const("kDetMaxSignals")) == (256, dt.MAX_BINS, dt.MAX_SIGNALS)
    assert _const("kDetWords") * 64 == dt.MAX_BINS and _const("kDetWords") == _const("kDetThreads")
    assert _const("kDetMaxLdsBytes") == 4 * dt.MAX_BINS + _const("kDetStaticLdsBytes") <= 80 * 1024
