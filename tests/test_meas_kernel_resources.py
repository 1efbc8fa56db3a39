"""tdsa_meas.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the kernel's two
load paths exist, use no scratch and spill no register, VGPRs stay within 128, and the LDS of a workgroup - the static
part the compiler reports plus the padded row the launcher asks for - stays within 80 KiB, so that two workgroups fit a
CU's 160 KiB."""
import functools
import os

import pytest

from kernel_build import CSRC, cross_compiled, header_const, in_makefile, no_scratch_no_spills
from topdogspectrumanalyser_amd import measure as ms


_const = functools.partial(header_const, "tdsa_meas.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    in_makefile("meas", ["tdsa_meas.hpp", "tdsa_wave.hpp"])      # no flags of its own: the Makefile's
    return cross_compiled(tmp_path_factory, "tdsa_meas.hip")


def test_meas_kernel_has_no_scratch_no_spills_and_fits_two_workgroups_per_cu(kernels):
    found = [k for k in kernels if "meas_kernel" in k]
    assert len(found) == 2 and len(kernels) == 2, sorted(kernels)          # 16-byte loads and float loads
    row_bytes = 4 * _const("kMeasRowFloats")
    for name in found:
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= 128, k
        assert int(k["LDS Size [bytes/block]"]) <= _const("kMeasStaticLdsBytes"), k
        assert int(k["LDS Size [bytes/block]"]) + row_bytes <= 80 * 1024, k


def test_the_header_budgets_what_the_python_layer_promises():
    assert (_const("kMeasThreads"), _const("kMeasMaxBins"), _const("kMeasMaxChannels")) == (256, ms.MAX_BINS, ms.MAX_CHANNELS)
    assert _const("kMeasOwn") * _const("kMeasThreads") == ms.MAX_BINS     # one thread per 64 bins of the widest row
    assert _const("kMeasRowFloats") == ms.MAX_BINS + ms.MAX_BINS // 64   # one float of padding per 64 bins
    assert _const("kMeasMaxLdsBytes") == 4 * _const("kMeasRowFloats") + _const("kMeasStaticLdsBytes") <= 80 * 1024
    assert _const("kMeasMaxGrid") == 2048


def test_the_lane_folds_are_the_shared_headers():
    src = [ln for ln in open(os.path.join(CSRC, "tdsa_meas.hip")).read().splitlines() if not ln.lstrip().startswith("//")]
    for idiom in ("__shfl", "__builtin_amdgcn_update_dpp", "atomic"):
        assert not [ln for ln in src if idiom in ln], idiom
    assert any("wave_sum<64>" in ln for ln in src) and any('#include "tdsa_wave.hpp"' in ln for ln in src)
