"""tdsa_meas.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the kernel's two
load paths exist, use no scratch and spill no register, VGPRs stay within 128, and the LDS of a workgroup - the static
part the compiler reports plus the padded row the launcher asks for - stays within 80 KiB, so that two workgroups fit a
CU's 160 KiB."""
import os
import re
import shutil

import pytest

from kernel_build import CSRC, HIPCC, compile_kernels, makefile
from topdogspectrumanalyser_amd import measure as ms


def _const(name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, open(os.path.join(CSRC, "tdsa_meas.hpp")).read())
    expr = re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), m.group(1))
    return int(eval(expr))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = makefile()
    assert "$(B)/tdsa_meas.o" in mk and re.search(r"^CAPI\s*=.*\bmeas\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_meas\.hpp\b", mk, re.M) and re.search(r"^HDRS\s*=.*\btdsa_wave\.hpp\b", mk, re.M)
    assert not re.search(r"^\$\(B\)/tdsa_meas\.o:", mk, re.M)            # no flags of its own: the Makefile's
    return compile_kernels("tdsa_meas.hip", str(tmp_path_factory.mktemp("meas") / "tdsa_meas.o"))


def test_meas_kernel_has_no_scratch_no_spills_and_fits_two_workgroups_per_cu(kernels):
    found = [k for k in kernels if "meas_kernel" in k]
    assert len(found) == 2 and len(kernels) == 2, sorted(kernels)          # 16-byte loads and float loads
    row_bytes = 4 * _const("kMeasRowFloats")
    for name in found:
        k = kernels[name]
        print(name, k)
        assert k["ScratchSize [bytes/lane]"] == "0", k
        assert k.get("VGPRs Spill", "0") == "0" and k.get("SGPRs Spill", "0") == "0", k
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
