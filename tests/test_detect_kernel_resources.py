"""tdsa_detect.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the kernel's
two load paths exist, use no scratch and spill no register, VGPRs stay within 128, and the LDS of a workgroup - the
static part the compiler reports plus the row the launcher asks for - stays within 80 KiB, so that two workgroups fit a
CU's 160 KiB."""
import os
import re
import shutil

import pytest

from kernel_build import CSRC, HIPCC, compile_kernels, makefile
from topdogspectrumanalyser_amd import detect as dt


def _const(name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, open(os.path.join(CSRC, "tdsa_detect.hpp")).read())
    expr = re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), m.group(1))
    return int(eval(expr))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = makefile()
    assert "$(B)/tdsa_detect.o" in mk and re.search(r"^CAPI\s*=.*\bdetect\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_detect\.hpp\b", mk, re.M) and re.search(r"^HDRS\s*=.*\btdsa_rows_align\.hpp\b", mk, re.M)
    assert not re.search(r"^\$\(B\)/tdsa_detect\.o:", mk, re.M)          # no flags of its own: the Makefile's
    return compile_kernels("tdsa_detect.hip", str(tmp_path_factory.mktemp("detect") / "tdsa_detect.o"))


def test_detect_kernel_has_no_scratch_no_spills_and_fits_two_workgroups_per_cu(kernels):
    found = [k for k in kernels if "detect_kernel" in k]
    assert len(found) == 2 and len(kernels) == 2, sorted(kernels)          # 16-byte loads and float loads
    row_bytes = 4 * _const("kDetMaxBins")
    for name in found:
        k = kernels[name]
        print(name, k)
        assert k["ScratchSize [bytes/lane]"] == "0", k
        assert k.get("VGPRs Spill", "0") == "0" and k.get("SGPRs Spill", "0") == "0", k
        assert int(k["VGPRs"]) <= 128, k
        assert int(k["LDS Size [bytes/block]"]) <= _const("kDetStaticLdsBytes"), k
        assert int(k["LDS Size [bytes/block]"]) + row_bytes <= 80 * 1024, k


def test_the_header_budgets_what_the_python_layer_promises():
    assert (_const("kDetThreads"), _const("kDetMaxBins"), _const("kDetMaxSignals")) == (256, dt.MAX_BINS, dt.MAX_SIGNALS)
    assert _const("kDetWords") * 64 == dt.MAX_BINS and _const("kDetWords") == _const("kDetThreads")
    assert _const("kDetMaxLdsBytes") == 4 * dt.MAX_BINS + _const("kDetStaticLdsBytes") <= 80 * 1024
