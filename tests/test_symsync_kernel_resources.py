"""tdsa_symsync.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the one kernel
exists, uses no scratch and spills no register, VGPRs stay within 128, the static LDS is what the header budgets for,
and the dynamic LDS the launcher asks for stays within ~100 KiB of a CU's 160 for every K the library accepts."""
import os
import re
import shutil

import pytest

from kernel_build import CSRC, HIPCC, compile_kernels, flags, makefile
from topdogspectrumanalyser_amd import symbols as sy


def _const(name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, open(os.path.join(CSRC, "tdsa_symsync.hpp")).read())
    expr = re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), m.group(1))
    return int(eval(expr))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    mk = makefile()
    assert "$(B)/tdsa_symsync.o" in mk and re.search(r"^CAPI\s*=.*\bsymsync\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_symsync\.hpp\b", mk, re.M) and re.search(r"^HDRS\s*=.*\btdsa_symsync_math\.hpp\b", mk, re.M)
    assert re.search(r"^\$\(B\)/tdsa_symsync\.o: EXTRA \+= -ffp-contract=off$", mk, re.M)      # contraction is off for the file
    assert "-ffp-contract=off" in flags("tdsa_symsync.hip")
    return compile_kernels("tdsa_symsync.hip", str(tmp_path_factory.mktemp("symsync") / "tdsa_symsync.o"))


def test_symsync_kernel_has_no_scratch_no_spills_and_the_budgeted_static_lds(kernels):
    found = [k for k in kernels if "symsync_kernel" in k]
    assert len(found) == 1 and len(kernels) == 1, sorted(kernels)
    k = kernels[found[0]]
    print(found[0], k)
    assert k["ScratchSize [bytes/lane]"] == "0", k
    assert k.get("VGPRs Spill", "0") == "0" and k.get("SGPRs Spill", "0") == "0", k
    assert int(k["LDS Size [bytes/block]"]) <= _const("kSymStaticLdsBytes"), k
    assert int(k["VGPRs"]) <= 128, k


def test_dynamic_lds_stays_within_the_budget_for_every_accepted_k():
    assert (_const("kSymThreads"), _const("kSymMaxSymbols"), _const("kSymMaxGrid")) == (256, sy.MAX_SYMBOLS, 8192)
    limit = _const("kSymMaxLdsBytes")
    assert limit <= 101 * 1024                                   # y at most 32 KiB, the transform at most 64 KiB, scratch
    worst = 0
    for K in range(2, sy.MAX_SYMBOLS + 1):
        G = 2 * (1 << (K - 1).bit_length())
        assert G >= 2 * K and G <= _const("kSymMaxGrid")
        worst = max(worst, 8 * (K + G))
    print("worst dynamic LDS per workgroup", worst)
    assert worst + _const("kSymStaticLdsBytes") <= limit
