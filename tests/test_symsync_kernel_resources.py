"""tdsa_symsync.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the one kernel
exists, uses no scratch and spills no register, VGPRs stay within 128, the static LDS is what the header budgets for,
and the dynamic LDS the launcher asks for stays within ~100 KiB of a CU's 160 for every K the library accepts."""
import os
import re
import shutil
import subprocess

import pytest

from topdogspectrumanalyser_amd import symbols as sy

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _const(name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, open(os.path.join(CSRC, "tdsa_symsync.hpp")).read())
    expr = re.sub(r"\bk\w+", lambda k: str(_const(k.group(0))), m.group(1))
    return int(eval(expr))


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/tdsa_symsync.o" in mk and re.search(r"^CAPI\s*=.*\bsymsync\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\btdsa_symsync\.hpp\b", mk, re.M) and re.search(r"^HDRS\s*=.*\btdsa_symsync_math\.hpp\b", mk, re.M)
    assert re.search(r"^\$\(B\)/tdsa_symsync\.o: EXTRA \+= -ffp-contract=off$", mk, re.M)      # contraction is off for the file
    extra = re.search(r"^EXTRA\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    return [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + ["-ffp-contract=off", "--cuda-device-only"]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("symsync") / "tdsa_symsync.o")
    r = subprocess.run(_flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "tdsa_symsync.hip", "-o", out],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def test_symsync_kernel_has_no_scratch_no_spills_and_the_budgeted_static_lds(remarks):
    kernels, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)\s+\[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
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
