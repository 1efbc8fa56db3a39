"""tdsa_corr.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: no kernel uses
scratch or spills a register, every one stays within the registers and the LDS that tdsa_corr.hpp states, and the
workgroups per CU follow from them.  The Makefile builds the unit with fused multiply-adds only where the kernel writes
them, the header's constants are those correlate.py and include/tdsa_hip.h promise, atomics are integer, and nothing is
launched cooperatively or waits for another workgroup."""
import functools
import os
import re

import pytest

from kernel_build import CSRC, cross_compiled, flags, header_const, in_makefile, no_scratch_no_spills
from kernel_build import public_define as _define
from topdogspectrumanalyser_amd import correlate as co


_const = functools.partial(header_const, "tdsa_corr.hpp")
MATCH_PASSES = ("corr_bmax_kernel", "corr_count_kernel", "corr_scan_kernel", "corr_emit_kernel")
VARIANTS = ((4, 0, 0), (8, 0, 0), (16, 0, 0), (4, 1, 0), (8, 1, 0), (8, 0, 1), (8, 1, 1))   # windows per thread, packed, reference in LDS:
                                                               # the shipped one and what corrbench times


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return cross_compiled(tmp_path_factory, "tdsa_corr.hip", listing=True)


def _one(kernels, part):
    found = [k for k in kernels if part in k]
    assert len(found) == 1, (part, sorted(kernels))
    return kernels[found[0]]


def test_the_kernels_have_no_scratch_no_spills_and_stay_within_the_stated_budget(kernels):
    remarks, _ = kernels
    assert len(remarks) == len(MATCH_PASSES) + len(VARIANTS), sorted(remarks)
    simd_vgprs, simds, waves = 512, 4, _const("kCorrThreads") // 64
    assert (simd_vgprs // _const("kCorrVgprBudget")) * simds // waves == 4      # four workgroups per CU by registers
    for name in MATCH_PASSES:
        k = _one(remarks, name)
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= _const("kCorrVgprBudget"), k
        assert int(k["LDS Size [bytes/block]"]) <= _const("kCorrScanLdsBudget" if name == "corr_scan_kernel" else "kCorrMatchLdsBudget"), k
    for r, packed, rlds in VARIANTS:
        k = _one(remarks, "corr_kernelILi%dELb%dELb%dEE" % (r, packed, rlds))
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= _const("kCorrVgprBudget"), k
        budget = _const("kCorrLdsBudget") if r <= _const("kCorrWindowsPerThread") else _const("kCorrLdsBudgetWide")
        assert int(k["LDS Size [bytes/block]"]) <= budget, k
    # by LDS as many workgroups on a CU as by registers; the budget is the largest variant's figure, not just a bound
    largest = max(int(_one(remarks, "corr_kernelILi%dELb%dELb%dEE" % v)["LDS Size [bytes/block]"]) for v in VARIANTS if v[0] <= 8)
    assert _const("kCorrLdsBudget") - 2048 < largest <= _const("kCorrLdsBudget")
    assert 4 * _const("kCorrLdsBudget") <= 160 * 1024 and 2 * _const("kCorrLdsBudgetWide") <= 160 * 1024


def test_the_inner_loops_are_fused_multiply_adds_and_the_packed_variants_are_packed(kernels):
    _, asm = kernels
    bodies = {}
    for m in re.finditer(r"^(_ZN4tdsa\S*corr_kernelILi(\d+)ELb(\d)ELb(\d)EE\S*):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.S | re.M):
        bodies[(int(m.group(2)), int(m.group(3)), int(m.group(4)))] = m.group(5)
    assert sorted(bodies) == sorted(VARIANTS)
    for (r, packed, rlds), body in bodies.items():
        pk = len(re.findall(r"\bv_pk_fma_f32", body))
        scalar = len(re.findall(r"\bv_fmac?_f32", body))
        assert (pk >= 3 * r * r and scalar < pk) if packed else (pk == 0 and scalar >= 6 * r * r)
        loop = body[body.index("s_cbranch"):]                 # behind the staging
        assert rlds or re.search(r"s_load_dwordx(2|4|8|16)", loop), "the reference comes through scalar loads"


def test_the_makefile_builds_the_unit_without_contraction():
    in_makefile("corr", ["tdsa_corr.hpp", "tdsa_wave.hpp", "tdsa_unpack.hpp"], own_flags="-ffp-contract=off")
    fl = flags("tdsa_corr.hip")
    assert "-ffp-contract=off" in fl and "--offload-arch=gfx950" in fl
    assert not [f for f in fl if "flush-denormals" in f or "fast-math" in f or "denormal-fp-math" in f], fl


def test_the_source_launches_plain_kernels_and_uses_integer_atomics_only():
    src = open(os.path.join(CSRC, "tdsa_corr.hip")).read()
    code = "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("//"))
    assert code.count("hipLaunchKernelGGL(") == 5 and "extern __shared__" not in code
    for banned in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipExtLaunch", "__hip_atomic", "atomicCAS", "atomicExch",
                   "atomicMax", "atomicMin"):
        assert banned not in code, banned
    # integer atomics only: a workgroup's count of bad windows in LDS, then the stream's 64-bit counter
    adds = re.findall(r"atomicAdd\(&([\w.\[\]]+)", code)
    assert sorted(adds) == ["a.sum[c].n_bad", "l.n_bad"], adds
    assert "int n_bad;" in code and "unsigned long long n_total, n_windows, n_decided, n_matches, n_lost, n_bad;" in \
        open(os.path.join(CSRC, "tdsa_corr.hpp")).read()
    # no workgroup waits for another: no spin on memory, no ticket
    assert not re.search(r"while\s*\(.*(volatile|__atomic|atomic)", code) and "volatile" not in code


def test_the_header_budgets_what_the_python_layer_promises():
    assert _const("kCorrThreads") == 256 == _const("kCorrBlock")
    assert _const("kCorrMaxStreams") == co.MAX_STREAMS == _define("TDSA_CORR_MAX_STREAMS") == 256
    assert _const("kCorrWindowsPerThread") == co.WINDOWS_PER_THREAD == _define("TDSA_CORR_WINDOWS_PER_THREAD")
    # the two instantiations that ship are among those compiled, and the launcher names them
    assert (_const("kCorrShortWindowsPerThread"), 1, 0) in VARIANTS and (_const("kCorrWindowsPerThread"), 0, 1) in VARIANTS
    assert "a.variant ? a.variant : a.L <= kCorrShortRef ? 4 : 6" in open(os.path.join(CSRC, "tdsa_corr.hip")).read()
    assert 16 < _const("kCorrShortRef") < co.MAX_REF
    assert _const("kCorrTile") == co.TILE == _define("TDSA_CORR_TILE") == 256 * co.WINDOWS_PER_THREAD
    assert _const("kCorrMaxRecords") == co.MAX_RECORDS == _define("TDSA_CORR_MAX_RECORDS") == 1 << 22
    assert (_const("kCorrMinRef"), _const("kCorrMaxRef")) == (co.MIN_REF, co.MAX_REF) == (_define("TDSA_CORR_MIN_REF"), _define("TDSA_CORR_MAX_REF"))
    assert _const("kCorrMaxDistance") == co.MAX_DISTANCE == _define("TDSA_CORR_MAX_DISTANCE") == 65536
    assert _const("kCorrMaxLaunchTiles") == co.MAX_LAUNCH_TILES == _define("TDSA_CORR_MAX_LAUNCH_TILES") >= co.MAX_STREAMS
    assert _const("kCorrTraceBytes") == co.TRACE_BYTES == 1 << 28 and _const("kCorrRingEntryBytes") == co.RING_ENTRY_BYTES == 24
    assert _const("kCorrMaxLaunchTiles") * _const("kCorrTile") < 1 << 31       # a launch's sample indices fit an int
