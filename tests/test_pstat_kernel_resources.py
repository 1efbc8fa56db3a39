"""tdsa_pstat.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: pstat_kernel has
at most two instantiations, uses no scratch and spills no register, VGPRs stay within 128, and the LDS of a workgroup
stays within 40 KiB, so that four workgroups fit a CU's 160 KiB.  The Makefile builds the unit without fused
multiply-add, and the header's constants are those powerstats.py and the contract promise."""
import functools
import os

import pytest

import pstat_contract as pc
from kernel_build import CSRC, cross_compiled, flags, header_const, in_makefile, no_scratch_no_spills
from kernel_build import public_define as _define
from topdogspectrumanalyser_amd import powerstats as ps


_const = functools.partial(header_const, "tdsa_pstat.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return cross_compiled(tmp_path_factory, "tdsa_pstat.hip")


def test_pstat_kernel_has_no_scratch_no_spills_and_fits_four_workgroups_per_cu(kernels):
    found = [k for k in kernels if "pstat_kernel" in k]
    assert 1 <= len(found) <= 2 and len(kernels) == len(found), sorted(kernels)
    for name in found:
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= 128, k
        assert int(k["LDS Size [bytes/block]"]) == _const("kPstatLdsBytes") <= 40 * 1024, k      # no dynamic LDS is asked for


def test_the_makefile_builds_the_unit_without_fused_multiply_add():
    in_makefile("pstat", ["tdsa_pstat.hpp", "tdsa_unpack.hpp"], own_flags="-ffp-contract=off")
    fl = flags("tdsa_pstat.hip")
    assert "-ffp-contract=off" in fl and "--offload-arch=gfx950" in fl
    assert not [f for f in fl if "flush-denormals" in f or "fast-math" in f or "denormal-fp-math" in f], fl
    src = open(os.path.join(CSRC, "tdsa_pstat.hip")).read()
    assert "hipLaunchKernelGGL(pstat_kernel" in src and "extern __shared__" not in src
    code = [ln for ln in src.splitlines() if not ln.lstrip().startswith("//")]
    assert not [ln for ln in code if "fmaf" in ln or "__fmaf" in ln or "atomicAdd(reinterpret_cast<float" in ln]


def test_the_header_budgets_what_the_python_layer_promises():
    assert _const("kPstatThreads") == 256 and _const("kPstatMaxStreams") == ps.MAX_STREAMS == _define("TDSA_PSTAT_MAX_STREAMS")
    assert _const("kPstatBins") == ps.BINS == pc.BINS == _define("TDSA_PSTAT_BINS") == 2048
    assert _const("kPstatBinsPerOctave") == ps.BINS_PER_OCTAVE == _define("TDSA_PSTAT_BINS_PER_OCTAVE") == 32
    assert _const("kPstatOctaves") == ps.OCTAVES == 64
    assert _const("kPstatExponents") == ps.EXPONENTS == pc.EXPONENTS == _define("TDSA_PSTAT_EXPONENTS") == 256
    assert (_const("kPstatExpLoMin"), _const("kPstatExpLoMax")) == (ps.EXP_LO_MIN, ps.EXP_LO_MAX) == (-126, 64)
    assert (_define("TDSA_PSTAT_EXP_LO_MIN"), _define("TDSA_PSTAT_EXP_LO_MAX")) == (-126, 64)
    tile, launch = _const("kPstatTile"), _const("kPstatMaxLaunchSamples")
    assert tile % (8 * 256) == 0 and launch % tile == 0 and launch < 1 << 32       # 32-bit LDS counts cannot wrap in a launch
    assert _const("kPstatMaxGrid") == 2048
    assert _const("kPstatLdsBytes") == 4 * ps.BINS + 8 * ps.EXPONENTS + 4 * 256 + 32
