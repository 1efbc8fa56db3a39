"""tdsa_pulse.hip cross-compiled for gfx950 (no GPU), read through the compiler's resource remarks only: the three kernels
use no scratch and spill no register, their VGPRs and LDS stay within the budget tdsa_pulse.hpp states, and the
workgroups per CU the header promises follow from them.  The Makefile builds the unit without fused multiply-add, the
header's constants are those pulses.py and include/tdsa_hip.h promise, and no kernel is launched cooperatively."""
import functools
import os
import re

import pytest

import pulse_contract as pc
from kernel_build import CSRC, cross_compiled, flags, header_const, in_makefile, no_scratch_no_spills
from kernel_build import public_define as _define
from topdogspectrumanalyser_amd import pulses as pu


_const = functools.partial(header_const, "tdsa_pulse.hpp")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return cross_compiled(tmp_path_factory, "tdsa_pulse.hip")


def test_the_kernels_have_no_scratch_no_spills_and_stay_within_the_stated_budget(kernels):
    tile = [k for k in kernels if "pulse_tile_kernelILb0" in k]
    emit = [k for k in kernels if "pulse_tile_kernelILb1" in k]
    stitch = [k for k in kernels if "pulse_stitch_kernel" in k]
    assert len(tile) == len(emit) == len(stitch) == 1 and len(kernels) == 3, sorted(kernels)
    simd_vgprs, simds, waves = 512, 4, _const("kPulseThreads") // 64
    for name, budget, per_cu in ((tile[0], "kPulseVgprBudget", "kPulseWorkgroupsPerCu"), (emit[0], "kPulseVgprBudget", "kPulseWorkgroupsPerCu"),
                                 (stitch[0], "kPulseVgprBudget", "kPulseWorkgroupsPerCu")):
        k = kernels[name]
        print(name, k)
        no_scratch_no_spills(k)
        assert int(k["VGPRs"]) <= _const(budget), k
        assert int(k["LDS Size [bytes/block]"]) <= _const("kPulseLdsBudget"), k             # no dynamic LDS is asked for
        # workgroups per CU: waves per SIMD by registers, times the SIMDs, over the waves of a workgroup; LDS allows more
        assert (simd_vgprs // _const(budget)) * simds // waves == _const(per_cu)
        assert _const(per_cu) * _const("kPulseLdsBudget") <= 160 * 1024


def test_the_makefile_builds_the_unit_without_fused_multiply_add():
    in_makefile("pulse", ["tdsa_pulse.hpp", "tdsa_wave.hpp"], own_flags="-ffp-contract=off")
    fl = flags("tdsa_pulse.hip")
    assert "-ffp-contract=off" in fl and "--offload-arch=gfx950" in fl
    assert not [f for f in fl if "flush-denormals" in f or "fast-math" in f or "denormal-fp-math" in f], fl


def test_the_source_launches_three_plain_kernels_and_uses_no_float_atomics():
    src = open(os.path.join(CSRC, "tdsa_pulse.hip")).read()
    code = "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("//"))
    assert code.count("hipLaunchKernelGGL(") == 3 and "extern __shared__" not in code
    for banned in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipExtLaunch", "__hip_atomic", "fmaf", "fma("):
        assert banned not in code, banned
    # integer atomics only: every atomicAdd adds an int or an unsigned long long counter in LDS
    assert not re.search(r"atomic(Add|Max|Min|Exch|CAS)\s*\(\s*(reinterpret_cast<\s*(float|double)|&\w+\.(energy|acc_))", code)
    adds = re.findall(r"atomicAdd\(&l\.(\w+)", code)
    assert adds and set(adds) == {"cnt"}, adds
    # no workgroup waits for another: no spin on memory, no ticket
    assert not re.search(r"while\s*\(.*(volatile|__atomic|atomic)", code) and "volatile" not in code


def test_the_header_budgets_what_the_python_layer_promises():
    assert _const("kPulseThreads") == 256 and _const("kPulseMaxStreams") == pu.MAX_STREAMS == _define("TDSA_PULSE_MAX_STREAMS") == 256
    assert _const("kPulseSamplesPerThread") == pu.SAMPLES_PER_THREAD == _define("TDSA_PULSE_SAMPLES_PER_THREAD")
    assert _const("kPulseTile") == pu.TILE == _define("TDSA_PULSE_TILE") == 256 * pu.SAMPLES_PER_THREAD
    assert _const("kPulseMaxRecords") == pu.MAX_RECORDS == _define("TDSA_PULSE_MAX_RECORDS") == 1 << 22
    assert _define("TDSA_PULSE_FLAG_INF") == pu.FLAG_INF == pc.FLAG_INF == 1
    assert _const("kPulseTile") % 8 == 0                                   # a tile keeps its stream's 16-byte alignment
    assert _const("kPulseMaxLaunchTiles") >= pu.MAX_STREAMS                # a launch takes a tile of every stream
    assert _const("kPulseMaxLaunchTiles") * _const("kPulseTile") < 1 << 31  # a launch's sample indices fit an int
