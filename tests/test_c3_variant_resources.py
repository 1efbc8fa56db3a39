"""The 16384-point frame kernel with the sliding front end (tdsa_spectrum_c3_inst.hip: HOLDX bit 4 of spectrum_kernel, hold
off / max hold) is an instantiation and an object of its own, beside the frozen ones (tests/test_isa_frozen.py) and not in
their place.  CPU: hipcc cross-compiles gfx950; the compiler's own resource report and the listings are read."""
import concurrent.futures
import json
import os
import re
import shutil

import pytest

from kernel_build import CSRC, FRAME_SOURCE, HIPCC, ROOT, compile_kernels, cross_compiled, flags, makefile, no_scratch_no_spills

VARIANT_SOURCE = "tdsa_spectrum_c3_inst.hip"
VARIANTS = {hold: f"_ZN4tdsa15spectrum_kernelILi14ELb0ELi{16 | hold}ELi0EEEvNS_10SpecParamsE" for hold in (0, 1)}


@pytest.fixture(scope="module")
def variant(tmp_path_factory):
    return cross_compiled(tmp_path_factory, VARIANT_SOURCE, listing=True)


@pytest.mark.parametrize("hold", [0, 1])
def test_variant_fits_four_waves_without_scratch(variant, hold):
    """The kept raw rows and their DC sums live beside hmax[16]: no scratch, no spilled VGPR, <= 128 VGPRs, four waves."""
    reports, _ = variant
    assert sorted(reports) == sorted(VARIANTS.values()), sorted(reports)
    k = reports[VARIANTS[hold]]
    no_scratch_no_spills(k)
    assert int(k["VGPRs"]) <= 128, k
    assert int(k["Occupancy [waves/SIMD]"]) == 4, k


def test_variant_names_do_not_collide_with_the_frozen_ones():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_frozen.json")))["kernels"]
    assert len(gold) == 6 and not set(VARIANTS.values()) & set(gold)


def test_frozen_instantiations_are_still_made_by_the_size_objects(tmp_path):
    """The six frozen names are still defined in the listings of tdsa_spectrum_inst.hip (sizes 12, 13, 14), and the
    variant is not among them: it has its own object."""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_frozen.json")))["kernels"]

    def listing(k):
        out = str(tmp_path / f"inst_{k}.s")
        compile_kernels(FRAME_SOURCE, out, k)
        return open(out).read()

    with concurrent.futures.ThreadPoolExecutor(3) as ex:
        text = "\n".join(ex.map(listing, (12, 13, 14)))
    defined = set(re.findall(r"^(_ZN4tdsa15spectrum_kernel\w+):", text, re.M))
    assert set(gold) <= defined, sorted(set(gold) - defined)
    assert not set(VARIANTS.values()) & defined


def test_variant_object_is_built_like_the_size_objects():
    """csrc/Makefile links the variant's object and compiles it with the flags of tdsa_spectrum_inst.hip."""
    assert re.search(r"^OBJS\s*=.*\$\(B\)/tdsa_spectrum_c3_inst\.o\b", makefile(), re.M)
    assert flags(VARIANT_SOURCE) == flags(FRAME_SOURCE)
    assert os.path.exists(os.path.join(CSRC, VARIANT_SOURCE))

