"""The instruction streams of the frame kernel's BASELINE instantiations are frozen (round-3 / round-4 verdicts: the C3
kernel sits at 75 % of a proven VALU-issue floor, every re-ordering measured within +-5 %; "do not touch the C3 / C2 / C4
instantiations").  This test recompiles the three sizes (hipcc cross-compiles gfx950 on a CPU-only box) and compares the
opcode sequence of spectrum_kernel<12 | 13 | 14, bytes, hold off | max hold> with the fingerprints committed in
tests/golden/isa_frozen.json (tools/isa_hash.py: mnemonics only - registers, kernarg offsets and labels may move).
A change that is meant regenerates the fingerprints AND brings its own same-box A/B (profiles/)."""
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from kernel_build import CSRC, FRAME_SOURCE, HIPCC, ROOT, compile_kernels

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _listing(log2n, tmp):
    out = os.path.join(tmp, f"inst_{log2n}.s")
    compile_kernels(FRAME_SOURCE, out, log2n)
    return out


def test_baseline_instantiations_keep_their_instruction_stream(tmp_path):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    import isa_hash
    record = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_frozen.json")))
    ver = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    hip = re.search(r"HIP version:\s*(\S+)", ver)
    if not hip or hip.group(1) != record["compiler"]["hip_version"]:
        pytest.skip(f"fingerprints are those of hipcc {record['compiler']['hip_version']}; this is "
                    f"{hip.group(1) if hip else 'unknown'}: another compiler's instruction selection is not a changed kernel")
    gold = record["kernels"]
    assert len(gold) == 6
    with concurrent.futures.ThreadPoolExecutor(3) as ex:
        listings = list(ex.map(lambda k: _listing(k, str(tmp_path)), (12, 13, 14)))
    seen = {}
    for path in listings:
        for name, ops in isa_hash.kernels(path).items():
            if name in gold:
                n, h = isa_hash.fingerprint(ops)
                seen[name] = {"instructions": n, "sha256_16": h}
    assert seen == gold, {k: (seen.get(k), gold[k]) for k in gold if seen.get(k) != gold[k]}


# Lines outside tdsa_wave.hpp that may still say __shfl_xor: file -> (lines, why they are not a call of the header).  Each
# was tried through the header; "stream" = the kernel's instruction stream changed (profiles/wave_refactor_isa.txt).
SHUFFLES_LEFT = {
    "tdsa_analytics.hip": (6, "four loops that fold several values with different ops in one butterfly, one of them "
                              "inside a scan's loop: stream"),
    "tdsa_zerospan.hip": (3, "MinMax::wave_fold folds min, max and the NaN flag in one butterfly: stream"),
    "tdsa_demod.hip": (6, "the FIR's (x, y) pairs and the five statistics fold side by side: stream"),
    "tdsa_ddc.hip": (2, "the FIR's (x, y) pairs fold side by side: stream"),
    "tdsa_detect.hip": (6, "peak + power + moment, and the two edges, fold side by side: stream"),
    "tdsa_history.hip": (2, "hist_reduce_kernel's group width G is a run-time value"),
    "tdsa_trace.hip": (1, "I and Q of a frame fold side by side: stream"),
    "tdsa_big.hip": (1, "I and Q of a frame fold side by side: stream"),
    "tdsa_chirp.hip": (2, "I and Q of a frame fold side by side, twice: stream"),
    "tdsa_smooth.hip": (1, "I and Q of a frame fold side by side: stream"),
    "tdsa_spectrum_passes.inc": (3, "one step at distance 32, the other half-thread: no butterfly"),
}


def test_lane_level_idioms_are_written_once():
    """The DPP builtin and the IEEE-order float atomics exist in tdsa_wave.hpp alone, and a shuffle butterfly outside it
    only where SHUFFLES_LEFT says why."""
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".hpp", ".inc", ".cpp")):
            continue
        lines = [ln for ln in open(os.path.join(CSRC, f)).read().splitlines() if not ln.lstrip().startswith("//")]
        if f != "tdsa_wave.hpp":
            assert not [ln for ln in lines if "__builtin_amdgcn_update_dpp" in ln], f
            assert not [ln for ln in lines if "atomicMax(reinterpret_cast<int*>" in ln], f
            n = sum("__shfl_xor" in ln for ln in lines)
            if n:
                found[f] = n
    assert found == {f: n for f, (n, why) in SHUFFLES_LEFT.items()}, found
    wave = open(os.path.join(CSRC, "tdsa_wave.hpp")).read()
    assert "__builtin_amdgcn_update_dpp" in wave and wave.count("atomicMax(reinterpret_cast<int*>") == 1
    assert re.search(r"^HDRS\s*=.*\btdsa_wave\.hpp\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)


def test_no_developer_switch_is_left_in_the_shipped_kernels():
    """Round-4 verdict item 5: the ablation / experiment switches are gone from the shipped sources, what is left of the
    developer builds sits behind TDSA_DEV, and the library reads nothing from the environment."""
    for f in os.listdir(CSRC):
        if not f.endswith((".hip", ".hpp", ".cpp")):
            continue
        src = open(os.path.join(CSRC, f)).read()
        for tok in ("TDSA_ABLATE", "TDSA_EXP_", "TDSA_DIF", "TDSA_UNFUSED", "TDSA_NO_INL", "TDSA_STAGGER", "TDSA_EXACT_MASK",
                    "TDSA_AVG_OLD", "TDSA_BIG_ROWS_OLD", "TDSA_COLS_", "getenv"):
            hits = [ln for ln in src.splitlines() if tok in ln and not ln.lstrip().startswith("//")]
            assert not hits, (f, tok, hits[:3])
