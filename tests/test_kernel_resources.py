"""Register / scratch budget of the frame kernel's hot instantiations (CPU: hipcc cross-compiles gfx950).

Round-2 verdict item 4: `spectrum_kernel<14, false, 1, false>` (C3: int8 frames, max hold) carried one spilled
VGPR - 8 bytes of scratch per lane, 2.1 MB of spill writes per launch.  Round-3 verdict item 4: the max + min hold
instantiations of five sizes carried 8 - 84 bytes.  Every instantiation of every size must be free of scratch at the
occupancy it is launched for; this test recompiles the nine sizes with -Rpass-analysis=kernel-resource-usage and reads
the compiler's own report.  The long-frame kernels (column pass, row pass) are checked from tdsa_big.hip.
"""
import concurrent.futures
import os
import shutil

import pytest

from kernel_build import FRAME_SIZES as SIZES, FRAME_SOURCE, HIPCC, compile_kernels, no_scratch_no_spills


def _report(log2n, tmp):
    return compile_kernels(FRAME_SOURCE, os.path.join(tmp, f"spec_{log2n}.o"), log2n)



@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    tmp = str(tmp_path_factory.mktemp("kres"))
    with concurrent.futures.ThreadPoolExecutor(min(len(SIZES), os.cpu_count() or 1)) as ex:
        return dict(zip(SIZES, ex.map(lambda k: _report(k, tmp), SIZES)))


def _kernel(reports, log2n, in_c64, hold, chirp=0):
    name = f"_ZN4tdsa15spectrum_kernelILi{log2n}ELb{int(in_c64)}ELi{hold}ELi{chirp}EEEvNS_10SpecParamsE"
    assert name in reports[log2n], sorted(reports[log2n])
    return reports[log2n][name]


@pytest.mark.parametrize("log2n", SIZES)
@pytest.mark.parametrize("in_c64", [False, True])
@pytest.mark.parametrize("hold", [0, 1, 2, 3, 4])
def test_every_instantiation_is_free_of_scratch(reports, log2n, in_c64, hold):
    """All nine sizes x both input formats x hold off / max / min / max + min (an ordinary GUI state of the reference,
    core/display_data_processor.py:371-395) / 4 = the averager's chunk aggregates (utils/signal_processing.py:35-61): no scratch, no spilled VGPR, and the register count of the occupancy the
    instantiation is launched for (round-3 verdict: five max + min instantiations carried 8 - 84 bytes of scratch per
    lane, and a spilled value is reloaded behind the row stores' vmcnt)."""
    k = _kernel(reports, log2n, in_c64, hold)
    waves = 4                                              # every instantiation is launched for four waves per SIMD
    assert int(k["ScratchSize [bytes/lane]"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= (512 // waves) // 8 * 8, k
    assert int(k["Occupancy [waves/SIMD]"]) >= waves, k


@pytest.mark.parametrize("log2n", [10, 11, 12, 13, 14])
@pytest.mark.parametrize("in_c64", [False, True])
@pytest.mark.parametrize("hold", [8, 9])
def test_frame_statistics_instantiations_are_free_of_scratch(reports, log2n, in_c64, hold):
    """HOLD | 8 = the STATS epilogue (per-frame peak / argmax / band power from the bins in registers; hold none / max, frames
    of whole waves): no scratch and no spilled VGPR in any of them - in the C3-shaped one (16384 points, bytes, max hold) a
    single spilled trace register is reloaded behind vmcnt(0) every frame (three variants of the epilogue did that) - and no
    spilled SGPR in the byte-format ones of the BASELINE sizes."""
    k = _kernel(reports, log2n, in_c64, hold)
    assert int(k["ScratchSize [bytes/lane]"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k
    if not in_c64 and log2n >= 12:                         # the BASELINE shapes (C2 / C4 / C3)
        assert int(k["SGPRs Spill"]) == 0, k


@pytest.mark.parametrize("log2n", [10, 11, 12, 13, 14])
@pytest.mark.parametrize("chirp", [3])
def test_chirp_transform_instantiations_are_free_of_scratch(reports, log2n, chirp):
    """The instantiation that carries a chirp-z plan's element-wise passes (tdsa_chirp.hip; complex64 in, no hold,
    M = 1024 ... 16384): 3 = the whole convolution of a frame in one pass through its workgroup (1 / 2 = its two transforms
    as two launches: developer builds only, -DTDSA_DEV).  No scratch at four waves per SIMD - as run-time branches of the
    plain complex64 kernel the same code spilled 68 - 98 registers.  One exception, stated: the one-launch instantiation at
    16384 points (1024 threads, 136 KB of LDS: no room for a twiddle table, no fifth wave) keeps 7 dwords in scratch; it
    still beats its two-launch alternative by 26 % (profiles/r05_chirp.txt).  The shipped library holds no two-launch
    instantiation."""
    assert not any("ELi0ELi1EEEv" in n or "ELi0ELi2EEEv" in n for n in reports[log2n]), "two-launch chirp kernels in the shipped build"
    k = _kernel(reports, log2n, True, 0, chirp)
    allowed = 32 if (log2n, chirp) == (14, 3) else 0
    assert int(k["ScratchSize [bytes/lane]"]) <= allowed and int(k["VGPRs Spill"]) <= allowed // 4, k
    assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k


def test_long_chirp_row_pass_instantiation_is_free_of_scratch(reports):
    """spectrum_kernel<14, true, 0, 4>: the row passes of a long chirp-z frame's two transforms in one kernel."""
    k = _kernel(reports, 14, True, 0, 4)
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["VGPRs Spill"]) == 0, k
    assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4, k


def test_mixed_radix_kernel_is_free_of_scratch(tmp_path):
    """tdsa_smooth.hip (frame lengths 2^a 3^b 5^c): three instantiations of one kernel, no scratch, <= 64 VGPRs."""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    reps = compile_kernels("tdsa_smooth.hip", str(tmp_path / "s.o"))
    # one pass in LDS (frames up to 10 000 points), column pass and row pass of the two-pass transform above
    assert sorted(reps) == [f"_ZN4tdsa13smooth_kernelILi{k}EEEvNS_12SmoothParamsE" for k in (0, 1, 2)], reps
    for rep in reps.values():
        assert int(rep["ScratchSize [bytes/lane]"]) == 0 and int(rep["VGPRs Spill"]) == 0 and int(rep["VGPRs"]) <= 64, rep


def test_byte_input_hot_instantiations_keep_four_waves(reports):
    """C2 (4096), C4 (8192), C3 (16384): int8 / uint8 frames, no hold / max hold - the BASELINE shapes - at <= 128 VGPRs."""
    for log2n in (12, 13, 14):
        for hold in (0, 1):
            k = _kernel(reports, log2n, False, hold)
            assert int(k["VGPRs"]) <= 128 and int(k["Occupancy [waves/SIMD]"]) >= 4 and int(k["SGPRs Spill"]) == 0, k


def test_long_frame_column_pass_keeps_three_waves_and_no_vmem_wait_between_its_stores(tmp_path):
    """Column pass of the 2^20-point chain (C5): 64 complex points per thread must stay at <= 168 VGPRs (3 waves per
    SIMD) without scratch, and its store loop must not contain a vector-memory load: gfx9 counts loads and stores in one
    in-order vmcnt, so a table load between the row stores waits for every store before it (round 3: 154 -> 116 us)."""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    asm = str(tmp_path / "big.s")
    reports = compile_kernels("tdsa_big.hip", asm)

    def body_of(name):
        body, on = [], False
        for ln in open(asm):
            if ln.startswith(name + ":"):
                on = True
            elif on and ln.startswith(".Lfunc_end"):
                break
            elif on:
                body.append(ln.split(";")[0].strip())
        return body

    # four instantiations per size: the window from a table / one value for every sample, with / without DC removal
    for flat in (0, 1):
        for dc in (0, 1):
            name = f"_ZN4tdsa15big_cols_kernelILi6ELb{flat}ELb{dc}ELb0EEEvNS_13BigColsParamsE"
            rep = reports[name]
            no_scratch_no_spills(rep)
            assert int(rep["VGPRs"]) <= 168 and int(rep["Occupancy [waves/SIMD]"]) >= 3, rep
            body = [ln for ln in body_of(name) if ln]
            stores = [i for i, ln in enumerate(body) if ln.startswith("buffer_store_dwordx4")]
            assert len(stores) == 32, len(stores)
            tail = body[stores[0]:stores[-1] + 1]
            assert not any(ln.startswith(("buffer_load", "global_load", "flat_load")) for ln in tail)
            assert not any(ln.startswith("s_waitcnt") and "vmcnt" in ln for ln in tail)
            # the gfx950 store-data hazard (a > 8-byte buffer store whose data registers the next VALU instruction
            # overwrites) is pinned in the source: every 16-byte store is followed by its own wait states
            assert all(body[i + 1].startswith("s_nop 1") for i in stores), [body[i + 1] for i in stores]
            loads = sum(ln.startswith("buffer_load_dword ") for ln in body)       # the table's 4-byte window loads
            assert (loads >= 64) == (flat == 0), (flat, loads)

    # the long chirp-z frames' instantiations (raw frames in, times window x chirp; power / dB rows out): no scratch
    for name in ("_ZN4tdsa15big_cols_kernelILi6ELb1ELb0ELb1EEEvNS_13BigColsParamsE",
                 "_ZN4tdsa19big_cols_out_kernelILi6EEEvNS_16BigColsOutParamsE"):
        no_scratch_no_spills(reports[name])

    # row pass (big_rows_kernel): 128 VGPRs / 4 waves per SIMD without scratch, and the fetch of the next row spread over
    # the row's work - eight 16-byte loads, one at a time, each behind a stretch of arithmetic (bursts cost 13 %)
    name = "_ZN4tdsa15big_rows_kernelENS_13BigRowsParamsE"
    rep = reports[name]
    assert int(rep["ScratchSize [bytes/lane]"]) == 0 and int(rep["VGPRs"]) <= 128 and int(rep["Occupancy [waves/SIMD]"]) >= 4, rep
    body = body_of(name)
    barriers = [i for i, ln in enumerate(body) if ln.startswith("s_barrier")]
    loop = body[barriers[0] + 1:barriers[-1] + 1]                 # from behind the prologue's barrier to the loop's last one
    loads = [i for i, ln in enumerate(loop) if ln.startswith("buffer_load_dwordx4")]
    assert len(loads) == 8, loads
    gaps = [sum(ln.startswith("v_") for ln in loop[a:b]) for a, b in zip(loads, loads[1:])]
    assert sum(g >= 20 for g in gaps) >= 4, f"VALU instructions between consecutive loads of the row pass's loop: {gaps}"
    assert loads[-1] - loads[0] >= 0.6 * len(loop), (loads, len(loop))       # ... and they span most of the row's work
    assert not any(ln.startswith(("global_store", "buffer_store", "scratch_")) for ln in loop)
