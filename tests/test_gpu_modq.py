"""The modulation quality stage on the device (tdsa_modq_*) against tests/modq_contract.py on the
same symbols: the record, the indices and the error vectors bit for bit (phase_sumsq within the arctangent's bound), the
same bits across n_seg, the segment's place and the entry point, in place behind the symbol recovery, past 2^32 bytes,
and every argument error of a live handle with its text."""
import ctypes as C

import numpy as np
import pytest

import modq_contract as mc
import symsync_contract as sc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer, _native as nat
from topdogspectrumanalyser_amd import modquality as mq
from topdogspectrumanalyser_amd import symbols as sy

pytestmark = pytest.mark.gpu

KS = (2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 4095, 4096)


@pytest.fixture(scope="module")
def handles():
    """ModQuality handles by table, made once."""
    made = {}

    def get(mod=None, points=None):
        key = mod if mod else np.asarray(points).tobytes()
        if key not in made:
            made[key] = mq.ModQuality(mod, points)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def noisy(rng, tab, n, gain=0.8 - 0.3j, offset=0.04 - 0.02j, noise=0.03):
    """n random points of the table through a gain and an offset, plus noise, as complex64."""
    i = rng.integers(0, tab.shape[0], n)
    y = gain * (tab[i, 0] + 1j * tab[i, 1]) + offset + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return y.astype(np.complex64)


def layouts(K):
    """(n_seg, in_stride): one segment; two with the stride above K; three back to back; three that overlap by one; 257
    one symbol apart."""
    return [(1, K), (2, K + 3), (3, K), (3, max(1, K - 1)), (257, 1)]


def check_call(r, y, K, in_stride, n_seg, tab, segs, what):
    """The segments `segs` of a host call's result against the contract; the gaps of a wider stride keep the sentinels."""
    assert r.indices.shape == r.errors.shape and r.indices.shape[0] == n_seg
    assert np.all(r.indices[:, K:] == mq.SENTINEL_INDEX) and np.all(r.errors[:, K:] == mq.SENTINEL), what
    for g in segs:
        want = mc.analyse(y[g * in_stride:g * in_stride + K], tab)
        mc.compare(r.records[g], r.indices[g, :K], r.errors[g, :K], want, (what, g))


# ---- every shape, stride and named table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_shapes_strides_and_named_tables_give_the_contracts_bits(handles, K):
    """Random points plus noise at every K, n_seg in {1, 2, 3, 257}, in_stride in {1, K - 1, K, K + 3}, out_stride in
    {K, K + 5}, the five named tables in turn; a segment alone gives the bits it has among the others, and the device
    entry point the host's."""
    rng = np.random.default_rng(K)
    for n, (n_seg, in_stride) in enumerate(layouts(K)):
        mod = mc.MODULATIONS[(n + K) % 5]
        tab, h = mc.table(mod), handles(mod)
        y = noisy(rng, tab, (n_seg - 1) * in_stride + K)
        stride = K + 5 if n % 2 else K
        r = h.process(y, K, in_stride, errors=True, out_stride=stride)
        segs = sorted({0, 1, n_seg // 2, n_seg - 1} & set(range(n_seg)))
        check_call(r, y, K, in_stride, n_seg, tab, segs, (mod, K, n_seg, in_stride, stride))
        g = segs[-1]
        one = h.process(y[g * in_stride:g * in_stride + K], errors=True)
        assert one.records[0].tobytes() == r.records[g].tobytes() and one.indices[0].tobytes() == r.indices[g, :K].tobytes()
        assert one.errors[0].tobytes() == r.errors[g, :K].tobytes()
        if n in (1, 4):
            with DeviceBuffer.of(y) as d_y, DeviceBuffer(n_seg * stride) as d_i, DeviceBuffer(8 * n_seg * stride) as d_e:
                d_i.put(np.full(n_seg * stride, mq.SENTINEL_INDEX, dtype=np.uint8))
                d_e.put(np.full(n_seg * stride, mq.SENTINEL, dtype=np.complex64))
                dev = h.process_device(None, d_y.ptr, K, in_stride, n_seg, d_i.ptr, stride, d_e.ptr)
                idx, err = d_i.get((n_seg, stride), np.uint8), d_e.get((n_seg, stride), np.complex64)
                none = h.process_device(None, d_y.ptr, K, in_stride, n_seg, d_i.ptr, stride)        # without error vectors
            assert dev.records.tobytes() == r.records.tobytes() == none.records.tobytes() and dev.indices is None
            assert idx.tobytes() == r.indices.tobytes() and err.tobytes() == r.errors.tobytes()


@pytest.mark.parametrize("T", (1, 2, 63, 64))
def test_tables_of_the_callers(handles, T):
    rng = np.random.default_rng(100 + T)
    tab = (rng.standard_normal((T, 2)) + 0.2).astype(np.float32)
    h = handles(points=tab)
    for K in (3, 257, 1000):
        y = noisy(rng, tab, 2 * K + 3)
        check_call(h.process(y, K, K + 3, errors=True, out_stride=K + 5), y, K, K + 3, 2, tab, (0, 1), (T, K))
    if T == 1:
        r = h.process(noisy(rng, tab, 50), errors=True)
        assert r.flags[0] == mq.ONE_POINT and not r.indices.any()


def test_a_duplicated_point_decides_for_its_lowest_index_and_8psk_as_a_table_of_the_callers(handles):
    rng = np.random.default_rng(7)
    dup = np.array([[1, 0], [0, 1], [1, 0], [0, -1], [-1, 0], [0, 1]], dtype=np.float32)
    y = noisy(rng, dup, 600, gain=1.1 + 0.1j)
    r = handles(points=dup).process(y, 300, errors=True)
    check_call(r, y, 300, 300, 2, dup, (0, 1), "duplicated")
    assert set(np.unique(r.indices)) == {0, 1, 3, 4}
    psk = mc.table("8psk")
    y = noisy(rng, psk, 513)
    own, named = handles(points=psk).process(y, errors=True), handles("8psk").process(y, errors=True)
    check_call(own, y, 513, 513, 1, psk, (0,), "8psk")
    assert own.records.tobytes() == named.records.tobytes() and own.indices.tobytes() == named.indices.tobytes()


# ---- exact and edge inputs ---------------------------------------------------------------------------------------------------
def test_an_exact_grid_returns_gain_offset_indices_and_a_zero_error_exactly(handles):
    tab = np.array([[-1, -1], [-1, 1], [1, -1], [1, 1]], dtype=np.float32)
    h = handles(points=tab)
    for K, e in ((4, 0), (100, -2), (1024, 3), (4096, -7)):
        i = np.random.default_rng(K).permutation(np.repeat(np.arange(4), K // 4))
        y = (2.0 ** e * (tab[i, 0] + 1j * tab[i, 1]) + (0.5 - 0.125j)).astype(np.complex64)
        r = h.process(y, errors=True)
        rec = r.records[0]
        assert (rec["a_re"], rec["a_im"], rec["c_re"], rec["c_im"]) == (2.0 ** e, 0.0, 0.5, -0.125), (K, rec)
        assert np.array_equal(r.indices[0], i) and rec["err_sumsq"] == 0 and rec["err_peak"] == 0 and rec["err_peak_k"] == 0
        assert rec["mag_sumsq"] == 0 and rec["phase_sumsq"] == 0 and rec["ref_sumsq"] == 2.0 * K and rec["changed"] == 0
        assert rec["flags"] == 0 and not r.errors.any() and r.evm_rms[0] == 0 and r.gain[0] == 2.0 ** e


def test_symbols_within_an_ulp_of_a_decision_boundary(handles):
    """qpsk, the symbols on a 2^-20 grid and every one with its negative beside it, so that S_y = 0 and round 1 decides with
    c = 0 exactly: a fifth of the symbols sit on an axis of the normalised plane, at the origin or an ulp beside them,
    where two or four points are equally near and the lowest index wins."""
    rng = np.random.default_rng(3)
    tab, h = mc.table("qpsk"), handles("qpsk")
    for K in (64, 512, 4096):
        z = noisy(rng, tab, K // 2, gain=1.0, offset=0.0, noise=0.05).astype(np.complex128)
        z = np.round(z * 2.0 ** 20) / 2.0 ** 20
        k = np.arange(0, K // 2, 5)
        keep = rng.integers(0, 2, (k.size, 2))
        tiny = 2.0 ** -24 * rng.integers(-2, 3, (k.size, 2))
        z[k] = (z[k].real * keep[:, 0] + tiny[:, 0]) + 1j * (z[k].imag * keep[:, 1] + tiny[:, 1])
        y = rng.permutation(np.concatenate([z, -z])).astype(np.complex64)
        r = h.process(y, errors=True)
        assert r.records["s_y"][0].tolist() == [0.0, 0.0]
        check_call(r, y, K, K, 1, tab, (0,), ("boundary", K))
        w = mc.normalise(y, (0, 0), mc.inverse(mc.analyse(y, tab)["deciders"][0][0]))
        assert np.count_nonzero((w[0] == 0) | (w[1] == 0)) >= K // 32          # ties there are


def test_one_point_degenerate_and_denormal_segments(handles):
    tab, h = mc.table("16qam"), handles("16qam")
    rng = np.random.default_rng(4)
    twice = np.array([[0.6, 0.8], [0.6, 0.8]], dtype=np.float32)
    y = noisy(rng, twice, 257)
    r = handles(points=twice).process(y, errors=True)
    check_call(r, y, 257, 257, 1, twice, (0,), "one point")
    assert r.flags[0] == mq.ONE_POINT and r.changed[0] == 0 and not r.indices.any()
    for y in (np.zeros(300, np.complex64), np.full(300, 0.25 - 2j, np.complex64)):
        r = h.process(y, errors=True)
        check_call(r, y, 300, 300, 1, tab, (0,), "degenerate")
        assert r.flags[0] == mq.DEGENERATE and not r.indices.any() and r.gain[0] == 0 and r.evm_rms[0] == 0
        assert r.records["c_re"][0] == y[0].real and r.records["c_im"][0] == y[0].imag and not r.errors.any()
    small = noisy(rng, tab, 513)
    for scale in (1e-20, 1e-22, 1e-38, 1e-41, 1e-44):          # v a float32 denormal; then the symbols themselves
        y = (small.astype(np.complex128) * scale).astype(np.complex64)
        r = h.process(y, errors=True)
        check_call(r, y, 513, 513, 1, tab, (0,), ("denormal", scale))


@pytest.mark.parametrize("bad", [complex(np.nan, 0), complex(0, np.inf), complex(3e30, -3e30)])
def test_a_non_finite_segment_is_flagged_and_its_neighbours_keep_their_bits(handles, bad):
    """A NaN and an infinity flag their segment (zero indices, NaN error vectors, a zero record); a symbol whose |y|^2
    overflows float32 does not - its sums are finite in float64 - and what the contract's operations make of it is what
    the device returns.  The segments beside it keep their bits."""
    tab, h = mc.table("qpsk"), handles("qpsk")
    K = 257
    y = noisy(np.random.default_rng(6), tab, 3 * K)
    clean = h.process(y, K, errors=True)
    for at in (K, K + 100, 2 * K - 1):
        z = y.copy()
        z[at] = np.complex64(bad)
        r = h.process(z, K, errors=True, out_stride=K + 5)
        check_call(r, z, K, K, 3, tab, (0, 1, 2), (bad, at))
        for g in (0, 2):
            assert r.records[g].tobytes() == clean.records[g].tobytes() and r.indices[g, :K].tobytes() == clean.indices[g].tobytes()
        if not np.isfinite(bad):
            assert r.flags.tolist() == [0, mq.NONFINITE, 0] and not r.indices[1, :K].any() and np.all(np.isnan(r.errors[1, :K].real))
            zero = np.zeros(1, dtype=mq.RECORD)
            zero["flags"] = mq.NONFINITE
            assert r.records[1].tobytes() == zero[0].tobytes()
        else:
            assert not r.flags[1] & mq.NONFINITE


# ---- in place behind the symbol recovery -----------------------------------------------------------------------------------
def test_in_place_behind_the_symbol_recovery_on_a_down_converter_stream(handles):
    """capture -> DownConverter(D = 2, RRC taps) -> SymbolSync -> ModQuality on the engine's stream, every stage reading
    the one before in HBM; against the contract on the device's own symbols."""
    from topdogspectrumanalyser_amd import DownConverter, SpectrumEngine
    sps, L, D, mod = 4, 1023, 2, "16qam"
    x, _, _ = sc.make_signal(mod, sps * D, 2 * (3 * L + 40), seed=9, alpha=0.35)
    x = x.astype(np.complex64)
    taps = sy.rrc_taps(sps * D, 0.35, 4)
    tab, h = mc.table(mod), handles(mod)
    with SpectrumEngine(64) as eng, DownConverter(D, 1.0, taps=taps) as ddc, sy.SymbolSync(sps, mod) as s:
        K, n_seg, stride = s.symbols_per_segment(L), 3, s.symbols_per_segment(L) + 5
        with DeviceBuffer.of(x) as d_x, DeviceBuffer(8 * (x.size // D + 8)) as d_y, DeviceBuffer(8 * n_seg * stride) as d_s, \
                DeviceBuffer(n_seg * stride) as d_i, DeviceBuffer(8 * n_seg * stride) as d_e:
            d_i.put(np.full(n_seg * stride, mq.SENTINEL_INDEX, dtype=np.uint8))
            ny = ddc.process_device(eng, nat.IN_C64, d_x.ptr, x.size, d_y.ptr)
            assert ny >= n_seg * L
            s.process_device(eng, d_y.ptr, L, L, n_seg, d_s.ptr, stride)
            r = h.process_device(eng, d_s.ptr, K, stride, n_seg, d_i.ptr, stride, d_e.ptr)
            sym = d_s.get((n_seg, stride), np.complex64)
            idx, err = d_i.get((n_seg, stride), np.uint8), d_e.get((n_seg, stride), np.complex64)
    assert np.all(idx[:, K:] == mq.SENTINEL_INDEX)
    for g in range(n_seg):
        mc.compare(r.records[g], idx[g, :K], err[g, :K], mc.analyse(sym[g, :K], tab), ("in place", g))
    print(f"16qam behind the down-converter: evm_rms {r.evm_rms}, changed {r.changed}")
    assert not r.flags.any()


def test_second_row_past_4_gib(handles):
    """Two rows, the second 2^29 + 1 symbols on: past 2^32 bytes, its error vectors past 2^32 bytes as well.  Only the
    two rows are uploaded."""
    K, stride = 1025, (1 << 29) + 1
    tab, h = mc.table("64qam"), handles("64qam")
    rows = [noisy(np.random.default_rng(30 + g), tab, K) for g in range(2)]
    with room_or_skip((stride + K) * 8) as d_y, room_or_skip((stride + K) * 8) as d_e, room_or_skip(stride + K) as d_i:
        d_y.put(rows[0])
        d_y.put(rows[1], stride * 8)
        dev = h.process_device(None, d_y.ptr, K, stride, 2, d_i.ptr, stride, d_e.ptr)
        idx = [d_i.get((K,), np.uint8, g * stride) for g in range(2)]
        err = [d_e.get((K,), np.complex64, g * stride * 8) for g in range(2)]
    for g in range(2):
        one = h.process(rows[g], errors=True)
        assert dev.records[g].tobytes() == one.records[0].tobytes(), g
        assert idx[g].tobytes() == one.indices[0].tobytes() and err[g].tobytes() == one.errors[0].tobytes(), g
    assert idx[0].tobytes() != idx[1].tobytes()


# ---- argument errors of a live handle --------------------------------------------------------------------------------------
def test_every_argument_error_of_a_live_handle_with_its_text():
    lib, P = nat.lib, C.c_void_p

    def says(rc, text):
        assert rc == -1 and lib.tdsa_last_error_string().decode() == text, lib.tdsa_last_error_string()

    raw = C.c_void_p()
    nat.check(lib.tdsa_modq_create(0, 64, C.byref(raw)))
    host = (C.c_ubyte * 4096)()
    rec = np.zeros(4, dtype=mq.RECORD)
    pr = rec.ctypes.data
    try:
        with DeviceBuffer(4096) as d:
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 1, host, 8, None, P(pr)), "no reference points: call tdsa_modq_set_points first")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr), 8, None, P(pr)),
                 "no reference points: call tdsa_modq_set_points first")
            pts = (C.c_float * 8)(1, 1, 1, -1, -1, 1, -1, -1)
            assert lib.tdsa_modq_set_points(raw, pts, 4) == 0
            says(lib.tdsa_modq_set_points(raw, pts, 0), "n_points=0: 1 .. 64 reference points")
            says(lib.tdsa_modq_process(raw, None, 64, 8, 8, 1, host, 8, None, P(pr)), "null symbols")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 1, None, 8, None, P(pr)), "null indices")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 1, host, 8, None, None), "null records")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 1, host, 8, None, P(pr + 4)), "records must be aligned to 8 bytes")
            says(lib.tdsa_modq_process(raw, host, 64, 1, 8, 1, host, 8, None, P(pr)), "K=1: 2 .. 4096 symbols per segment")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 0, 1, host, 8, None, P(pr)), "in_stride=0: at least one symbol")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 0, host, 8, None, P(pr)), "n_seg=0: at least one segment")
            says(lib.tdsa_modq_process(raw, host, 64, 8, 8, 1, host, 7, None, P(pr)), "out_stride=7: a segment gives 8 symbols")
            says(lib.tdsa_modq_process(raw, host, 7, 8, 8, 1, host, 8, None, P(pr)),
                 "1 segments of 8 symbols every 8 need 8 symbols, the block has 7")
            says(lib.tdsa_modq_process(raw, host, 23, 8, 8, 3, host, 8, None, P(pr)),
                 "3 segments of 8 symbols every 8 need 24 symbols, the block has 23")
            says(lib.tdsa_modq_process(raw, host, 65, 8, 8, 3, host, 8, None, P(pr)),
                 "block of 65 symbols, the handle stages at most 64 (max_host_symbols)")
            says(lib.tdsa_modq_process_dev(raw, None, None, 8, 8, 1, P(d.ptr), 8, None, P(pr)), "null symbols")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, None, 8, None, P(pr)), "null indices")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 8, None, None), "null records")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr + 4), 8, 8, 1, P(d.ptr + 1024), 8, None, P(pr)),
                 "symbols pointer must be aligned to one complex64 symbol (8 bytes)")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 8, P(d.ptr + 2052), P(pr)),
                 "errors pointer must be aligned to one complex64 error vector (8 bytes)")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 8, None, P(pr + 4)),
                 "records must be aligned to 8 bytes")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 4097, 8, 1, P(d.ptr + 1024), 4097, None, P(pr)),
                 "K=4097: 2 .. 4096 symbols per segment")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 0, 1, P(d.ptr + 1024), 8, None, P(pr)), "in_stride=0: at least one symbol")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 0, P(d.ptr + 1024), 8, None, P(pr)), "n_seg=0: at least one segment")
            says(lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 7, None, P(pr)),
                 "out_stride=7: a segment gives 8 symbols")
            n_dev = C.c_int()
            assert lib.tdsa_device_count(C.byref(n_dev)) == 0
            if n_dev.value > 1:                                                                # a plan on another device
                from topdogspectrumanalyser_amd import SpectrumEngine
                with SpectrumEngine(64, device=1) as eng:
                    says(lib.tdsa_modq_process_dev(raw, eng._h, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 8, None, P(pr)),
                         "plan and modulation quality handle live on different devices")
            says(lib.tdsa_modq_timer_end(raw, None), "null elapsed_ms")
            # and after all of them the handle works
            d.put(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j] * 2, dtype=np.complex64))
            assert lib.tdsa_modq_process_dev(raw, None, P(d.ptr), 8, 8, 1, P(d.ptr + 1024), 8, None, P(pr)) == 0
            assert (rec["a_re"][0], rec["c_re"][0], rec["err_sumsq"][0], rec["flags"][0]) == (1.0, 0.0, 0.0, 0)
            assert d.get((8,), np.uint8, 1024).tolist() == [0, 1, 2, 3] * 2
    finally:
        lib.tdsa_modq_destroy(raw)


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", ("qpsk", "16qam"))
def test_evm_of_a_burst_through_the_chain_matches_the_contracts(handles, mod):
    """A burst through DownConverter (RRC) -> SymbolSync -> ModQuality on the device against the float64 contract of the
    symbol recovery followed by this stage's contract, both fed the down-converter's output: evm_rms within 1 %.
    Measured on the device: a ratio of 1.00000 for both (evm_rms 0.10379 for qpsk, 0.09933 for 16qam)."""
    from topdogspectrumanalyser_amd import DownConverter
    sps, L, D = 4, 4100, 2
    x, _, _ = sc.make_signal(mod, sps * D, 2 * (L + 80), seed=12, alpha=0.35, noise_db=-30.0)
    taps = sy.rrc_taps(sps * D, 0.35, 4)
    with DownConverter(D, 1.0, taps=taps) as ddc, sy.SymbolSync(sps, mod) as s:
        y = ddc.process(x.astype(np.complex64))[40:40 + L]
        sym = s.process(y, L)
        assert not sym.flags.any()
        r = handles(mod).process(sym.symbols[0])
    M = sc.ORDER[mod]
    ref = sc.recover(y.astype(np.complex128), sps, M, sc.reference_phase(sc.points(mod), M))
    want = mc.analyse(ref["symbols"].astype(np.complex64), mc.table(mod))
    ratio = float(r.evm_rms[0]) / mc.evm_rms(want)
    print(f"{mod}: evm_rms on the device {float(r.evm_rms[0]):.5f}, the contract's {mc.evm_rms(want):.5f}, ratio {ratio:.5f}, "
          f"changed {int(r.changed[0])}, mer {float(r.mer_db[0]):.2f} dB")
    assert r.flags[0] == 0 and abs(ratio - 1.0) <= 0.01
