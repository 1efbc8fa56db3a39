"""The constellation pass (tdsa_constellation.hip) pinned bit for bit against tests/constellation_contract.py at every
shape where it takes another path: every partial-block tree of numpy's pairwise sum, samples placed on, beside and
outside the float64 histogram edges, reference tables of every kind through the C-ABI, the segment path at small
shapes and past 2^32 bytes, the AGC threshold and the non-finite / denormal extremes, and the C-ABI edges.  No
tolerance anywhere: rms as float32, evm as float, counts as uint32, the tail as float32 with NaN equal to NaN.  Every
input family asserts on the CPU that it discriminates."""
import ctypes as C

import numpy as np
import pytest

import constellation_contract as cc
from device_room import room_or_skip
from topdogspectrumanalyser_amd import DeviceBuffer

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]        # every test under a time limit of its own

MAX_HOST = 1 << 15
F32 = np.float32


@pytest.fixture(scope="module")
def handle():
    from topdogspectrumanalyser_amd import Constellation
    with Constellation(max_host_samples=MAX_HOST) as c:
        yield c


@pytest.fixture
def cst(handle):
    """The module's one handle, in its default state."""
    handle.set_modulation("qpsk")
    handle.set_bins(128)
    handle.set_range(1.5)
    return handle


def _nat():
    from topdogspectrumanalyser_amd import _native as nat
    return nat


def _bits(a, b, dt):
    """a and b hold the same bits as dt (so -0.0 is not 0.0), any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=dt).reshape(-1), np.asarray(b, dtype=dt).reshape(-1)
    u = np.uint32 if dt == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def _check(res, want, tag, n_tail=0):
    assert _bits(res.rms, want["rms"], np.float32), (tag, res.rms, want["rms"])
    if want["evm"] is None:
        assert res.evm_rms is None, (tag, res.evm_rms)
    else:
        assert res.evm_rms is not None and _bits(res.evm_rms, want["evm"], np.float64), (tag, res.evm_rms, want["evm"])
    assert res.counts.dtype == np.uint32 and np.array_equal(res.counts, want["counts"]), tag
    if n_tail:
        ti, tq = res.scatter()
        assert ti.size == n_tail and tq.size == n_tail, (tag, ti.size, n_tail)
        assert _bits(ti, want["i"][-n_tail:], np.float32), (tag, "tail i", n_tail)
        assert _bits(tq, want["q"][-n_tail:], np.float32), (tag, "tail q", n_tail)


def _set_pts(c, pts):
    """tdsa_constellation_set_refs with an explicit table; returns the status."""
    xy = np.ascontiguousarray(pts)
    assert xy.dtype in (np.float32, np.float64) and (xy.size == 0 or xy.shape[1] == 2)
    ptr = xy.ctypes.data_as(C.c_void_p) if xy.size else None
    return _nat().lib.tdsa_constellation_set_refs(c._h, ptr, len(xy), int(xy.dtype == np.float64))


# ---- 1. every length -------------------------------------------------------------------------------------------------

def _lengths():
    ls = set(range(1, 273))
    for b in (512, 1024, 2048, 4096, 8192, 16384):
        ls |= {b + d for d in range(-9, 10)}
    ls |= {int(n) for n in np.random.default_rng(20240).choice(np.arange(273, 8192), 96, replace=False)}
    for m in (1, 2):
        ls |= {8192 * m + r for r in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 136, 4095, 8191)}
    return sorted(ls)


LENGTHS = _lengths()
TAIL_LENGTHS = set(LENGTHS[::7]) | {1, 2, 127, 128, 129, 255, 256, 257, 2000, 2001, 8191, 8192, 8193, 16384, 24575}


def _block(n):
    """standard_normal * 0.3 seeded by n; every 50th sample or so is 10^3 larger, so the order of a sum shows."""
    rng = np.random.default_rng(n)
    iq = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    big = rng.choice(n, 1 + n // 50, replace=False)
    iq[big] *= F32(1e3)
    return iq


def test_length_sweep_discriminates():
    """Over the lengths above 128 a sequential float32 fold gives another power sum than numpy's tree for most."""
    over = [n for n in LENGTHS if n > 128]
    differ = 0
    for n in over:
        a = cc.cabs(_block(n))
        p = (a * a).astype(np.float32)
        differ += bool(cc.np_sum(p) != cc.sequential_sum(p))
    print(f"power sum: numpy's tree != sequential fold at {differ} of {len(over)} lengths above 128")
    assert 2 * differ >= len(over), (differ, len(over))


@pytest.mark.parametrize("mod", ["qpsk", "8psk", "64qam"])       # float64 grid, float32 brute force, float32 grid
def test_every_length(cst, mod):
    assert cc.reference_points(mod).dtype == (np.float64 if mod == "qpsk" else np.float32)
    cst.set_modulation(mod)
    for n in LENGTHS:
        iq = _block(n)
        want = cc.evaluate(iq, mod, 1.5)
        _check(cst.process(iq), want, (mod, n))
        if n in TAIL_LENGTHS:
            for nt in sorted({1, min(n, 2000), n}):
                _check(cst.process(iq, n_tail=nt), want, (mod, n, nt), n_tail=nt)


def test_tail_starts_inside_on_and_before_a_block(cst):
    """n = 20000 is blocks [0, 8192), [8192, 16384), [16384, 20000) and the tail starts at sample n - n_tail: 11809,
    11808 and 11807 (inside the middle block), 8192 and 16384 (exactly on a block boundary), 16383, and 0."""
    n = 20000
    iq = _block(n)
    want = cc.evaluate(iq, "qpsk", 1.5)
    for nt in (8191, 8192, 8193, 11808, 3616, 3617, 20000):
        _check(cst.process(iq, n_tail=nt), want, nt, n_tail=nt)


# ---- 2. bins and edges -----------------------------------------------------------------------------------------------

def _axis_values(r, bins):
    """float32 values on, just below and just above every float64 edge, around +-r, and the special values."""
    up, dn = F32(np.inf), F32(-np.inf)
    ef = cc.edges(r, bins).astype(np.float32)
    rf = F32(r)
    tiny = np.nextafter(F32(0), up)
    special = np.array([rf, -rf, np.nextafter(rf, up), np.nextafter(-rf, dn), 0.0, -0.0, np.inf, -np.inf, np.nan,
                        1e-40, -1e-40, tiny, -tiny, 3.4e38, -3.4e38], dtype=np.float32)
    return np.concatenate([ef, np.nextafter(ef, dn), np.nextafter(ef, up), special]).astype(np.float32)


def _few_values(r, bins):
    """A handful from the same list: both ends, the edge nearest the middle, its neighbour, zero, one just outside."""
    up = F32(np.inf)
    ef = cc.edges(r, bins).astype(np.float32)
    mid = ef[(bins + 1) // 2]
    return np.array([-F32(r), mid, np.nextafter(mid, up), -0.0, 1e-40, F32(r), np.nextafter(F32(r), up)],
                    dtype=np.float32)


@pytest.mark.parametrize("r", [0.7, 1.0, 1.5, 2.0, 1e-3, 1e3])
def test_samples_on_and_beside_every_edge(cst, r):
    """One NaN sample makes rms NaN, which switches the AGC off: the samples reach bin_of as they are placed."""
    cst.set_range(r)
    for bins in (1, 2, 3, 7, 64, 100, 127, 128):
        cst.set_bins(bins)
        full, few = _axis_values(r, bins), _few_values(r, bins)
        for transposed in (False, True):
            a, b = np.repeat(full, few.size), np.tile(few, full.size)
            i, q = (b, a) if transposed else (a, b)
            iq = np.empty(i.size, np.complex64)
            iq.real, iq.imag = i, q
            assert _bits(iq.real, i, np.float32) and _bits(iq.imag, q, np.float32)
            want = cc.evaluate(iq, "qpsk", r, bins)
            assert np.isnan(want["rms"]) and _bits(want["i"], i, np.float32) and _bits(want["q"], q, np.float32)
            inside = int(((np.abs(i.astype(np.float64)) <= r) & (np.abs(q.astype(np.float64)) <= r)).sum())
            assert 0 < inside < iq.size, (r, bins, inside, iq.size)          # the grid discriminates
            res = cst.process(iq, n_tail=iq.size)
            assert np.array_equal(res.counts, cc.histogram(i, q, r, bins)), (r, bins, transposed)
            assert int(res.counts.sum()) == inside, (r, bins, transposed, int(res.counts.sum()), inside)
            _check(res, want, (r, bins, transposed), n_tail=iq.size)


@pytest.mark.parametrize("bins", [2, 64, 128])
def test_agc_on_with_samples_exactly_on_edges(cst, bins):
    """(+-1, 0) and (0, +-1) only: rms is exactly 1, so at range 1.0 the normalised samples sit on the first edge, the
    centre edge and the last edge."""
    n = {(1, 0): 300, (-1, 0): 211, (0, 1): 127, (0, -1): 62}
    iq = np.concatenate([np.full(k, complex(*z), np.complex64) for z, k in n.items()])
    iq = iq[np.random.default_rng(5).permutation(iq.size)]
    cst.set_range(1.0)
    cst.set_bins(bins)
    want = cc.evaluate(iq, "qpsk", 1.0, bins)
    assert _bits(want["rms"], F32(1.0), np.float32)
    res = cst.process(iq, n_tail=iq.size)
    _check(res, want, bins, n_tail=iq.size)
    mid, last = bins // 2, bins - 1                      # counts[q_bin][i_bin]; 0 is the left edge of bin bins / 2
    explicit = np.zeros((bins, bins), np.uint32)
    for (qb, ib), k in zip(((mid, last), (mid, 0), (last, mid), (0, mid)), n.values()):
        explicit[qb, ib] += k
    assert np.array_equal(res.counts, explicit)


# ---- 3. tables through the C-ABI -------------------------------------------------------------------------------------

LV_X = np.array([-1.5, -1.0, -0.375, -0.125, 0.25, 0.5, 0.875, 1.375])       # uneven, multiples of 1/8
LV_Y = np.array([-1.25, -0.75, -0.5, 0.0, 0.125, 0.625, 1.0, 1.5])


def _grid(xs, ys, dt, seed=0):
    g = np.array([[x, y] for x in xs for y in ys], dtype=dt)
    return g[np.random.default_rng(seed).permutation(len(g))]          # a grid in any point order


def _tables():
    rng = np.random.default_rng(64)
    dup = _grid(LV_X[2:6], LV_Y[1:5], np.float32, 3)
    dup[11] = dup[4]                                        # 16 points, 4 x 4 levels, but not the full grid
    psk = np.array([[np.cos(a), np.sin(a)] for a in (k * np.pi / 4 for k in range(8))], dtype=np.float64)
    return {
        "grid8x8_f64": _grid(LV_X, LV_Y, np.float64, 1),
        "grid8x8_f32": _grid(LV_X, LV_Y, np.float32, 2),
        "grid2x32": _grid(np.linspace(-0.4, 0.9, 2), np.linspace(-1.5, 1.4, 32) ** 3 / 2.0, np.float32, 4),
        "grid32x2": _grid(np.linspace(-1.3, 1.5, 32), np.array([-0.3, 1.1]), np.float64, 5),
        "random64": rng.uniform(-1.5, 1.5, (64, 2)).astype(np.float32),
        "random63_f64": rng.uniform(-1.5, 1.5, (63, 2)),
        "one_point": np.array([[0.3, -0.2]], dtype=np.float32),
        "grid4x4_dup": dup,
        "8psk_f64": psk,
    }


def _exact_rms_one_block():
    """Samples exactly half-way between neighbouring levels of LV_X (as i, with q = 0) and of LV_Y (as q, with i = 0),
    each 256 times, filled up with 0 and 2 so that the mean power is exactly 1: on an axis |x| is exact, every power is
    a multiple of 2^-8 and every partial sum stays below 2^16, so all sums are exact, rms = 1 and the AGC multiplies
    by 1.  The samples reach the distance search as placed."""
    hx, hy = (LV_X[:-1] + LV_X[1:]) / 2, (LV_Y[:-1] + LV_Y[1:]) / 2
    z = np.concatenate([np.repeat(hx, 256) + 0j, 1j * np.repeat(hy, 256)])
    deficit = z.size - float(np.sum(z.real ** 2 + z.imag ** 2))         # an integer: 256 copies of multiples of 2^-8
    assert deficit == int(deficit) and deficit > 0
    twos = -(-int(deficit) // 3)                                        # a 2 adds 4 to the power and 1 to the count
    zeros = 3 * twos - int(deficit)
    z = np.concatenate([z, np.full(twos, 2 + 0j), np.zeros(zeros, complex)])
    return z[np.random.default_rng(9).permutation(z.size)].astype(np.complex64)


def _table_blocks():
    rng = np.random.default_rng(33)
    n = 8192 + 777                                          # a full block (chains) and a partial one (tree)
    rnd = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.6).astype(np.complex64)
    far = rnd.copy()
    far[[5, 4000, 8500]] = [complex(1e6, -1e6), complex(-1e6, 3.0), complex(0.5, 1e6)]
    inf = rnd.copy()
    inf[[7, 8800]] = [complex(np.inf, 0.2), complex(-0.1, -np.inf)]
    return {"random": rnd, "half_way": _exact_rms_one_block(), "at_1e6": far, "inf": inf}


def test_tables_of_every_kind(cst):
    tables, blocks = _tables(), _table_blocks()
    # the half-way block discriminates: rms is exactly 1 and a sample has two nearest levels at the same distance
    hw = cc.evaluate(blocks["half_way"], pts=tables["grid8x8_f64"])
    assert _bits(hw["rms"], F32(1.0), np.float32) and _bits(hw["i"], blocks["half_way"].real, np.float32)
    d = np.sort(np.abs(hw["i"].astype(np.float64)[:, None] - LV_X[None, :]), axis=1)
    assert int((d[:, 0] == d[:, 1]).sum()) >= 7 * 256
    # the duplicate table is no grid: reading it as 4 x 4 levels would find the missing point
    dup = tables["grid4x4_dup"]
    full = np.array([[x, y] for x in np.unique(dup[:, 0]) for y in np.unique(dup[:, 1])], dtype=np.float32)
    assert len(full) == len(dup) == 16 and len(np.unique(dup, axis=0)) == 15
    assert cc.evaluate(blocks["random"], pts=full)["evm"] != cc.evaluate(blocks["random"], pts=dup)["evm"]
    for tname, pts in tables.items():
        assert _set_pts(cst, pts) == 0, tname
        for bname, iq in blocks.items():
            want = cc.evaluate(iq, r=1.5, pts=pts)
            assert want["evm"] is not None
            _check(cst.process(iq, n_tail=500), want, (tname, bname), n_tail=500)


def test_empty_table_oversized_table_and_non_finite_points(cst):
    nat = _nat()
    iq = _block(9000)
    want = cc.evaluate(iq, "8psk", 1.5)
    cst.set_modulation("8psk")
    _check(cst.process(iq), want, "8psk")
    # 65 points: refused, the 8psk table still in place
    big = np.random.default_rng(1).uniform(-1, 1, (65, 2)).astype(np.float32)
    assert _set_pts(cst, big) == -1 and b"n_points=65" in nat.lib.tdsa_last_error_string()
    _check(cst.process(iq), want, "after 65 points")
    # a NaN or infinite point: refused (np.min would give a NaN EVM, the kernel's fmin would drop the point; the
    # reference has no such table), the 8psk table still in place
    for dt in (np.float32, np.float64):
        for bad in (np.nan, np.inf, -np.inf):
            for col in (0, 1):
                pts = cc.reference_points("16qam").astype(dt)
                pts[9, col] = bad
                assert _set_pts(cst, pts) == -1, (dt, bad, col)
                msg = nat.lib.tdsa_last_error_string()
                assert b"must be finite" in msg and b"point 9" in msg, msg
                _check(cst.process(iq), want, ("after a non-finite point", dt, bad, col))
    # no points: EVM is None from the host call and NaN per segment, rms and counts as ever
    assert _set_pts(cst, np.zeros((0, 2), np.float32)) == 0
    none = cc.evaluate(iq, pts=np.zeros((0, 2), np.float32))
    assert none["evm"] is None and np.array_equal(none["counts"], want["counts"])
    _check(cst.process(iq, n_tail=100), none, "no table", n_tail=100)
    seg, hop, n_seg = 4000, 2500, 3
    with DeviceBuffer(iq.nbytes) as d_in, DeviceBuffer(n_seg * 128 * 128 * 4) as d_cnt:
        d_in.put(iq)
        d_cnt.put(np.full(n_seg * 128 * 128, 0xFFFFFFFF, np.uint32))
        rms, evm = cst.process_segments(None, d_in.ptr, nat.IN_C64, seg, hop, n_seg, d_cnt.ptr)
        assert np.isnan(evm).all()
        for s in range(n_seg):
            w = cc.evaluate(iq[s * hop:s * hop + seg], pts=np.zeros((0, 2), np.float32))
            assert _bits(rms[s], w["rms"], np.float32), s
            assert np.array_equal(d_cnt.get((128, 128), np.uint32, s * 128 * 128 * 4), w["counts"]), s


# ---- 4. the segment path at small shapes -----------------------------------------------------------------------------

SEG_FMT = {"int8": (cc.IN_I8, "16qam"), "uint8": (cc.IN_U8, "qpsk"), "complex64": (cc.IN_C64, "8psk")}
SEG_BINS = (1, 3, 127, 128)


def _raw(fmt, n, rng):
    """n samples of raw input, as the array the device reads."""
    if fmt == cc.IN_I8:
        return np.clip(np.round(rng.standard_normal(2 * n) * 45), -128, 127).astype(np.int8)
    if fmt == cc.IN_U8:
        raw = rng.integers(0, 256, 2 * n).astype(np.uint8)
        edge = np.array([0, 127, 128, 255, 255, 0, 128, 127], np.uint8)
        raw[:min(8, raw.size)] = edge[:min(8, raw.size)]
        return raw
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.4).astype(np.complex64)


def _seg_hops():
    """(seg_len, hop): 1, seg_len - 1 where that is positive, seg_len and seg_len + 3."""
    return [(n, hop) for n in (1, 7, 129, 8191, 8192, 8193, 20011)
            for hop in sorted({1, n, n + 3} | ({n - 1} if n > 1 else set()))]


@pytest.mark.parametrize("seg_len,hop", _seg_hops())
@pytest.mark.parametrize("fmt_name", ["int8", "uint8", "complex64"])
def test_segments_at_small_shapes(cst, fmt_name, seg_len, hop):
    """Every segment is the contract of its slice; the counts buffer holds garbage before the call; without a counts
    buffer rms and EVM are the same; a host call on the handle afterwards (its per-block buffers have grown) too."""
    fmt, mod = SEG_FMT[fmt_name]
    per = 1 if fmt == cc.IN_C64 else 2                      # array elements per sample
    cst.set_modulation(mod)
    cst.set_range(0.7)                                      # float64 edges that are no float32 numbers
    rng = np.random.default_rng(100000 * fmt + 5 * seg_len + hop)
    for n_seg in (1, 2, 257):                               # 257: cst_evm_kernel on two workgroups
        # every bin count for 1 and 2 segments; the 257-segment calls take one each, in turn over the (seg_len, hop)
        all_bins = SEG_BINS if n_seg < 257 else (SEG_BINS[_seg_hops().index((seg_len, hop)) % 4],)
        raw = _raw(fmt, hop * (n_seg - 1) + seg_len, rng)
        if fmt == cc.IN_I8 and n_seg == 2:
            raw[2 * hop:] = -128                            # segment 1: every byte -128
        if fmt == cc.IN_U8 and seg_len >= 4:
            assert {0, 127, 128, 255} <= set(raw[:2 * seg_len].tolist())
        slices = np.lib.stride_tricks.sliding_window_view(cc.to_complex(raw, fmt), seg_len)[::hop]
        assert len(slices) == n_seg
        want = cc.evaluate_rows(slices, mod, 0.7, all_bins[0])   # every segment, the contract of its slice
        with DeviceBuffer(max(raw.nbytes, 8)) as d_in:
            d_in.put(raw)
            for bins in all_bins:
                cst.set_bins(bins)
                nb2 = bins * bins
                with DeviceBuffer(n_seg * nb2 * 4) as d_cnt:
                    d_cnt.put(np.full(n_seg * nb2, 0xFFFFFFFF, np.uint32))
                    rms, evm = cst.process_segments(None, d_in.ptr, fmt, seg_len, hop, n_seg, d_cnt.ptr)
                    counts = d_cnt.get((n_seg, bins, bins), np.uint32)
                want_counts = cc.histogram_rows(want["i"], want["q"], 0.7, bins)
                for s in range(n_seg):
                    tag = (fmt_name, seg_len, hop, n_seg, bins, s)
                    assert _bits(rms[s], want["rms"][s], np.float32), (tag, rms[s], want["rms"][s])
                    assert _bits(evm[s], want["evm"][s], np.float64), (tag, evm[s], want["evm"][s])
                    assert np.array_equal(counts[s], want_counts[s]), tag
            rms2, evm2 = cst.process_segments(None, d_in.ptr, fmt, seg_len, hop, n_seg, None)
        assert _bits(rms, rms2, np.float32) and _bits(evm, evm2, np.float64), n_seg
        # the host call on the same handle: segment 0 again, from the host, against the contract of one block
        sl = raw[:per * seg_len]
        nt = min(seg_len, 300)
        _check(cst.process(sl, fmt=fmt, n_tail=nt), cc.evaluate(cc.to_complex(sl, fmt), mod, 0.7, bins),
               (fmt_name, seg_len, hop, n_seg, "host"), n_tail=nt)


def test_segment_cases_cover_every_bin_count():
    """The 257-segment calls meet every bin count at one block (seg_len <= 8192) and at more than one."""
    cases = _seg_hops()
    assert len(cases) == 26
    for multi in (False, True):
        assert {SEG_BINS[c % 4] for c, (n, _) in enumerate(cases) if (n > 8192) == multi} == set(SEG_BINS)


# ---- 5. extremes with the AGC on -------------------------------------------------------------------------------------

def _base_block(n=9001, seed=77):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)


@pytest.mark.parametrize("mod", ["qpsk", "8psk"])
def test_agc_threshold_both_sides(cst, mod):
    """One block scaled by 2^-k (exact): the contract's rms passes float32(1e-10) between two k; the raw samples are
    taken at and below it, the normalised ones above."""
    cst.set_modulation(mod)
    cst.set_range(1e-3)
    base = _base_block()
    taken = set()
    for k in range(28, 40):
        iq = (base * F32(2.0 ** -k)).astype(np.complex64)
        want = cc.evaluate(iq, mod, 1e-3)
        on = bool(want["rms"] > F32(1e-10))
        assert on == (not _bits(want["i"], iq.real, np.float32))
        taken.add(on)
        _check(cst.process(iq, n_tail=1000), want, (mod, k, on), n_tail=1000)
    assert taken == {True, False}                           # the family takes both branches
    # rms exactly float32(1e-10): not above it, no AGC
    iq = np.full(8, complex(F32(1e-10), 0), np.complex64)    # eight equal powers: every sum is exact
    want = cc.evaluate(iq, mod, 1e-3)
    assert _bits(want["rms"], F32(1e-10), np.float32) and _bits(want["i"], iq.real, np.float32)
    _check(cst.process(iq, n_tail=8), want, (mod, "at the threshold"), n_tail=8)


@pytest.mark.parametrize("mod", ["qpsk", "8psk", "64qam"])
def test_extreme_blocks(cst, mod):
    cst.set_modulation(mod)
    rng = np.random.default_rng(12)
    base = _base_block()
    tiny = np.nextafter(F32(0), F32(1))
    blocks = {}
    blocks["zeros"] = np.zeros(8200, np.complex64)
    # float32 denormals only: |x|^2 underflows to 0, rms = 0, the raw denormals reach the tail and the histogram
    den = (rng.integers(-(1 << 22), 1 << 22, 9001) * np.float64(tiny)).astype(np.float32)
    blocks["denormals"] = (den + 1j * np.roll(den, 17)).astype(np.complex64)
    # the AGC makes denormals: a few samples at 1e8 among samples at 1e-32, scale about 1e-6
    mix = (base * F32(1e-32)).astype(np.complex64)
    mix[[3, 5000, 8999]] = [complex(1e8, 0), complex(0, -1e8), complex(-7e7, 7e7)]
    blocks["agc_to_denormals"] = mix
    one_inf = base.copy()
    one_inf[4444] = complex(np.inf, 0.25)
    blocks["one_inf"] = one_inf
    minus_inf = base.copy()
    minus_inf[8500] = complex(0.5, -np.inf)
    blocks["one_minus_inf_q"] = minus_inf
    blocks["overflow"] = (base * F32(1e20)).astype(np.complex64)
    nan_q = base.copy()
    nan_q[8192] = complex(0.125, np.nan)
    blocks["nan_in_q_only"] = nan_q
    w = {}
    for r in (1e-3, 1.5):
        cst.set_range(r)
        for name, iq in blocks.items():
            w[name] = cc.evaluate(iq, mod, r)
            _check(cst.process(iq, n_tail=iq.size), w[name], (mod, r, name), n_tail=iq.size)
    # what each block is there for, by the contract
    assert w["zeros"]["rms"] == 0 and w["zeros"]["counts"].sum() == 8200
    assert w["denormals"]["rms"] == 0 and np.count_nonzero(w["denormals"]["i"]) > 9000
    sub = np.abs(w["agc_to_denormals"]["i"])
    assert w["agc_to_denormals"]["rms"] > 1 and int(((sub > 0) & (sub < F32(2.0 ** -126))).sum()) > 4000
    assert np.isinf(w["one_inf"]["rms"]) and np.isnan(w["one_inf"]["i"]).sum() == 1 and np.isnan(w["one_inf"]["evm"])
    assert np.isinf(w["overflow"]["rms"]) and not w["overflow"]["i"].any() and np.isfinite(w["overflow"]["evm"])
    assert np.isnan(w["nan_in_q_only"]["rms"]) and w["nan_in_q_only"]["counts"].sum() > 0


# ---- 6. offsets past 2^31 samples and 2^32 bytes ---------------------------------------------------------------------

@pytest.mark.parametrize("fmt_name,hop", [("int8", (1 << 31) + 8), ("complex64", (1 << 29) + 1)])
def test_second_segment_past_4_gib(cst, fmt_name, hop):
    """Two segments of 8193 samples, the second one hop samples on: past 2^31 samples (int8) and past 2^32 bytes
    (both).  Only the two segments are uploaded; nothing between them is read."""
    fmt, mod = SEG_FMT[fmt_name]
    seg_len, per, unit = 8193, (1 if fmt == cc.IN_C64 else 2), (8 if fmt == cc.IN_C64 else 2)
    assert hop * unit > 1 << 32
    cst.set_modulation(mod)
    rng = np.random.default_rng(hop % 1000)
    segs = [_raw(fmt, seg_len, rng) for _ in range(2)]
    with room_or_skip((hop + seg_len) * unit) as d_in, DeviceBuffer(2 * 128 * 128 * 4) as d_cnt:
        d_in.put(segs[0])
        d_in.put(segs[1], hop * unit)
        d_cnt.put(np.full(2 * 128 * 128, 0xFFFFFFFF, np.uint32))
        rms, evm = cst.process_segments(None, d_in.ptr, fmt, seg_len, hop, 2, d_cnt.ptr)
        counts = d_cnt.get((2, 128, 128), np.uint32)
    assert not np.array_equal(segs[0], segs[1])
    for s in range(2):
        res = cst.process(segs[s], fmt=fmt)
        assert _bits(rms[s], res.rms, np.float32) and _bits(evm[s], res.evm_rms, np.float64), (s, rms[s], res.rms)
        assert np.array_equal(counts[s], res.counts), s
        _check(res, cc.evaluate(cc.to_complex(segs[s], fmt), mod, 1.5), (fmt_name, s))


# ---- 7. C-ABI edges --------------------------------------------------------------------------------------------------

def test_misaligned_device_pointer_is_refused_on_the_host(cst):
    """A pointer not aligned to one sample never reaches a launch: rc -1, the message, the handle usable afterwards."""
    nat = _nat()
    iq = _block(3000)
    want = cc.evaluate(iq, "qpsk", 1.5)
    rms, evm = np.zeros(1, np.float32), np.zeros(1, np.float64)
    with DeviceBuffer(iq.nbytes + 64) as d_in:
        d_in.put(iq)
        for fmt, offs in ((nat.IN_I8, (1, 3)), (nat.IN_U8, (1, 5)), (nat.IN_C64, (1, 2, 4, 7))):
            for off in offs:
                rc = nat.lib.tdsa_constellation_process_dev(cst._h, None, fmt, d_in.at(off), 100, 100,
                                                            1, rms.ctypes.data_as(C.c_void_p),
                                                            evm.ctypes.data_as(C.c_void_p), None)
                assert rc == -1, (fmt, off, rc)
                assert b"aligned to one sample" in nat.lib.tdsa_last_error_string(), (fmt, off)
                assert rms[0] == 0 and evm[0] == 0
        _check(cst.process(iq), want, "after the refusals")
        # aligned to one sample, not to more: sample 1 of the buffer as the first
        r1, e1 = cst.process_segments(None, d_in.at(8), nat.IN_C64, 2999, 2999, 1, None)
        w1 = cc.evaluate(iq[1:], "qpsk", 1.5)
        assert _bits(r1[0], w1["rms"], np.float32) and _bits(e1[0], w1["evm"], np.float64)


def test_handle_limits_and_tail_arguments():
    from topdogspectrumanalyser_amd import Constellation
    nat = _nat()
    n = 8192 + 300
    iq = _block(n)
    want = cc.evaluate(iq, "qpsk", 1.5)
    with Constellation(max_host_samples=n) as c:             # n == max_host_samples exactly
        _check(c.process(iq, n_tail=n), want, "n == max_host_samples", n_tail=n)
        with pytest.raises(nat.TdsaError, match="max_host_samples"):
            c.process(_block(n + 1))
        # n_tail > n through the C-ABI: clamped to n, i[n] then q[n]
        rms, evm, has = C.c_float(), C.c_double(), C.c_int()
        tail = np.full(2 * n + 16, -7.0, np.float32)
        rc = nat.lib.tdsa_constellation_process(c._h, nat.IN_C64, iq.ctypes.data_as(C.c_void_p), n, n + 12345,
                                                C.byref(rms), C.byref(evm), C.byref(has), None,
                                                tail.ctypes.data_as(C.c_void_p))
        assert rc == 0 and has.value == 1
        assert _bits(rms.value, want["rms"], np.float32) and _bits(evm.value, want["evm"], np.float64)
        assert _bits(tail[:n], want["i"], np.float32) and _bits(tail[n:2 * n], want["q"], np.float32)
        assert (tail[2 * n:] == -7.0).all()
        # n_tail > 0 with no tail buffer: nothing to write to, the other outputs as ever
        cnt = np.zeros((128, 128), np.uint32)
        rc = nat.lib.tdsa_constellation_process(c._h, nat.IN_C64, iq.ctypes.data_as(C.c_void_p), n, 500, C.byref(rms),
                                                C.byref(evm), C.byref(has), cnt.ctypes.data_as(C.c_void_p), None)
        assert rc == 0 and _bits(rms.value, want["rms"], np.float32) and _bits(evm.value, want["evm"], np.float64)
        assert np.array_equal(cnt, want["counts"])
    with Constellation(max_host_samples=1) as c:             # the smallest handle
        for z in (complex(0.3, -0.4), complex(0, 0), complex(np.nan, 1)):
            one = np.array([z], np.complex64)
            _check(c.process(one, n_tail=1), cc.evaluate(one, "qpsk", 1.5), z, n_tail=1)
        with pytest.raises(nat.TdsaError, match="max_host_samples"):
            c.process(np.zeros(2, np.complex64))
