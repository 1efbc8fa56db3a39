"""Constellation analysis on the MI355X through the C-ABI (tdsa_constellation_*): every vector captured from the
imported reference (tests/golden/constellation.npz) is reproduced bit for bit, the unchanged DataProcessor drives a
ConstellationView to the reference's read-out, a C3-sized capture in HBM is analysed per segment, and the error paths
leave the handle usable."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import constellation_contract as cc
from topdogspectrumanalyser_amd import DeviceBuffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "constellation.npz"))


@pytest.fixture(scope="module")
def cst():
    from topdogspectrumanalyser_amd import Constellation
    with Constellation(max_host_samples=1 << 17) as c:
        yield c


def _case(g, k):
    fmt, r, mp, scatter = g[f"c{k}_meta"]
    return int(fmt), float(r), int(mp), bool(scatter), str(g[f"c{k}_mod"])


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_every_reference_vector_bit_for_bit(g, cst):
    for k in range(int(g["n_cases"])):
        fmt, r, mp, scatter, mod = _case(g, k)
        raw = g[f"c{k}_raw"]
        n = raw.size // 2 if fmt != cc.IN_C64 else raw.size
        want = cc.evaluate(cc.to_complex(raw, fmt), mod, r)
        cst.set_modulation(mod)
        cst.set_range(r)
        start = slice(-min(mp, n), None).indices(n)[0]
        res = cst.process(raw, fmt=fmt, n_tail=n - start)
        assert _same(res.rms, want["rms"]), (k, res.rms, want["rms"])
        if g[f"c{k}_evm_none"]:
            assert res.evm_rms is None, k
        else:
            assert _same(res.evm_rms, float(g[f"c{k}_evm"])), (k, res.evm_rms, float(g[f"c{k}_evm"]))
        if scatter:
            si, sq = res.scatter()
            assert np.array_equal(si, g[f"c{k}_sx"], equal_nan=True), k
            assert np.array_equal(sq, g[f"c{k}_sy"], equal_nan=True), k
        else:
            assert np.array_equal(res.counts, g[f"c{k}_counts"]), k
            assert np.array_equal(res.image(), np.log1p(g[f"c{k}_counts"].astype(np.float64))), k
        assert np.array_equal(res.counts, want["counts"]), k


def test_data_processor_drives_the_view_to_the_reference_readout(g):
    from topdogspectrumanalyser_amd import ConstellationView, DataProcessor
    from topdogspectrumanalyser_amd.utils.constants import DisplayMode

    class Label:
        text = None

        def setText(self, s):
            self.text = s

    view = ConstellationView()
    for k in range(int(g["n_cases"])):
        fmt, r, mp, scatter, mod = _case(g, k)
        view.set_mode("scatter" if scatter else "density")
        view.set_modulation(mod)
        view.set_range(r)
        view.set_max_points(mp)
        label = Label()
        block = cc.to_complex(g[f"c{k}_raw"], fmt)
        mw = types.SimpleNamespace(current_source=types.SimpleNamespace(read_samples_only=lambda b=block: b),
                                   current_stacked_index=DisplayMode.CONSTELLATION_2D, constellation_2d_widget=view,
                                   marker_readout_label=label)
        dp = DataProcessor.__new__(DataProcessor)
        dp.mw, dp.dm = mw, types.SimpleNamespace(constellation_modulation=mod)
        dp._process_constellation_data()
        if np.isnan(g[f"c{k}_evm"]) and not g[f"c{k}_evm_none"]:
            # a NaN EVM: the reference's read-out tests `evm > 0` and prints nothing; this package's DataProcessor
            # tests `evm <= 0` and formats the NaN - a difference of the read-out code, which this change leaves as is
            assert np.isnan(view.last_evm_rms) and str(g[f"c{k}_text"]) == "", k
        else:
            assert label.text == str(g[f"c{k}_text"]), k
        if g[f"c{k}_evm_none"]:
            assert view.last_evm_rms is None, k
        else:
            assert _same(view.last_evm_rms, float(g[f"c{k}_evm"])), k
        if scatter:
            assert np.array_equal(view.scatter_xy[0], g[f"c{k}_sx"], equal_nan=True), k
            assert np.array_equal(view.scatter_xy[1], g[f"c{k}_sy"], equal_nan=True), k
        else:
            assert np.array_equal(view.image, np.log1p(g[f"c{k}_counts"].astype(np.float64))), k
    # an empty or missing block changes nothing; an error keeps the last value
    last = view.last_evm_rms
    view.update_iq_data(None)
    view.update_iq_data(np.zeros(0, np.complex64))
    view.update_iq_data(np.ones(64, np.float32))          # real input: refused, logged
    assert view.last_evm_rms is last


def test_nan_block(cst):
    rng = np.random.default_rng(11)
    iq = ((rng.standard_normal(9000) + 1j * rng.standard_normal(9000)) * 0.3).astype(np.complex64)
    iq[4321] = complex(np.nan, 0.1)
    cst.set_modulation("qpsk")
    cst.set_range(1.5)
    res = cst.process(iq)
    assert np.isnan(res.rms) and np.isnan(res.evm_rms)
    want = cc.histogram(iq.real, iq.imag, 1.5)              # no AGC: rms is NaN
    assert np.array_equal(res.counts, want)
    assert int(res.counts.sum()) == int(((np.abs(iq.real) <= 1.5) & (np.abs(iq.imag) <= 1.5)).sum())
    assert cc.readout(res.evm_rms, "qpsk") == ""


@pytest.mark.parametrize("mod", ["64qam", "qpsk"])
def test_c3_capture_in_hbm(cst, mod):
    """20 M int8 samples in HBM as 16 384-sample ticks: per-segment rms / EVM and histograms are the reference's."""
    from topdogspectrumanalyser_amd import _native as nat
    seg, n_seg = 16384, 1220
    rng = np.random.default_rng(3 if mod == "qpsk" else 4)
    raw = np.clip(np.round(rng.standard_normal(2 * seg * n_seg) * 40 + 20 * np.sign(rng.standard_normal(2 * seg * n_seg))),
                  -128, 127).astype(np.int8)
    cst.set_modulation(mod)
    cst.set_range(1.5)
    with DeviceBuffer.of(raw) as d_in, DeviceBuffer(n_seg * 128 * 128 * 4) as d_cnt:
        rms, evm = cst.process_segments(None, d_in.ptr, nat.IN_I8, seg, seg, n_seg, d_cnt.ptr)
        for s in list(rng.choice(n_seg, 10, replace=False)) + [0, n_seg - 1]:
            want = cc.evaluate(cc.to_complex(raw[2 * s * seg:2 * (s + 1) * seg], cc.IN_I8), mod, 1.5)
            assert rms[s] == want["rms"] and evm[s] == want["evm"], (s, rms[s], want["rms"], evm[s], want["evm"])
            if s % 3 == 0 or s in (0, n_seg - 1):
                got = d_cnt.get((128, 128), np.uint32, s * 128 * 128 * 4)
                assert np.array_equal(got, want["counts"]), s


def test_overlapping_odd_segments_equal_host_blocks(cst):
    """hop != seg_len and partial blocks: each device segment is exactly the host call on that slice."""
    from topdogspectrumanalyser_amd import _native as nat
    rng = np.random.default_rng(8)
    seg, hop, n_seg = 20011, 7777, 9
    iq = ((rng.standard_normal(hop * (n_seg - 1) + seg) + 1j * rng.standard_normal(hop * (n_seg - 1) + seg)) * 0.2
          ).astype(np.complex64)
    cst.set_modulation("8psk")
    cst.set_range(2.0)
    with DeviceBuffer.of(iq) as d_in, DeviceBuffer(n_seg * 128 * 128 * 4) as d_cnt:
        rms, evm = cst.process_segments(None, d_in.ptr, nat.IN_C64, seg, hop, n_seg, d_cnt.ptr)
        for s in range(n_seg):
            res = cst.process(iq[s * hop:s * hop + seg])
            assert rms[s] == res.rms and evm[s] == res.evm_rms, s
            assert np.array_equal(d_cnt.get((128, 128), np.uint32, s * 128 * 128 * 4), res.counts), s


def test_hot_bin_counts_exactly(cst):
    from topdogspectrumanalyser_amd import _native as nat
    n = 1 << 24
    raw = np.tile(np.array([40, -40], np.int8), n)
    cst.set_modulation("qpsk")
    cst.set_range(1.5)
    with DeviceBuffer.of(raw) as d_in, DeviceBuffer(128 * 128 * 4) as d_cnt:
        rms, evm = cst.process_segments(None, d_in.ptr, nat.IN_I8, n, n, 1, d_cnt.ptr)
        got = d_cnt.get((128, 128), np.uint32)
        assert int(got.max()) == n and int(got.sum()) == n
        x = cc.to_complex(raw[:2], cc.IN_I8)                 # every sample: the same |x|^2, summed 2^24 times
        a = cc.cabs(x)
        want_rms = np.sqrt(cc.np_mean(np.full(n, (a * a)[0], np.float32))).astype(np.float32)
        assert rms[0] == want_rms
        scl = np.float32(1.0) / want_rms
        i = (x.real + x.imag * np.float32(0)) * scl
        q = (x.imag - x.real * np.float32(0)) * scl
        assert np.array_equal(np.argwhere(got), np.argwhere(cc.histogram(i, q, 1.5)))


def test_error_paths_leave_the_handle_usable(cst):
    from topdogspectrumanalyser_amd import _native as nat
    rng = np.random.default_rng(2)
    raw = rng.integers(-100, 100, 2 * 5000).astype(np.int8)
    cst.set_modulation("16qam")
    cst.set_range(1.5)
    want = cc.evaluate(cc.to_complex(raw, cc.IN_I8), "16qam", 1.5)

    def ok():
        res = cst.process(raw)
        assert res.rms == want["rms"] and res.evm_rms == want["evm"] and np.array_equal(res.counts, want["counts"])

    ok()
    with pytest.raises(ValueError, match="real input"):
        cst.process(np.ones(100, np.float32))
    x = np.ones(100, np.float32)
    rc = nat.lib.tdsa_constellation_process(cst._h, 3, x.ctypes.data_as(C.c_void_p), 50, 0, None, None, None, None,
                                            None)
    assert rc == -1 and b"real input" in nat.lib.tdsa_last_error_string()
    ok()
    with pytest.raises(nat.TdsaError, match="bins=129"):
        cst.set_bins(129)
    ok()
    with pytest.raises(nat.TdsaError, match="max_host_samples"):
        cst.process(np.zeros(cst.max_host_samples + 1, np.complex64))
    ok()
    with pytest.raises(nat.TdsaError, match="empty"):
        cst.process(np.zeros(0, np.complex64))
    ok()
    cst.set_bins(64)                                   # a coarser histogram, then back
    res = cst.process(raw)
    assert np.array_equal(res.counts, cc.evaluate(cc.to_complex(raw, cc.IN_I8), "16qam", 1.5, bins=64)["counts"])
    cst.set_bins(128)
    ok()
