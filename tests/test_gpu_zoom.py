"""Zoom front end on the MI355X: the down-converter against the float64 restatement of tests/zoom_contract.py, bit for
bit where the contract fixes the bits (impulses, splits of the input, raw against unpacked input, device composition),
and ZoomSpectrum's rows against the oracle's frame path."""
import ctypes as C

import numpy as np
import pytest

import zoom_contract as zc
from oracle import spectrum_oracle as so
from topdogspectrumanalyser_amd import Constellation, DeviceBuffer, SpectrumEngine, _native as nat
from topdogspectrumanalyser_amd.zoom import DownConverter, ZoomSpectrum, design_decimator, nco_step, zoom_window

pytestmark = pytest.mark.gpu

FS = 20e6


def _raw(rng, n, fmt):
    if fmt == zc.FMT_I8:
        return rng.integers(-128, 128, 2 * n).astype(np.int8)
    if fmt == zc.FMT_U8:
        return rng.integers(0, 256, 2 * n).astype(np.uint8)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)


def _split(raw, fmt, cuts):
    step = 1 if fmt == zc.FMT_C64 else 2
    edges = [0] + list(cuts) + [len(raw) // step]
    return [raw[step * a:step * b] for a, b in zip(edges[:-1], edges[1:])]


def _run(ddc, parts):
    return np.concatenate([ddc.process(p) for p in parts])


@pytest.mark.parametrize("D,T", [(8, 34 * 8), (5, 37), (3, 2)])
def test_impulse_is_bit_exact(D, T):
    rng = np.random.default_rng(T)
    h = rng.standard_normal(T).astype(np.float32)
    n = 4 * T + 5 * D + 11
    for n0 in (0, 1, D - 1, T // 2 + 3, 2 * T + 1):
        x = np.zeros(n, np.complex64)
        x[n0] = 1
        for cut in (n0, n0 + 1, max(1, n0 - D)):
            with DownConverter(D, FS, taps=h) as ddc:
                y = _run(ddc, _split(x, zc.FMT_C64, [cut]))
            k = np.arange(y.size) * D - n0
            want = np.where((k >= 0) & (k < T), h[np.clip(k, 0, T - 1)], 0).astype(np.complex64)
            assert y.size == zc.n_outputs(n, D)
            assert np.array_equal(y, want), (n0, cut)


def test_impulse_with_offset_checks_the_rotator():
    D, T = 4, 64
    h = design_decimator(D, 16)
    rng = np.random.default_rng(7)
    for s in (1, 0x12345678, 0x80000000, 0xFFFFFFFF, int(rng.integers(1, 1 << 32))):
        for n0 in (0, 5, 777, 4093):
            x = np.zeros(4200, np.complex64)
            x[n0] = 1
            with DownConverter(D, FS, taps=h) as ddc:
                nat.check(nat.lib.tdsa_ddc_set_nco(ddc._h, s))
                y = _run(ddc, _split(x, zc.FMT_C64, [n0 // 2 + 1]))
            m = np.arange(y.size)
            k = m * D - n0
            on = (k >= 0) & (k < T)
            rot = np.exp(-2j * np.pi * ((n0 * s) % (1 << 32)) / 2.0 ** 32)
            want = h[k[on]].astype(np.float64) * rot
            ulp = np.spacing(np.abs(h[k[on]]).astype(np.float32)).astype(np.float64)
            err = np.maximum(np.abs(y[on].real - want.real), np.abs(y[on].imag - want.imag))
            assert np.all(err <= 2 * ulp), (s, n0, float(np.max(err / ulp)))
            assert np.all(y[~on] == 0)


@pytest.mark.parametrize("D", [2, 3, 8, 64, 1000, 4096])
@pytest.mark.parametrize("fmt", [zc.FMT_I8, zc.FMT_U8, zc.FMT_C64])
def test_accuracy_against_the_restatement(D, fmt):
    rng = np.random.default_rng(D * 7 + fmt)
    for custom in (False, True):
        h = (rng.standard_normal(3 * D + 1).astype(np.float32) / D) if custom else design_decimator(D)
        T = h.size
        n = T + 48 * D + 5
        raw = _raw(rng, n, fmt)
        x = zc.unpack(raw, fmt)
        bound = np.abs(h.astype(np.float64)).sum() * np.abs(x).max()
        for off in (0.0, 0.3 * FS, -0.3 * FS, 0.49 * FS, -0.49 * FS):
            with DownConverter(D, FS, off, taps=h) as ddc:
                y = ddc.process(raw)
                step = ddc.phase_step
            assert y.size == zc.n_outputs(n, D)
            ms = np.unique(np.concatenate([np.arange(0, y.size, max(1, y.size // 40)), [y.size - 1]]))
            ref = zc.reference(raw, fmt, h, D, [(0, step)], ms)
            err = np.abs(y[ms] - ref)
            assert err.max() <= 1e-5 * bound, (custom, off, err.max() / bound)
            assert np.sqrt(np.mean(err ** 2)) <= 1e-6 * bound, (custom, off, np.sqrt(np.mean(err ** 2)) / bound)


@pytest.mark.parametrize("D,T", [(8, None), (64, None), (3, 40)])
def test_chunking_is_bit_identical(D, T):
    rng = np.random.default_rng(D + 1)
    h = design_decimator(D) if T is None else rng.standard_normal(T).astype(np.float32)
    T = h.size
    n = 6 * T + 9 * D + 3
    raw = _raw(rng, n, zc.FMT_I8)
    retune_at = n // 2 + 3

    def run(cuts):
        edges = [0] + sorted(set(int(c) for c in cuts) | {retune_at}) + [n]
        with DownConverter(D, FS, 0.21 * FS, taps=h) as ddc:
            out = []
            for a, b in zip(edges[:-1], edges[1:]):
                out.append(ddc.process(raw[2 * a:2 * b]))
                if b == retune_at:
                    ddc.set_offset(-0.37 * FS)
            return np.concatenate(out)

    whole = run([])
    small = [1, 2, 3, D - 1, D, D + 1, T + 1, T + 2]
    cuts = list(np.cumsum(small))
    cuts += list(range(cuts[-1] + D - 1, n, D - 1))[:20]
    cuts += list(np.cumsum(rng.integers(1, 3 * T, 40)) + cuts[-1])
    for cs in (cuts, list(rng.integers(1, n, 30)), list(range(1, 200))):
        got = run([c for c in cs if 0 < c < n])
        assert got.dtype == np.complex64 and np.array_equal(got.view(np.uint64), whole.view(np.uint64))


def test_zoom_spectrum_chunking_rows_and_holds_are_bit_identical():
    D, N, hop = 8, 1024, 512
    rng = np.random.default_rng(3)
    n = 40 * N * D // 4
    raw = _raw(rng, n, zc.FMT_I8)
    retune_at = n // 3

    def run(cuts):
        with ZoomSpectrum(FS, D, N, offset_hz=0.1 * FS, hop=hop) as z:
            z.engine.configure(hold_max=True, hold_min=True)
            rows = []
            edges = [0] + sorted(set(cuts) | {retune_at}) + [n]
            for a, b in zip(edges[:-1], edges[1:]):
                rows.append(z.process(raw[2 * a:2 * b]))
                if b == retune_at:
                    z.set_offset(-0.2 * FS)
            mx, mn = z.hold()
            return np.concatenate(rows), mx, mn

    r0, mx0, mn0 = run([])
    assert r0.shape[0] == (-(-n // D) - -(-(design_decimator(D).size - 1) // D) - N) // hop + 1
    for cuts in ([1, D - 1, D + 1, 500, 501, 5000], list(rng.integers(1, n, 25)), list(range(7, n, 3001))):
        r, mx, mn = run([c for c in cuts if 0 < c < n])
        assert np.array_equal(r, r0) and np.array_equal(mx, mx0) and np.array_equal(mn, mn0)


def _raw_against_unpacked(D, fmt):
    rng = np.random.default_rng(fmt + 11)
    raw = _raw(rng, 30000, fmt)
    with DownConverter(D, FS, 0.17 * FS) as a, DownConverter(D, FS, 0.17 * FS) as b:
        ya = a.process(raw)
        yb = b.process(zc.unpack(raw, fmt))
    assert np.array_equal(ya.view(np.uint64), yb.view(np.uint64))


@pytest.mark.parametrize("fmt", [zc.FMT_I8, zc.FMT_U8])
def test_raw_input_equals_its_complex_unpacking(fmt):
    _raw_against_unpacked(8, fmt)


@pytest.mark.parametrize("D", [13, 24])
@pytest.mark.parametrize("fmt", [zc.FMT_I8, zc.FMT_U8])
def test_raw_input_equals_its_complex_unpacking_at_lanes_16_and_32(D, fmt):
    _raw_against_unpacked(D, fmt)


def _oracle_rows(y, N, hop, m0, fs_out):
    br = so.HackrfBranchOracle(N, fs_out, dc_alpha=0.0, precision="gold")
    nf = (len(y) - m0 - N) // hop + 1
    return np.stack([br.power_levels(y[m0 + k * hop: m0 + k * hop + N]) for k in range(nf)])


def test_zoomed_rows_match_the_oracle_frame_path():
    D, N, hop = 64, 4096, 2048
    rng = np.random.default_rng(5)
    n = (12 * N + 40) * D
    t = np.arange(n)
    x = (0.5 * np.exp(2j * np.pi * (1.0e6 + 3 * FS / (D * N)) * t / FS) + 0.01 * (rng.standard_normal(n) +
         1j * rng.standard_normal(n))).astype(np.complex64)
    with ZoomSpectrum(FS, D, N, offset_hz=1.0e6, hop=hop) as z:
        rows = z.process(x)
        m0 = z.ddc.first_full_output
    with DownConverter(D, FS, 1.0e6) as ddc:
        y = ddc.process(x)
    gold = _oracle_rows(y, N, hop, m0, FS / D)
    assert rows.shape == gold.shape and rows.shape[0] >= 20
    rel, ddb = so.parity_metrics(rows, gold)
    assert rel <= 1e-4 and ddb <= 1e-3, (rel, ddb)


def test_bin_placement():
    D, N = 64, 1024
    off = 2.5e6
    for j in (-300, -1, 0, 7, 400):
        f = off + j * FS / (D * N)
        n = (4 * N) * D
        x = np.exp(2j * np.pi * f * np.arange(n) / FS).astype(np.complex64)
        with ZoomSpectrum(FS, D, N, offset_hz=off) as z:
            rows = z.process(x)
            fb = z.freq_bins(100e6)
        assert rows.shape[0] >= 1
        assert np.all(np.argmax(rows, axis=1) == N // 2 + j), j
        assert np.isclose(fb[N // 2 + j], 100e6 + z.offset_hz + j * FS / (D * N))


def test_alias_rejection():
    D, N = 16, 1024
    off = 1e6
    j = 100                                   # in band: 0.1 fs/D of the 0.4 fs/D alias-free band
    fo = FS / D
    n = 3 * N * D
    t = np.arange(n)

    def level(f):
        x = np.exp(2j * np.pi * f * t / FS).astype(np.complex64)
        with ZoomSpectrum(FS, D, N, offset_hz=off) as z:
            return z.process(x)[:, N // 2 + j].max()

    inband = level(off + j * fo / N)
    for k in (1, -1, 2):                      # stop-band tones that fold onto the same bin
        assert inband - level(off + j * fo / N + k * fo) >= 95.0, k


def test_composition_on_the_device():
    D, N = 8, 512
    rng = np.random.default_rng(9)
    n = 64 * N * D // 8 + 13
    raw = _raw(rng, n, zc.FMT_I8)
    with DownConverter(D, FS, 0.05 * FS) as ddc:
        y_host = ddc.process(raw)
    with DownConverter(D, FS, 0.05 * FS) as ddc, SpectrumEngine(N, max_frames=64) as eng, \
            Constellation(max_host_samples=1 << 16) as cst, DeviceBuffer(raw.nbytes) as d_in, \
            DeviceBuffer(8 * (n // D + 1)) as d_y, DeviceBuffer(4 * 64 * N) as d_rows:
        eng.set_window(zoom_window(N))
        eng.configure(db_mode="mag", dc_alpha=-1.0)
        d_in.put(raw)
        n_out = ddc.process_device(eng, nat.IN_I8, d_in.ptr, n, d_y.ptr)
        nf = (n_out - N) // N + 1
        eng.process_device(nat.IN_C64, d_y.ptr, n_out, N, nf, d_rows.ptr)
        seg = 1000
        rms, evm = cst.process_segments(eng, d_y.ptr, nat.IN_C64, seg, seg, n_out // seg)
        eng.synchronize()
        rows_dev = d_rows.get(nf * N, np.float32).reshape(nf, N)
        y_dev = d_y.get(n_out, np.complex64)
    assert np.array_equal(y_dev.view(np.uint64), y_host.view(np.uint64))
    with SpectrumEngine(N, max_frames=64) as eng2, Constellation(max_host_samples=1 << 16) as cst2:
        eng2.set_window(zoom_window(N))
        eng2.configure(db_mode="mag", dc_alpha=-1.0)
        rows_host = eng2.process(y_host[:(nf - 1) * N + N], hop=N)
        for s in range(n_out // seg):
            r = cst2.process(y_host[s * seg:(s + 1) * seg], counts=False)
            assert r.rms == rms[s] and (r.evm_rms == evm[s] or (np.isnan(evm[s]) and r.evm_rms is None))
    assert np.array_equal(rows_dev, rows_host)


def test_full_c3_capture():
    D = 64
    n = 20_000_000
    rng = np.random.default_rng(20)
    raw = rng.integers(-128, 128, 2 * n).astype(np.int8)
    h = design_decimator(D)
    n_out = zc.n_outputs(n, D)
    with DownConverter(D, FS, 0.123 * FS) as ddc, SpectrumEngine(1024) as eng, DeviceBuffer(raw.nbytes) as d_in, \
            DeviceBuffer(8 * (n_out + 8)) as d_y:
        step = ddc.phase_step
        d_in.put(raw)
        assert ddc.process_device(eng, nat.IN_I8, d_in.ptr, n, d_y.ptr) == n_out
        eng.synchronize()
        one = d_y.get(n_out, np.complex64)
        ddc.reset()
        cuts = [0, 1, 999_999, 5_000_003, 5_000_064, 12_345_678, 19_999_999, n]
        got = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            got += ddc.process_device(eng, nat.IN_I8, d_in.at(2 * a, 2 * (b - a)), b - a, d_y.at(8 * got))
        assert got == n_out
        eng.synchronize()
        chunked = d_y.get(n_out, np.complex64)
    assert np.array_equal(one.view(np.uint64), chunked.view(np.uint64))
    ms = np.sort(rng.choice(n_out, 2048, replace=False))
    k = np.arange(h.size)
    idx = ms[:, None] * D - k[None, :]
    ok = idx >= 0
    idx = np.where(ok, idx, 0)
    x = (raw[2 * idx].astype(np.float64) + 1j * raw[2 * idx + 1].astype(np.float64)) / 128.0
    v = np.where(ok, x * np.exp(-2j * np.pi * ((idx * step) % (1 << 32)) / 2.0 ** 32), 0)
    ref = v @ h.astype(np.float64)
    bound = np.abs(h.astype(np.float64)).sum() * 1.0
    err = np.abs(one[ms] - ref)
    assert err.max() <= 1e-5 * bound and np.sqrt(np.mean(err ** 2)) <= 1e-6 * bound


def test_error_paths_leave_the_handle_usable():
    D = 8
    rng = np.random.default_rng(4)
    raw = _raw(rng, 5000, zc.FMT_C64)
    with DownConverter(D, FS, 0.1 * FS, max_host_samples=4096) as ref:
        want = np.concatenate([ref.process(raw[:3000]), ref.process(raw[3000:])])
    with DownConverter(D, FS, 0.1 * FS, max_host_samples=4096) as ddc:
        n = C.c_size_t()
        out = np.empty(1000, np.complex64)
        p = out.ctypes.data_as(C.c_void_p)
        y1 = ddc.process(raw[:3000])
        assert nat.lib.tdsa_ddc_process(ddc._h, 9, p, 10, p, C.byref(n)) == -1
        assert nat.lib.tdsa_ddc_process(ddc._h, 2, p, 5000, p, C.byref(n)) == -1        # above max_host_samples
        assert nat.lib.tdsa_ddc_process(ddc._h, 2, p, 100, None, C.byref(n)) == -1      # outputs but nowhere to go
        assert nat.lib.tdsa_ddc_process_dev(ddc._h, None, 2, None, 100, None, C.byref(n)) == -1
        assert nat.lib.tdsa_ddc_set_taps(ddc._h, p, 0) == -1
        assert nat.lib.tdsa_ddc_set_taps(ddc._h, p, ddc.taps.size + 1) == -1
        with pytest.raises(ValueError):
            ddc.set_offset(0.6 * FS)
        y2 = ddc.process(raw[3000:])
    assert np.array_equal(np.concatenate([y1, y2]), want)
