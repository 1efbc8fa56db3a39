"""The 16384-point frame kernel with the sliding front end (tdsa_spectrum_c3_inst.hip) on the MI355X.

A byte-format plan with frame-mean DC, dB rows and hold off / max hold takes that kernel when hop == N/2 and the frozen
kernel at any other hop.  So the same plan run at hop 8191, one frame per call on the slice that holds the frame, is the
reference: it computes every frame with the parent's code path.  Rows and hold trace of the variant must equal it byte for
byte (integer DC sums are exact in any order, the float path is the same text), whatever mixture of whole and sliding
frames a workgroup sees: one frame (whole), two and three (on a 256-workgroup grid still one each), 257 (one workgroup
slides once), batches whose captures end between two workgroups (3 x 3 frames) and inside a workgroup's range
(3 x 171 frames: the first frame of a capture is whole again).  Both are also held against the float64 gold at the
project's two-unit bound.
"""
import numpy as np
import pytest

from oracle import spectrum_oracle as so
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat

pytestmark = pytest.mark.gpu

N, HOP, FS = 16384, 8192, 20e6
NF = 257                                  # one more than the grid of a 256-CU device
NS = HOP * (NF - 1) + N
COUNTS = (1, 2, 3, NF)
REL_TOL, DB_TOL, UNITS = 1e-4, 1e-3, 2    # tests/test_gpu_parity.py::_check


def _engine(hold):
    e = SpectrumEngine(N, max_frames=3 * 171)
    e.set_window(so.hackrf_window(N))
    e.configure(db_mode="mag", log_floor=so.LOG_FLOOR, dc_alpha=1.0, hold_max=hold)
    return e


@pytest.fixture(scope="module")
def capture():
    """fmt -> (raw bytes of NS samples, float64 gold rows of its NF frames at hop N/2)"""
    i8 = so.synth_iq_int8(NS, N, seed=41)
    out = {}
    for fmt in ("i8", "u8"):
        if fmt == "i8":
            raw, x = i8, so.unpack_iq_int8(i8)
        else:
            raw = (i8.astype(np.int16) + 128).astype(np.uint8)
            x = so.unpack_iq_uint8_rtl(raw)
        br = so.HackrfBranchOracle(N, FS, precision="gold")
        gold = np.stack([np.asarray(br.power_levels(x[k * HOP: k * HOP + N])) for k in range(NF)])
        raw.flags.writeable = False
        gold.flags.writeable = False
        out[fmt] = (raw, gold)
    return out


_FROZEN = {}


def _frozen(capture, fmt, hold):
    """Rows of the NF frames, and the hold trace after COUNTS frames, from the plan at hop 8191 (frozen kernel), one frame
    per call.  Computed once per (format, hold)."""
    if (fmt, hold) not in _FROZEN:
        raw, _ = capture[fmt]
        in_fmt = nat.IN_I8 if fmt == "i8" else nat.IN_U8
        holds = {}
        with DeviceBuffer.of(raw) as d_in, DeviceBuffer(NF * N * 4) as d_out, _engine(hold) as e:
            for f in range(NF):
                e.process_device(in_fmt, d_in.at(2 * HOP * f, 2 * N), N, HOP - 1, 1, d_out.at(4 * N * f, 4 * N))
                if hold and f + 1 in COUNTS:
                    e.synchronize()
                    holds[f + 1] = e.hold()[0]
            e.synchronize()
            rows = d_out.get((NF, N), np.float32)
        rows.flags.writeable = False
        _FROZEN[fmt, hold] = (rows, holds)
    return _FROZEN[fmt, hold]


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0].tolist()}"


def _gold_check(rows, gold, what):
    rel, ddb = so.parity_metrics(rows, gold, amp_floor=UNITS * so.AMP_FLOOR)
    assert rel <= REL_TOL and ddb <= DB_TOL, f"{what}: rel={rel:.3e} ddb={ddb:.3e}"


@pytest.mark.parametrize("hold", [True, False])
@pytest.mark.parametrize("nf", COUNTS)
@pytest.mark.parametrize("fmt", ["i8", "u8"])
def test_rows_and_hold_equal_the_frozen_kernel(capture, fmt, nf, hold):
    raw, gold = capture[fmt]
    want_rows, want_hold = _frozen(capture, fmt, hold)
    with _engine(hold) as e:
        rows = e.process(raw[: 2 * (HOP * (nf - 1) + N)], hop=HOP)
        mx = e.hold()[0] if hold else None
    assert rows.shape == (nf, N)
    _same_bytes(rows, want_rows[:nf], f"{fmt} {nf} frames")
    _gold_check(rows, gold[:nf], f"{fmt} {nf} frames")
    if hold:
        _same_bytes(mx, want_hold[nf], f"{fmt} hold over {nf} frames")
        rel, ddb = so.HoldAllowance(amp_floor=UNITS * so.AMP_FLOOR).update(gold[:nf]).metrics(mx, gold[:nf].max(axis=0))
        assert rel <= REL_TOL and ddb <= DB_TOL, (rel, ddb)


@pytest.mark.parametrize("fmt,nf,step", [("i8", 3, 3), ("u8", 3, 3), ("i8", 171, 43), ("u8", 171, 43)])
def test_batched_captures_equal_single_launches_and_the_frozen_kernel(capture, fmt, nf, step):
    """Three captures of nf frames in one launch; capture s holds frames s * step .. s * step + nf - 1 of the module's
    capture.  The strides are larger than the captures and an odd number of samples apart, the output has a gap."""
    raw, gold = capture[fmt]
    want_rows, _ = _frozen(capture, fmt, True)
    in_fmt = nat.IN_I8 if fmt == "i8" else nat.IN_U8
    n_seg, ns = 3, HOP * (nf - 1) + N
    seg_stride, out_stride = 2 * ns + 2 * 21, nf * N + 64
    blob = np.zeros(seg_stride * n_seg, dtype=np.uint8)
    for s in range(n_seg):
        blob[s * seg_stride: s * seg_stride + 2 * ns] = raw[2 * HOP * step * s: 2 * HOP * step * s + 2 * ns].view(np.uint8)
    with DeviceBuffer.of(blob) as d_in, DeviceBuffer(4 * out_stride * n_seg) as d_out:
        got, held = {}, {}
        for batched in (True, False):
            d_out.put(np.zeros(out_stride * n_seg, np.float32))
            with _engine(True) as e:
                if batched:
                    e.process_device_batch(in_fmt, d_in.ptr, seg_stride, n_seg, ns, HOP, nf, d_out.ptr, out_stride)
                else:
                    for s in range(n_seg):
                        e.process_device(in_fmt, d_in.at(s * seg_stride, 2 * ns), ns, HOP, nf, d_out.at(4 * s * out_stride, 4 * nf * N))
                e.synchronize()
                held[batched] = e.hold()[0]
            got[batched] = d_out.get((n_seg, out_stride), np.float32)
    _same_bytes(got[True], got[False], f"{fmt} batched against single launches")
    _same_bytes(held[True], held[False], f"{fmt} hold, batched against single launches")
    assert not got[True][:, nf * N:].any()                       # the gaps between the captures' rows stay untouched
    frames = np.concatenate([np.arange(s * step, s * step + nf) for s in range(n_seg)])
    rows = got[True][:, : nf * N].reshape(n_seg * nf, N)
    _same_bytes(rows, want_rows[frames], f"{fmt} batch of {n_seg} x {nf}")
    _gold_check(rows, gold[frames], f"{fmt} batch of {n_seg} x {nf}")
    _same_bytes(held[True], want_rows[frames].max(axis=0), f"{fmt} hold of the batch")
