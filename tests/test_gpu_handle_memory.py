"""Every handle type of the C-ABI layer gives its device memory back: created, driven through the host and the device
entry point and through every buffer that grows on demand, and closed, many times over, the free device memory returns.
test_no_device_memory_left_behind (test_gpu_parity.py) does this for plans, pipes, the density histogram, the waterfall
ring and the averager; here are the others: the 17 handle types that test does not reach, one case each and the
history once per kind, since its views differ - 18 cases.

Sizes: a buffer this test can see is one of 2 MiB or more - forgotten in each of the 40 measured cycles it costs 80 MiB,
above the 64 MiB the assertion allows - so the constructor arguments and the calls make every buffer a handle can
allocate that large where the API lets them (2^18 .. 2^21 staged samples, 2^16 segments per device call, 2^19 floats of
rows).  What the API fixes below that (NCO and reference tables, per-stream summaries, the counters) and pinned host
memory this test cannot see; tests/test_capi_memory.py covers those: no allocation is left that a list could forget."""
import gc
import os

import numpy as np
import pytest

from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat
from topdogspectrumanalyser_amd.analytics import Constellation
from topdogspectrumanalyser_amd.channelizer import Channelizer
from topdogspectrumanalyser_amd.correlate import Correlator, zadoff_chu
from topdogspectrumanalyser_amd.demod import Demodulator
from topdogspectrumanalyser_amd.detect import SignalDetector
from topdogspectrumanalyser_amd.engine import TraceState
from topdogspectrumanalyser_amd.eye import EyeDiagram
from topdogspectrumanalyser_amd.fsk import FskAnalyzer
from topdogspectrumanalyser_amd.history3d import TraceHistory
from topdogspectrumanalyser_amd.measure import ChannelMeasure
from topdogspectrumanalyser_amd.modquality import ModQuality
from topdogspectrumanalyser_amd.powerstats import PowerStats
from topdogspectrumanalyser_amd.pulses import PulseAnalyzer
from topdogspectrumanalyser_amd.sweep import SweepAssembler, plan_steps
from topdogspectrumanalyser_amd.symbols import SymbolSync
from topdogspectrumanalyser_amd.zerospan import ZeroSpan
from topdogspectrumanalyser_amd.zoom import DownConverter, zoom_window

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

M = 1 << 18                    # complex samples of one host block: 2 MiB
SEG, DEV_SEGS = 64, 1 << 16    # samples of a segment; segments of a device call (hop 2): 2^16 records


class Shared:
    """What the cycles read and write beside the handle under test; made once, before the first measurement."""

    def __init__(self):
        rng = np.random.default_rng(7)
        self.x = ((rng.standard_normal(M) + 1j * rng.standard_normal(M)) * 0.5).astype(np.complex64)
        self.rows = self.x.view(np.float32)                                   # 2^19 floats, as dB rows of any width
        self.d_x = DeviceBuffer.of(np.tile(self.x, 4))                        # 2^20 samples = 2^21 floats = 8 MiB
        self.d_y = DeviceBuffer(16 << 20)                                     # outputs of the device entry points
        self.engine = SpectrumEngine(1024, max_frames=2)                      # the producer of the sweep's rows
        self.engine.set_window(zoom_window(1024))
        self.engine.configure(db_mode="mag", log_floor=1e-12, dc_alpha=-1.0)

    def close(self):
        for h in (self.engine, self.d_y, self.d_x):
            h.close()


def _ddc(s):
    with DownConverter(2, 1e6, 1e5, max_host_samples=1 << 19) as h:
        h.process(s.x)
        h.process_device(None, nat.IN_C64, s.d_x.ptr, M, s.d_y.ptr)


def _chan(s):
    with Channelizer(8, 1e6, max_host_samples=1 << 19) as h:
        h.process(s.x)
        h.process_device(None, nat.IN_C64, s.d_x.ptr, M, s.d_y.ptr, M // 8 + 8)


def _demod(s):
    with Demodulator("fm", 1e6, decimation=2, channels=2, max_host_samples=1 << 20) as h:
        h.process(s.x.reshape(2, M // 2))
        h.process_device(None, s.d_x.ptr, M // 2, M // 2, s.d_y.ptr, M // 4 + 8)
        h.measure()


def _symsync(s):
    with SymbolSync(4.0, "qpsk", max_host_samples=1 << 19) as h:
        h.process(s.x, SEG, raw=True)                                                       # 2^12 records ...
        h.process_device(None, s.d_x.ptr, SEG, 2, DEV_SEGS, s.d_y.ptr, h.symbols_per_segment(SEG))   # ... grown to 2^16


def _fsk(s):
    with FskAnalyzer(4.0, 2, "iq", max_host_samples=1 << 21) as h:
        h.process(s.x, SEG)
        h.process_device(None, s.d_x.ptr, SEG, 2, DEV_SEGS, s.d_y.ptr, h.symbols_per_segment(SEG))


def _eye(s):
    with EyeDiagram(4.0, "iq", max_host_samples=M, max_segments=1 << 17) as h:
        ck = h.clocks(delta=1.0, n_seg=M // SEG)
        h.process(s.x, SEG, ck, traces=True)                                                # the traces' two buffers grow
        h.process_device(None, s.d_x.ptr, SEG, SEG, M // SEG, ck)
        h.read()


def _modq(s):
    with ModQuality("qpsk", max_host_symbols=M) as h:
        h.process(s.x, K=SEG, errors=True)                                                  # records and both outputs grow
        h.process_device(None, s.d_x.ptr, 4, 4, DEV_SEGS, s.d_y.ptr, 4)                     # the records grow again


def _detect(s):                # narrow rows, so that 2^16 of them fit: 2 MiB of row records, 10 MiB of signal records
    with SignalDetector(32, max_signals=4, max_host_rows=1 << 14) as h:
        h.process(s.rows.reshape(1 << 14, 32))
        h.process_device(None, s.d_x.ptr, 1 << 16)                                          # both record buffers grow
        h.occupancy()


def _meas(s):                  # likewise: 5 MiB of row records, 6 MiB of channel records
    with ChannelMeasure(32, [(8 * i, 8 * i + 7) for i in range(4)], limit=np.zeros(32), max_host_rows=1 << 14) as h:
        h.process(s.rows.reshape(1 << 14, 32))
        h.process_device(None, s.d_x.ptr, 1 << 16)
        h.totals()


def _pstat(s):
    with PowerStats(256, max_host_samples=M) as h:                                          # 256 streams: 4 MiB of counts
        h.process(s.x.reshape(256, M // 256))
        h.process_device(None, s.d_x.ptr, M // 256, M // 256)
        h.read()


def _pulse(s):
    with PulseAnalyzer(1, capacity=1 << 16, max_host_samples=M) as h:                       # 4 MiB of records
        h.configure(1.0)
        h.process(s.x)
        h.process_device(None, s.d_x.ptr, M)
        h.read_summaries()


def _corr(s):
    with Correlator(zadoff_chu(63), streams=16, capacity=4096, max_host_samples=M) as h:    # 2 MiB of records
        h.configure(0.5)
        h.process(s.x.reshape(16, M // 16))
        h.configure(0.5, min_distance=1 << 16)               # a longer ring and more blocks: all six buffers grow
        h.process_device(None, s.d_x.ptr, M // 16, M // 16)
        h.read_summaries()


def _sweep(s):
    N, F, hop, S = 1024, 2, 512, 512
    centres, kept, bin_hz = plan_steps(100e6, 100e6 + S * 768 * 2000.0, 2.048e6, N)
    grid = np.linspace(centres[0], centres[-1], 1 << 18)                                    # 2 MiB of grid, 2 MiB of trace
    n_per = (F - 1) * hop + N
    with SweepAssembler(N, centres, kept, bin_hz, grid) as h:                               # 1.5 MiB of step traces
        h.update_device(None, 0, S, s.d_x.ptr, F)
        h.run_device(s.engine, nat.IN_I8, s.d_x.ptr, 2 * n_per, 0, S, n_per, hop, F)        # 4 MiB of rows grow
        h.read("interp")
        s.engine.synchronize()


def _zspan(s):
    with ZeroSpan(float(1 << 20), buffer_s=1.0, max_host_samples=M) as h:                   # a ring of 2^20 floats
        h.push(s.x)
        h.push_device(None, nat.IN_C64, s.d_x.ptr, M)
        h.push_device(None, nat.IN_C64, s.d_x.ptr, M)
        h.view("free_run", n_display=600_000)                                               # 2.3 MiB of results grow


def _history(kind):
    def cycle(s):
        with TraceHistory(512, 1024, kind) as h:                                            # a ring of 2 MiB
            row = s.rows[:1024]
            if kind == "heights":
                h.push(row, row, row)                                                       # the staging of three rows grows
                h.push_rows(None, s.d_x.ptr, 512)
                h.ribbon(np.arange(1024.0), columns=256)                                    # the views' scratch grows ...
                h.lines(columns=256)                                                        # ... and again: 2 MiB a piece
            else:
                h.push(row)
                h.push_rows(None, s.d_x.ptr, 512)
                h.surface(columns=256)
    return cycle


def _constellation(s):
    with Constellation(max_host_samples=M) as h:
        h.process(s.x, n_tail=1000)
        h.process_segments(None, s.d_x.ptr, nat.IN_C64, 16, 2, M)                           # 2^18 segments: all four sums grow


def _trace(s):
    n = 1 << 19                                                                             # 2 MiB a trace
    with TraceState(n) as h:
        row = s.rows[:n]
        h.update(row, hold_max=True, hold_min=True)
        h.avg_set_mode("exp", 4)
        h.avg_process(np.abs(row).astype(np.float64))


CYCLES = {"ddc": _ddc, "chan": _chan, "demod": _demod, "symsync": _symsync, "fsk": _fsk, "eye": _eye, "modq": _modq,
          "detect": _detect, "meas": _meas, "pstat": _pstat, "pulse": _pulse, "corr": _corr, "sweep": _sweep,
          "zspan": _zspan, "history-heights": _history("heights"), "history-levels": _history("levels"),
          "constellation": _constellation, "trace": _trace}


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.close()


@pytest.mark.parametrize("name", sorted(CYCLES))
def test_a_handle_gives_its_device_memory_back(shared, name):
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("free device memory is a property of the whole GPU: other xdist workers allocate beside this one")
    import torch

    cycle = CYCLES[name]
    for _ in range(3):
        cycle(shared)                              # first-use allocations of the runtime itself
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        cycle(shared)
    gc.collect()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f"{name}: {(free0 - free1) / 2**20:.1f} MiB not returned after 40 cycles")
    assert free0 - free1 < 64 << 20, f"{name}: {(free0 - free1) / 2**20:.1f} MiB of device memory not returned"
