#!/usr/bin/env python3
"""Developer tool: C3-shaped launches in batches of 600, time per step against elapsed time - shows the ~50 ms an
idle MI355X needs before its clocks settle (profiles/r02_c3_experiments.txt), and the same after a 2 s pause."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from topdogspectrumanalyser_amd import DeviceBuffer, SpectrumEngine, _native as nat
n, hop, F = 16384, 8192, 2440
ns = hop * (F - 1) + n
iq = np.random.default_rng(0).integers(-100, 100, size=2 * ns, dtype=np.int8)
with DeviceBuffer(iq.nbytes) as dev_in, DeviceBuffer(F * n * 4) as dev_out:
    dev_in.put(iq)
    e = SpectrumEngine(n, max_frames=F)
    e.set_window(np.hanning(n).astype(np.float32))
    e.configure(db_mode="mag", log_floor=1e-12, dc_alpha=1.0, hold_max=True)
    t00 = time.perf_counter()
    for b in range(60):
        e.timer_begin()
        for _ in range(600):
            e.process_device(nat.IN_I8, dev_in.ptr, ns, hop, F, dev_out.ptr)
        ms = e.timer_end()
        print(f"t={time.perf_counter()-t00:6.2f}s  batch {b:2d}: {ms/600*1e3:.1f} us/step")
    time.sleep(2.0)
    for b in range(5):
        e.timer_begin()
        for _ in range(600):
            e.process_device(nat.IN_I8, dev_in.ptr, ns, hop, F, dev_out.ptr)
        ms = e.timer_end()
        print(f"after 2 s idle: batch {b}: {ms/600*1e3:.1f} us/step")
