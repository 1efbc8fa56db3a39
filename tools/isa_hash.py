#!/usr/bin/env python3
"""Opcode-sequence fingerprint of kernels in a gfx950 assembly listing (hipcc -S --cuda-device-only):
tools/isa_hash.py file.s [name-substring]  ->  one line per kernel: instructions, sha256[:16] of the mnemonic sequence.
tools/isa_hash.py --all  ->  the same for every .hip of csrc and the nine sizes of the frame kernel, each compiled with
the Makefile's flags (tests/kernel_build.py), under a line with the file's name: run it at two commits and compare.
Operands, labels, comments and directives are left out: register allocation details and kernarg offsets may move, the
instruction stream may not (tests/test_isa_frozen.py pins the BASELINE instantiations of the frame kernel with it)."""
import concurrent.futures
import hashlib
import os
import re
import sys
import tempfile


def kernels(path):
    out, name, ops = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, ops = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = ops
            name = None
            continue
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ops.append(t.split()[0])
    return out


def fingerprint(ops):
    return len(ops), hashlib.sha256("\n".join(ops).encode()).hexdigest()[:16]


def every_kernel(jobs=8):
    """[(title, {kernel: ops})] for every .hip of csrc, the frame kernel's file once per size."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import kernel_build as kb
    units = [(f, None) for f in sorted(os.listdir(kb.CSRC)) if f.endswith(".hip") and f != kb.FRAME_SOURCE]
    units += [(kb.FRAME_SOURCE, k) for k in kb.FRAME_SIZES]
    with tempfile.TemporaryDirectory() as tmp:
        def one(unit):
            src, log2n = unit
            asm = os.path.join(tmp, f"{src}.{log2n}.s")
            kb.compile_kernels(src, asm, log2n)
            return src if log2n is None else f"{src} -DTDSA_LOG2N={log2n}", kernels(asm)
        with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
            return list(ex.map(one, units))


if __name__ == "__main__":
    if sys.argv[1] == "--all":
        for title, found in every_kernel():
            print(title)
            for k, ops in found.items():
                print("  %s %d %s" % ((k,) + fingerprint(ops)))
        sys.exit(0)
    sub = sys.argv[2] if len(sys.argv) > 2 else ""
    for k, ops in kernels(sys.argv[1]).items():
        if sub in k:
            n, h = fingerprint(ops)
            print(f"{k} {n} {h}")
