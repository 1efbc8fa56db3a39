"""How csrc/Makefile compiles a kernel file, for the tests and tools that cross-compile one for gfx950 without a GPU and
read the result: the flags (the Makefile's CXXFLAGS with its global EXTRA, plus the file's own `EXTRA +=` line), the
hipcc call (object or assembly listing, device code only, with the compiler's resource remarks), and the remarks parsed
into {kernel: {field: value}}.  Used by tests/test_*kernel_resources.py, tests/test_isa_frozen.py and tools/isa_hash.py.

For the per-unit resource tests it also holds what each of them needs: a header's `constexpr` and a public `#define`
as Python ints, the unit's place in the Makefile, the skip-or-compile fixture body, and the no-scratch / no-spills
asserts on one kernel's remarks."""
import os
import re
import shutil
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "topdogspectrumanalyser_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FRAME_SOURCE, FRAME_SIZES = "tdsa_spectrum_inst.hip", tuple(range(6, 15))     # the frame kernel: one object per log2 N


def makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def flags(source):
    """The flags the Makefile compiles `source` (a file name of csrc) with."""
    mk = makefile()
    var = {name: re.search(r"^%s\s*\??=\s*(.*)$" % name, mk, re.M).group(1) for name in ("ARCH", "EXTRA", "CXXFLAGS")}
    own = re.search(r"^\$\(B\)/%s\.o:\s*EXTRA\s*\+=\s*(.*)$" % re.escape(os.path.splitext(source)[0]), mk, re.M)
    if own:
        var["EXTRA"] += " " + own.group(1)
    return re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"]).split()


def compile_kernels(source, out, log2n=None):
    """Device code of `source` into `out`: an assembly listing if `out` ends in .s, else an object.  Returns the
    compiler's kernel-resource-usage remarks as {kernel: {field: value}}."""
    cmd = [HIPCC] + flags(source) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    if log2n is not None:
        cmd.append(f"-DTDSA_LOG2N={log2n}")
    r = subprocess.run(cmd + ["-S" if out.endswith(".s") else "-c", source, "-o", out], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    return remarks(r.stderr)


def remarks(stderr):
    kernels, cur = {}, None
    for ln in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\S+)\s+\[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return kernels


def header_const(header, name):
    """`constexpr int` or `constexpr long long` `name` of csrc/`header` as a Python int; other k... names in its
    initialiser are looked up in the same header.  A name the header does not define is looked up in the headers of
    csrc it includes."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr (?:int|long long) %s = ([^;]+);" % name, text)
    if not m:
        for inc in re.findall(r'^#include "(\w+\.hpp)"', text, re.M):
            try:
                return header_const(inc, name)
            except LookupError:
                pass
        raise LookupError(f"{name} is not in {header} or what it includes")
    expr = re.sub(r"\bk\w+", lambda k: str(header_const(header, k.group(0))), m.group(1)).replace("1ll", "1")
    return int(eval(expr))


def public_define(name):
    """`#define name <integer>` of include/tdsa_hip.h, with or without parentheses and a `u` suffix."""
    m = re.search(r"^#define %s \(?(-?\d+)u?\)?$" % name, open(os.path.join(ROOT, "include", "tdsa_hip.h")).read(), re.M)
    return int(m.group(1))


def cross_compiled(tmp_path_factory, source, listing=False):
    """The body of a module fixture: skips without hipcc, else the remarks of `source`, or (remarks, assembly text)."""
    import pytest
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    stem = os.path.splitext(source)[0]
    out = str(tmp_path_factory.mktemp(stem) / (stem + (".s" if listing else ".o")))
    kernels = compile_kernels(source, out)
    return (kernels, open(out).read()) if listing else kernels


def in_makefile(unit, headers=(), own_flags=None):
    """Asserts that csrc/Makefile builds tdsa_`unit`.hip and its C-ABI file into the library, that a change of any of
    `headers` rebuilds it, and that the unit's only rule of its own is `EXTRA += own_flags` (none for None)."""
    mk = makefile()
    assert re.search(r"^OBJS\s*=.*\$\(B\)/tdsa_%s\.o\b" % unit, mk, re.M), unit
    assert re.search(r"^CAPI\s*=.*\b%s\b" % unit, mk, re.M), unit
    for h in headers:
        assert re.search(r"^HDRS\s*=.*\b%s\b" % re.escape(h), mk, re.M), h
    own = re.findall(r"^\$\(B\)/tdsa_%s\.o:(.*)$" % unit, mk, re.M)
    assert own == ([] if own_flags is None else [" EXTRA += " + own_flags]), own
    if own_flags:
        assert set(own_flags.split()) <= set(flags(f"tdsa_{unit}.hip"))


def no_scratch_no_spills(k):
    """One kernel's remarks: no scratch memory, no spilled vector register, no spilled scalar register."""
    assert int(k["ScratchSize [bytes/lane]"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0, k
    assert int(k["SGPRs Spill"]) == 0, k
