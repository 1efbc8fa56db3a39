"""How csrc/Makefile compiles a kernel file, for the tests and tools that cross-compile one for gfx950 without a GPU and
read the result: the flags (the Makefile's CXXFLAGS with its global EXTRA, plus the file's own `EXTRA +=` line), the
hipcc call (object or assembly listing, device code only, with the compiler's resource remarks), and the remarks parsed
into {kernel: {field: value}}.  Used by tests/test_*kernel_resources.py, tests/test_isa_frozen.py and tools/isa_hash.py."""
import os
import re
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
