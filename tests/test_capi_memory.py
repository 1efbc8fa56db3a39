"""The C-ABI layer owns device and pinned memory by type: Dev<T> and Pinned<T> of tdsa_capi_mem.hpp are the only
places that allocate and free it, so no destroy path has a list of buffers that could forget one.  Reads the sources;
reaches no device."""
import os
import re

CSRC = os.path.join(os.path.dirname(__file__), "..", "topdogspectrumanalyser_amd", "csrc")
MEM_HEADER = "tdsa_capi_mem.hpp"
RAW = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "free_all(", "grow_device(", "grow_pinned(")

# memory the CALLER owns: handed out as a raw pointer and freed by the caller's own call, so no type can hold it
RAW_LEFT = {
    "tdsa_capi_plan.cpp": (2, "tdsa_dev_*: the hipMalloc of the alloc call, the hipFree of the free call"),
    "tdsa_capi_welch.cpp": (3, "tdsa_peer_*: the hipMalloc of the alloc call, its hipFree when no IPC handle can be had, and "
                               "the hipFree of the free call"),
}
CALLER_OWNED = r"^int tdsa_(?:dev|peer)_(?:alloc|free)\(.*?^}"


def _code_lines(name):
    return [ln for ln in open(os.path.join(CSRC, name)).read().splitlines() if not ln.lstrip().startswith("//")]


def test_raw_allocation_calls_live_in_the_owning_types_alone():
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if not (re.fullmatch(r"tdsa_capi_\w+\.cpp", f) or f == "tdsa_capi_internal.hpp"):
            continue
        n = sum(ln.count(tok) for ln in _code_lines(f) for tok in RAW)
        if n:
            found[f] = n
    assert found == {f: n for f, (n, why) in RAW_LEFT.items()}, found
    # ... and what is left is inside the functions that hand memory to the caller and take it back
    for f, (n, why) in RAW_LEFT.items():
        bodies = re.findall(CALLER_OWNED, "\n".join(_code_lines(f)), re.M | re.S)
        assert len(bodies) == 2 and sum(b.count(tok) for b in bodies for tok in RAW) == n, (f, why)


def test_the_owning_types_are_one_header_that_the_build_knows():
    mem = "\n".join(_code_lines(MEM_HEADER))
    for tok in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree("):
        assert tok in mem, tok
    for cls in ("Dev", "Pinned"):
        assert re.search(r"%s\(const %s&\) = delete;" % (cls, cls), mem), cls      # a handle struct cannot be copied
        assert re.search(r"~%s\(\) \{ release\(\); \}" % cls, mem), cls
    internal = open(os.path.join(CSRC, "tdsa_capi_internal.hpp")).read()
    assert '#include "%s"' % MEM_HEADER in internal
    assert re.search(r"^HDRS\s*=.*\b%s\b" % re.escape(MEM_HEADER), open(os.path.join(CSRC, "Makefile")).read(), re.M)
