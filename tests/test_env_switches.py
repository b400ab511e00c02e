"""The library's environment switches: every SVT_HIP_* variable the kernel sources read is documented and is exercised by a test, a tool or the
benchmark -- a switch nobody sets selects code nobody runs -- and the switches retired with their kernel variants (docs/design/retired-variants.md)
stay out of the sources, the public headers and the knob list."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svt-av1_amd", "csrc")

RETIRED = ["SVT_HIP_SGR_WALK", "SVT_HIP_SGR_WALK_NA10", "SVT_HIP_SGR_WALK_CAND", "SVT_HIP_SGR_WALK_HIST", "SVT_HIP_SGR_WALK_PACKED", "SVT_HIP_WIENER_WALK",
           "SVT_HIP_CDEF_DEDUPE", "SVT_HIP_TF_DIV", "SVT_HIP_CDEF_SELECT_SLICES"]


def _files(top, skip_dirs=("build", "__pycache__")):
    if os.path.isfile(top):
        yield top
        return
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x not in skip_dirs]
        for n in names:
            yield os.path.join(d, n)


def _text(path):
    with open(path, errors="replace") as f:
        return f.read()


def _mentions(name, text):
    return re.search(r"\b" + re.escape(name) + r"(?![A-Z0-9_])", text) is not None   # the whole name: SVT_HIP_SGR_WALK is not SVT_HIP_SGR_WALK_HIST_W


def _switches():
    names = set()
    for p in _files(CSRC):
        if p.endswith((".hip", ".cpp", ".h")):
            names |= set(re.findall(r'getenv\(\s*"(SVT_HIP_[A-Z0-9_]+)"', _text(p)))
    return sorted(names)


def test_every_switch_is_documented_and_exercised():
    names = _switches()
    assert names, "no getenv(\"SVT_HIP_...\") found: the scan is broken"
    docs = _text(os.path.join(ROOT, "INTEGRATION.md")) + "".join(_text(p) for p in _files(os.path.join(ROOT, "docs", "kernels")))
    me = os.path.abspath(__file__)
    users = "".join(_text(p) for top in ("tests", "tools", "bench.py") for p in _files(os.path.join(ROOT, top))
                    if os.path.abspath(p) != me and not p.endswith((".npy", ".npz", ".bin", ".so", ".pyc")))
    undocumented = [n for n in names if not _mentions(n, docs)]
    unused = [n for n in names if not _mentions(n, users)]
    assert not undocumented, f"read in svt-av1_amd/csrc but in neither INTEGRATION.md nor docs/kernels/: {undocumented}"
    assert not unused, f"read in svt-av1_amd/csrc but set or read by nothing under tests/, tools/ or bench.py: {unused}"


def test_retired_switches_stay_out():
    where = [p for p in _files(CSRC) if p.endswith((".hip", ".cpp", ".h", ".map")) or os.path.basename(p) == "Makefile"]
    where += list(_files(os.path.join(ROOT, "include"))) + [os.path.join(ROOT, "INTEGRATION.md")]
    found = [(n, os.path.relpath(p, ROOT)) for p in where for n in RETIRED if _mentions(n, _text(p))]
    assert not found, f"retired switches (docs/design/retired-variants.md) are back: {found}"
