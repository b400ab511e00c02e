"""CPU: the ctypes binding of svt-av1_amd/__init__.py against include/svt_hip.h, whole: every structure typedef has one mirror with the header's member names
and a C99 compiler's size and offsets, every declared function is in PROTOTYPES with parameters and a return value of the declared kinds, and the constants the
package repeats are the header's.  A wrong entry would not fail in Python: it would hand a kernel launch a shifted argument."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

UNBOUND = {"svt_hip_rtcd_release", "svt_hip_rtcd_report"}   # svt_hip_rtcd.h: bookkeeping of the per-call wrappers, driven by the reference-side harness only
CONSTANTS = [("SQUARE_PU_COUNT", "SVT_HIP_SQUARE_PU_COUNT"), ("MAX_SAD_VALUE", "SVT_HIP_MAX_SAD_VALUE"), ("GM_MAX_REFS", "SVT_HIP_GM_MAX_REFS"),
             ("GM_FIT_MAX_JOBS", "SVT_HIP_GM_FIT_MAX_JOBS"), ("GM_MAX_CORNERS", "SVT_HIP_GM_MAX_CORNERS"), ("TPL_MAX_WINDOW", "SVT_HIP_TPL_MAX_WINDOW"),
             ("CDEF_SELECT_STATE_BYTES", "SVT_HIP_CDEF_SELECT_STATE_BYTES")]
C_INTS = {"int": (4, True), "unsigned": (4, False), "unsigned int": (4, False), "size_t": (8, False), "int8_t": (1, True), "uint8_t": (1, False),
          "int16_t": (2, True), "uint16_t": (2, False), "int32_t": (4, True), "uint32_t": (4, False), "int64_t": (8, True), "uint64_t": (8, False)}


def _text(name):
    """the header without comments and preprocessor lines"""
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", re.sub(r"//.*$", "", txt, flags=re.M), flags=re.M)


def _structs():
    """{SvtHipX: [member names]} of svt_hip.h; its structures are flat, so a body is declarations split at ';' and declarators split at ','"""
    txt = _text("svt_hip.h")
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", txt):
        out[name] = [re.sub(r"\[[^\]]*\]", "", d).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    closing = set(re.findall(r"\}\s*(\w+)\s*;", txt)) - {"SvtHipStatus"}   # the one enum
    assert closing == set(out), f"typedefs the struct pattern does not read: {sorted(closing ^ set(out))}"
    return out


def _prototypes():
    """{name: (return type, [parameter declarations])} of every svt_hip_* function the two headers declare"""
    out = {}
    for hdr in ("svt_hip.h", "svt_hip_rtcd.h"):
        txt = _text(hdr)
        found = re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(svt_hip_\w+)\s*\(([^;{}]*)\)\s*;", txt, flags=re.M)
        assert sorted(n for _, n, _ in found) == sorted(re.findall(r"\b(svt_hip_\w+)\s*\(", txt)), f"{hdr}: a declaration the prototype pattern does not read"
        for ret, name, params in found:
            assert name not in out, f"{name} declared twice"
            parts, depth = [""], 0
            for ch in params:
                depth += ch in "([" ; depth -= ch in ")]"
                if ch == "," and depth == 0: parts.append("")
                else: parts[-1] += ch
            parts = [" ".join(p.split()) for p in parts]
            out[name] = (" ".join(ret.split()), [] if parts == ["void"] else parts)
    return out


def _c_kind(decl, named):
    """a C declaration -> "ptr", "double", "float", (bytes, signed) or the structure's name; None when it is none of these"""
    if "*" in decl or "[" in decl: return "ptr"
    words = [w for w in decl.split() if w != "const"]
    if named: words = words[:-1]
    t = " ".join(words)
    return t if t in ("double", "float", "void") or t.startswith("SvtHip") else C_INTS.get(t)


def _py_kind(t, pkg):
    if t is None: return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)): return "ptr"
    if issubclass(t, C.Structure): return "SvtHip" + t.__name__ if getattr(pkg, t.__name__, None) is t else None
    code = getattr(t, "_type_", None)
    if code in ("d", "f"): return {"d": "double", "f": "float"}[code]
    return (C.sizeof(t), code.islower()) if isinstance(code, str) and code in "bBhHiIlLqQ" else None


@pytest.fixture(scope="module")
def compiled(pkg, tmp_path_factory):
    """what one C99 program prints: "<Struct> <sizeof>", "<Struct>.<field> <offsetof> <sizeof>" for every mirror field, "<constant> <value>" """
    mirrors = {"SvtHip" + n: t for n, t in vars(pkg).items() if isinstance(t, type) and issubclass(t, C.Structure) and t is not C.Structure}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "svt_hip.h"', "int main(void) {"]
    for c, t in mirrors.items():
        if c not in _structs(): continue   # reported by test_one_mirror_per_structure; its name would not compile
        lines.append(f'printf("{c} %zu\\n", sizeof({c}));')
        lines += [f'printf("{c}.{f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c} *)0)->{f}));' for f, *_ in t._fields_]
    lines += [f'printf("{py} %lld\\n", (long long)({c}));' for py, c in CONSTANTS] + ["return 0; }"]
    d = tmp_path_factory.mktemp("abi")
    (d / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "abi.c"), "-o", str(d / "abi")])
    got = {k: [int(x) for x in v] for k, *v in (l.split() for l in subprocess.run([str(d / "abi")], capture_output=True, text=True, check=True).stdout.splitlines())}
    return mirrors, got


def test_one_mirror_per_structure(compiled):
    mirrors, _ = compiled
    declared = _structs()
    assert len(declared) >= 49
    assert sorted(declared) == sorted(mirrors), f"no mirror: {sorted(set(declared) - set(mirrors))}; no such typedef: {sorted(set(mirrors) - set(declared))}"
    for c, t in mirrors.items():
        assert [f for f, *_ in t._fields_] == declared[c], f"{c}: the mirror's fields are not the header's members, in order"


def test_layouts_match_the_compiler(compiled):
    mirrors, got = compiled
    for c, t in mirrors.items():
        assert got[c] == [C.sizeof(t)], f"{c}: sizeof {got[c][0]} in C, {C.sizeof(t)} in ctypes"
        for f, *_ in t._fields_:
            d = getattr(t, f)
            assert got[f"{c}.{f}"] == [d.offset, d.size], f"{c}.{f}: offset, size {got[c + '.' + f]} in C, {[d.offset, d.size]} in ctypes"


def test_constants_match_the_header(pkg, compiled):
    for py, c in CONSTANTS:
        assert compiled[1][py] == [getattr(pkg, py)], f"{py} = {getattr(pkg, py)}, {c} = {compiled[1][py][0]}"


def test_every_prototype_is_bound_with_the_declared_kinds(pkg):
    declared = _prototypes()
    assert len(declared) >= 150
    assert sorted(set(declared) - UNBOUND) == sorted(pkg.PROTOTYPES), (f"declared, not bound: {sorted(set(declared) - UNBOUND - set(pkg.PROTOTYPES))}; "
                                                                       f"bound, not declared: {sorted(set(pkg.PROTOTYPES) - set(declared))}")
    for name, (restype, argtypes) in pkg.PROTOTYPES.items():
        ret, params = declared[name]
        want, have = [_c_kind(ret, False)] + [_c_kind(p, True) for p in params], [_py_kind(restype, pkg)] + [_py_kind(a, pkg) for a in argtypes]
        assert None not in want, f"{name}: cannot classify {[d for d, k in zip([ret] + params, want) if k is None]}"
        assert len(have) == len(want), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (w, h) in enumerate(zip(want, have)):
            assert w == h, f"{name}: {'return value' if i == 0 else 'parameter %d' % i} '{([ret] + params)[i]}' is {w} in the header, {h} in PROTOTYPES"
