#!/usr/bin/env python3
"""Compare the gfx950 machine code of kernel units between two revisions, kernel by kernel.

    tools/isa_diff.py REV_A REV_B UNIT        e.g.  tools/isa_diff.py HEAD~1 HEAD sgr_walk.hip
    tools/isa_diff.py REV_A REV_B --units-a UNIT... --units-b UNIT...
                                              e.g.  tools/isa_diff.py HEAD~1 HEAD --units-a percall.hip percall2.hip --units-b percall.hip cdef_select.hip

The second form is for code that moved between units: the kernels of each side's units are pooled and matched across the pools by name (one of the two lists may
be left out: it is then the other side's).  A kernel name that two units of one side define is an error.  Where a kernel's unit is not the same on both sides the
line ends in `{A: unit, B: unit}`.

A revision is anything `git archive` takes, or WORKTREE for the files as they are on disk.  Every unit is compiled at its revision with that revision's Makefile
FLAGS plus `--cuda-device-only -S`; the assembly is split per kernel (its label up to `.end_amdhsa_kernel`: the instruction stream and the `.amdhsa_*` descriptor --
registers, accumulation offset, LDS and scratch bytes) and one line per kernel is printed:

    identical      same name at both revisions, same code
    identical (A: <name>)   a kernel whose name changed (template parameters went) with the same code as that kernel of REV_A
    differs        same name, other code (`--show` prints the diff)
    only-in-A / only-in-B

What is normalised before the comparison, and nothing else: the kernel's own mangled name, the function index inside local labels (.LBB14_22 -> .LBB_22, .Ltmp and
.Lfunc_* likewise), trailing `;` comments, `.p2align` lines.  Exit status 1 if a kernel differs or exists at REV_B only.
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "svt-av1_amd/csrc"


def checkout(rev, dst):
    """The sources a unit needs (csrc + include) of `rev` under dst."""
    if rev == "WORKTREE":
        shutil.copytree(os.path.join(ROOT, CSRC), os.path.join(dst, CSRC), ignore=shutil.ignore_patterns("build"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(dst, "include"))
        return
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)


def compile_units(rev, side, units, work):
    """{mangled name: (unit, normalised lines)} over `units` of `rev`, and the seconds the compiler took."""
    dst = os.path.join(work, side)
    os.makedirs(dst)
    checkout(rev, dst)
    csrc = os.path.join(dst, CSRC)
    flags = None
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"FLAGS\s*:?=\s*(.*)", line)
        if m:
            flags = m.group(1).split()
    if flags is None:
        sys.exit(f"{rev}: no FLAGS in the Makefile")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def one(unit):
        out = os.path.join(dst, unit + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", out], check=True)
        return kernels(open(out).read())

    t0 = time.time()
    with ThreadPoolExecutor(4) as ex:
        per_unit = list(ex.map(one, units))
    pool = {}
    for unit, ks in zip(units, per_unit):
        for name, body in ks.items():
            if name in pool:
                sys.exit(f"{rev}: {demangle([name])[name]} is defined by {pool[name][0]} and by {unit}")
            pool[name] = (unit, body)
    return pool, time.time() - t0


def kernels(asm):
    """{mangled name: normalised lines} of every kernel of an assembly file."""
    lines = asm.split("\n")
    label = {}
    for i, l in enumerate(lines):
        m = re.match(r"([A-Za-z_$.][\w$.]*):", l)
        if m:
            label.setdefault(m.group(1), i)
    out = {}
    for j, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        end = next(k for k in range(j, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        body = []
        for l2 in lines[label[name]:end + 1]:
            l2 = l2.replace(name, "KERNEL").replace(name[2:], "KERNEL")   # the second form: statics of the kernel (_ZZ<name>E..)
            l2 = re.sub(r"\s*;.*$", "", l2).rstrip()
            l2 = re.sub(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", l2)
            if not l2.strip() or l2.strip().startswith(".p2align"):
                continue
            body.append(l2)
        out[name] = body
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::", "", d) for n, d in zip(names, res)}


def descriptor(body):
    want = {".amdhsa_next_free_vgpr": "vgpr", ".amdhsa_accum_offset": "accum", ".amdhsa_group_segment_fixed_size": "lds", ".amdhsa_private_segment_fixed_size": "scratch"}
    got = {}
    for l in body:
        p = l.split()
        if len(p) == 2 and p[0] in want:
            got[want[p[0]]] = p[1]
    return " ".join(f"{k}={got[k]}" for k in ("vgpr", "accum", "lds", "scratch") if k in got)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev_a")
    ap.add_argument("rev_b")
    ap.add_argument("unit", nargs="?", help="a .hip file of " + CSRC + " (both sides)")
    ap.add_argument("--units-a", nargs="+", metavar="UNIT", help="the units of REV_A whose kernels are pooled")
    ap.add_argument("--units-b", nargs="+", metavar="UNIT", help="the units of REV_B whose kernels are pooled")
    ap.add_argument("--show", action="store_true", help="print the diff of kernels that differ")
    a = ap.parse_args()
    if bool(a.unit) == bool(a.units_a or a.units_b):
        ap.error("give UNIT, or --units-a / --units-b")
    units_a, units_b = a.units_a or a.units_b or [a.unit], a.units_b or a.units_a or [a.unit]
    for units in (units_a, units_b):
        if len(set(units)) != len(units):
            ap.error("a unit is listed twice: " + " ".join(units))
    work = tempfile.mkdtemp(prefix="isa_diff_")
    try:
        with ThreadPoolExecutor(2) as ex:
            fa, fb = ex.submit(compile_units, a.rev_a, "A", units_a, work), ex.submit(compile_units, a.rev_b, "B", units_b, work)
            (ka, ta), (kb, tb) = fa.result(), fb.result()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    names = demangle(sorted(set(ka) | set(kb)))
    bad = 0
    left_a = {n for n in ka if n not in kb}
    print(f"# A = {a.rev_a} {' '.join(units_a)} ({len(ka)} kernels, compiled in {ta:.0f} s), B = {a.rev_b} {' '.join(units_b)} ({len(kb)} kernels, {tb:.0f} s)")
    pooled = len(units_a) > 1 or len(units_b) > 1

    def where(na, nb):   # the units, where they are not the same one
        ua, ub = ka[na][0] if na else None, kb[nb][0] if nb else None
        if na and nb:
            return "" if ua == ub else f"  {{A: {ua}, B: {ub}}}"
        return f"  {{{ua or ub}}}" if pooled else ""

    for n in sorted(kb, key=lambda n: names[n]):
        body = kb[n][1]
        if n in ka:
            same = ka[n][1] == body
            print(f"{'identical' if same else 'differs  '}  {names[n]}  [{descriptor(body)}]{where(n, n)}")
            if not same:
                bad += 1
                if a.show:
                    sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(ka[n][1], body, "A", "B", lineterm="", n=2))
            continue
        twin = next((m for m in sorted(left_a) if ka[m][1] == body), None)   # renamed: the same code under another name
        if twin:
            left_a.discard(twin)
            print(f"identical  {names[n]}  [{descriptor(body)}]  (A: {names[twin]}){where(twin, n)}")
        else:
            bad += 1
            print(f"only-in-B  {names[n]}  [{descriptor(body)}]{where(None, n)}")
    for n in sorted(left_a, key=lambda n: names[n]):
        print(f"only-in-A  {names[n]}  [{descriptor(ka[n][1])}]{where(n, None)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
