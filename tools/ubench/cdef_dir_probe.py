"""What does the direction search cost inside cdef_search_luma_kernel<uint8_t>?  Builds two timing libraries from a PATCHED COPY of cdef.hip (the product file is
not touched), both without the chroma launch, so that the search entry point times the luma kernel alone:

    variant 0   the luma kernel as it is
    variant 1   no direction search: a block takes the direction and variance that the launch's dir / var buffers already hold (the script fills them with the
                right values first, so everything after the direction search does the same work in both variants; with one constant for all blocks it would
                not: the direction picks the B-part shortcut and the variance the number of distinct strengths)

and times both on a 3840x2160 8-bit picture (cdef_common.make_frame, noisy, 30 % of the blocks skipped), 20 launches under the library's event timer.
Variant 0 - variant 1 is what the direction search costs per launch: the ceiling of any work on it.  Variant 1 is a clock, not a check.

    python tools/ubench/cdef_dir_probe.py build     # here: the two libraries under tools/ubench/probe_bin/ (needs the built tree: the other units' objects)
    python tools/ubench/cdef_dir_probe.py run       # on the GPU box: one child process per variant, one line each"""
import ctypes as C
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
CSRC = os.path.join(ROOT, "svt-av1_amd", "csrc")
BIN = os.path.join(HERE, "probe_bin")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off -Wno-unused-function -Wno-bitwise-instead-of-logical".split()


def lib_path(v):
    return os.path.join(BIN, f"libsvtav1_hip_dirprobe{v}.so")


def patched():
    t = open(os.path.join(CSRC, "cdef.hip")).read()

    def rep(old, new):
        nonlocal t
        assert t.count(old) == 1, old
        t = t.replace(old, new)

    rep("        dir16 = find_dir_batch16(tile + (8 * by + 2 * (lane >> 4) + kVB) * TS + 8 * bx + kHB, TS, live, cs, lane, var16);\n",
        "#if DIR_PROBE\n        dir16 = dir_out[fb * 64 + b]; var16 = var_out[fb * 64 + b];\n#else\n"
        "        dir16 = find_dir_batch16(tile + (8 * by + 2 * (lane >> 4) + kVB) * TS + 8 * bx + kHB, TS, live, cs, lane, var16);\n#endif\n")
    rep("        hipLaunchKernelGGL((cdef_search_chroma_kernel<PIX>), ", "        if (0) hipLaunchKernelGGL((cdef_search_chroma_kernel<PIX>), ")
    return t


def build():
    os.makedirs(BIN, exist_ok=True)
    src = os.path.join(BIN, "cdef_dirprobe.hip")
    open(src, "w").write(patched())
    others = [o for o in glob.glob(os.path.join(CSRC, "build", "*.o")) if os.path.basename(o) != "cdef.o"]
    assert others, "build the tree first"
    for v in (0, 1):
        obj = os.path.join(BIN, f"cdef_dirprobe{v}.o")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + [f"-DDIR_PROBE={v}", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj])
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-o", lib_path(v), obj] + others)
        print("built", lib_path(v))


def child(v):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_package
    import cdef_common as cc
    pkg = load_package()
    pkg.LIB_PATH = lib_path(v)
    hip = pkg.Context(0)
    W, H = 3840, 2160
    src, rec, skip8 = cc.make_frame(W, H, 8, seed=77, smooth=False)
    nv, nh = (H + 63) // 64, (W + 63) // 64
    _, best, var = cc.find_dir_costs(cc.luma_blocks(rec[0]).reshape(-1, 8, 8), 0)
    live = (skip8 == 0).reshape(-1)
    fb_dir = np.zeros((nv * 8, nh * 8), np.int64); fb_var = np.zeros((nv * 8, nh * 8), np.int64)
    fb_dir[:H // 8, :W // 8] = (best * live).reshape(H // 8, W // 8); fb_var[:H // 8, :W // 8] = (var * live).reshape(H // 8, W // 8)
    in_fb = lambda a, dt: np.ascontiguousarray(a.reshape(nv, 8, nh, 8).swapaxes(1, 2).reshape(-1).astype(dt))
    e_dir, e_var = in_fb(fb_dir, np.uint8), in_fb(fb_var, np.int32)
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    d_rec = [hip.to_device(p) for p in rec]; d_src = [hip.to_device(p) for p in src]
    d_skip, d_mse = hip.to_device(skip8), hip.to_device(np.zeros((2, nv * nh, 64), np.uint64))
    d_dir, d_var = hip.to_device(e_dir), hip.to_device(e_var)
    strides = I3(*[p.shape[1] for p in rec])

    def go():
        hip.check(hip.L.svt_hip_cdef_search_frame_dev(hip.h, 1, P3(*[p.value for p in d_rec]), strides, P3(*[p.value for p in d_src]), strides, W, H, d_skip, 4, 8,
                                                     d_mse, d_dir, d_var), "cdef search")

    ms = C.c_float()
    for _ in range(3): go()
    hip.L.svt_hip_timer_start(hip.h)
    for _ in range(20): go()
    hip.L.svt_hip_timer_stop_ms(hip.h, C.byref(ms))
    same = np.array_equal(hip.to_host(d_dir, e_dir.shape, np.uint8), e_dir) and np.array_equal(hip.to_host(d_var, e_var.shape, np.int32), e_var)
    mse = hip.to_host(d_mse, (2, nv * nh, 64), np.uint64)
    print(f"DIR_PROBE={v}  {ms.value * 1000 / 20:8.1f} us per luma launch   dir / var as expected: {same}   luma table checksum {int(mse[0].sum() % (1 << 32)):#010x}", flush=True)
    hip.close()


def run():
    for v in (0, 1, 0, 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(v)], capture_output=True, text=True, timeout=300)
        print(r.stdout.strip() or r.stderr[-800:], flush=True)
        if r.returncode:
            sys.exit(r.returncode)   # nothing more on the GPU after a child that failed


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(int(sys.argv[2]))
    else:
        {"build": build, "run": run}[sys.argv[1]]()
