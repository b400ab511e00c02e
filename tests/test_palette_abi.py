"""CPU: the palette search and the screen-content detection are declared, exported and bound (prototypes and layouts against the header:
tests/test_abi_binding.py), the header compiles as C99 with them, and calls the host can see to be wrong are refused with SVT_HIP_ERR_BAD_ARG before anything
touches HIP (no device exists here: a call that reached the runtime would fail differently or crash).  The same bad arguments with a live context:
tests/test_palette_gpu.py and tests/test_screen_content_gpu.py."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

BAD_ARG = 2   # SVT_HIP_ERR_BAD_ARG
ENTRY_POINTS = ("svt_hip_palette_search_batch_dev", "svt_hip_palette_search_host", "svt_hip_screen_content_detect_dev")


def test_declared_exported_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    assert re.search(r"SVT_HIP_ERR_BAD_ARG\s*=\s*%d\b" % BAD_ARG, hdr)
    assert re.search(r"#define\s+SVT_HIP_PALETTE_MAX_CANDS\s+%d\b" % pkg.PALETTE_MAX_CANDS, hdr)
    for m in ("palette_search_batch", "screen_content_detect"):
        assert hasattr(pkg.Context, m)
    assert callable(pkg.palette_search_host)
    for f in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % f, hdr) and f in pkg.PROTOTYPES and hasattr(pkg.lib(), f)
    assert [n for n, _ in pkg.PaletteJob._fields_] == ["x", "y", "bw", "bh", "cols", "rows", "n_cache", "dominant_step", "cache", "map_off"]
    assert [n for n, _ in pkg.PaletteResult._fields_] == ["colors", "n_cands"]
    assert [n for n, _ in pkg.PaletteCand._fields_] == ["color_cost", "colors", "raw", "size", "n", "kind", "reserved"]
    # the intra batch entry point still does no palette; the sentence that says so stays, and the new entry point says what it leaves out
    assert "palette and intra block copy are\n * not covered" in hdr
    assert "Palette chroma, the colour-map rate (svt_av1_cost_color_map) and intra block copy are not covered" in hdr


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "svt_hip.h"\nint main(void){SvtHipPaletteJob j = {0}; SvtHipPaletteResult r = {0}; SvtHipPaletteCand c = {0}; j.cache[15] = 1; c.raw[7] = 2;\n'
                   "return (int)sizeof(&svt_hip_palette_search_batch_dev) + (int)sizeof(&svt_hip_palette_search_host) + (int)sizeof(&svt_hip_screen_content_detect_dev) +"
                   " j.cache[15] + c.raw[7] + r.n_cands + SVT_HIP_PALETTE_MAX_CANDS == 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


# one thing wrong at a time; shared with the GPU tests, which repeat them with a live context.  1 = "a valid pointer"
SEARCH_OK = dict(pix_bytes=1, bd=8, d_plane=1, stride=64, d_jobs=1, njobs=1, d_results=1, d_cands=1, d_maps=1)
SEARCH_BAD = [dict(d_plane=None), dict(d_jobs=None), dict(d_results=None), dict(d_cands=None), dict(d_maps=None), dict(njobs=-1), dict(stride=0), dict(stride=-64),
              dict(pix_bytes=0), dict(pix_bytes=3), dict(bd=10), dict(bd=12), dict(pix_bytes=2, bd=9), dict(pix_bytes=2, bd=12)]
DETECT_OK = dict(pix_bytes=1, bd=8, d_plane=1, stride=64, width=64, height=32, d_out=1)
DETECT_BAD = [dict(d_plane=None), dict(d_out=None), dict(stride=0), dict(stride=-64), dict(width=0), dict(width=-16), dict(height=0), dict(height=-16), dict(pix_bytes=0),
              dict(pix_bytes=3), dict(bd=10), dict(pix_bytes=2, bd=8), dict(pix_bytes=2, bd=12), dict(width=65536, height=65536)]


def call_search(L, ctx, p, **chg):
    """`p` stands in for every pointer that is 1 in SEARCH_OK"""
    a = dict(SEARCH_OK); a.update(chg)
    q = lambda k: p if a[k] == 1 else a[k]
    return L.svt_hip_palette_search_batch_dev(ctx, a["pix_bytes"], a["bd"], q("d_plane"), a["stride"], q("d_jobs"), a["njobs"], q("d_results"), q("d_cands"), q("d_maps"))


def call_detect(L, ctx, p, **chg):
    a = dict(DETECT_OK); a.update(chg)
    q = lambda k: p if a[k] == 1 else a[k]
    return L.svt_hip_screen_content_detect_dev(ctx, a["pix_bytes"], a["bd"], q("d_plane"), a["stride"], a["width"], a["height"], q("d_out"))


def test_null_context_and_bad_arguments_are_refused(pkg):
    L = pkg.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    for c in [{}] + SEARCH_BAD:
        assert call_search(L, None, p, **c) == BAD_ARG, c
    for c in [{}] + DETECT_BAD:
        assert call_detect(L, None, p, **c) == BAD_ARG, c
