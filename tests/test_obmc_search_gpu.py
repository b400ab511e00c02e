"""GPU: svt_hip_obmc_target_batch_dev and svt_hip_obmc_search_batch_dev against the numpy restatement (tests/obmc_common.py), which
tests/test_obmc_search_ref_cpu.py pins to the reference: every wsrc / mask value of the full target case lists in one launch per picture, the same arrays fed
unchanged to the existing svt_hip_obmc_cost_batch_dev, every field of every search result, empty lists, and the two stages back to back on one stream with no
synchronisation between them.  Integers only: no tolerance.  A 96 x 64 picture with 80 samples of border for the sizes up to 64 x 64, a 128 x 128 picture with 144
for the three 128-wide sizes; the conditions these lists exist for are asserted on the CPU."""
import ctypes as C

import numpy as np
import pytest

import obmc_common as S
import test_obmc_search_abi as abi

pytestmark = pytest.mark.gpu
FILL = 0xC3
FILL_WORD = int(np.frombuffer(bytes([FILL] * 4), np.int32)[0])


def search_args(pkg, case, jobs=None):
    return dict(picture=S.picture_view(case), pad_w=case["pad_w"], pad_h=case["pad_h"], mi_rows=case["mi_rows"], mi_cols=case["mi_cols"], joint_cost=case["jc"],
                comp_cost=case["cc"], jobs=S.c_search_jobs(pkg, case["jobs"] if jobs is None else jobs))


def check_results(pkg, res, case, want):
    n = len(case["jobs"])
    for k, (r, w) in enumerate(zip(S.results_as_dicts(res, n), want)):
        assert r == w, (k, case["specs"][k])
    # every field of every result was written
    assert not (np.frombuffer(bytes(res), np.uint32)[:n * len(S.RESULT_FIELDS)] == FILL_WORD & 0xFFFFFFFF).any()


@pytest.mark.parametrize("which", ["small", "big"])
def test_target_equals_the_restatement(hip, pkg, which):
    case, (wsrc, mask), _ = S.cached("target", which)
    got_w, got_m, none = hip.obmc_batch(case["plane"], case["nbr"], S.c_target_jobs(pkg, case["jobs"]), case["wm_samples"], fill=FILL)
    assert none is None and (got_w == wsrc).all() and (got_m == mask).all()


def test_target_output_feeds_the_obmc_cost_kernel(hip, pkg):
    """the arrays of stage 1 stay on the device and go to svt_hip_obmc_cost_batch_dev as they are; sad and variance of the block of a plane at the job's position"""
    case, (wsrc, mask), _ = S.cached("target", "small")
    h, w = case["plane"].shape
    pre = np.random.default_rng(11).integers(0, 256, (h + 1, w + 1)).astype(np.uint8)   # readable one sample right / below of every block
    jobs = case["jobs"]
    blks = (pkg.ObmcBlk * len(jobs))(*[pkg.ObmcBlk(j["x"], j["y"], S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]], 0, 0, j["wm_off"]) for j in jobs])
    tj = S.c_target_jobs(pkg, jobs)
    with hip.scope() as s:
        p, d_n, d_pre, d_blk = s.plane(case["plane"]), s.upload(case["nbr"]), s.upload(pre), s.structs(blks)
        d_w, d_m = s.filled(case["wm_samples"] * 4, FILL, np.uint8), s.filled(case["wm_samples"] * 4, FILL, np.uint8)
        d_out = s.filled(3 * len(jobs), 0xC3C3C3C3, np.uint32)
        hip.call("obmc_target_batch_dev", p.ptr, p.stride, w, h, d_n, case["nbr"].size, C.cast(tj, C.c_void_p), len(jobs), d_w, d_m, case["wm_samples"])
        hip.call("obmc_cost_batch_dev", d_pre, pre.shape[1], d_w, d_m, d_blk, len(jobs), d_out)
        hip.sync()
        out = s.download(d_out, (len(jobs), 3), np.uint32)
    for k, j in enumerate(jobs):
        bw, bh = S.BLOCK_W[j["bsize"]], S.BLOCK_H[j["bsize"]]
        blk = pre[j["y"]:j["y"] + bh, j["x"]:j["x"] + bw]
        wm = slice(j["wm_off"], j["wm_off"] + bw * bh)
        var, sse = S.obmc_variance(blk, wsrc[wm].reshape(bh, bw), mask[wm].reshape(bh, bw))
        assert out[k].tolist() == [S.obmc_sad(blk, wsrc[wm].reshape(bh, bw), mask[wm].reshape(bh, bw)), sse, var], (k, case["specs"][k])


@pytest.mark.parametrize("which", ["small", "big"])
def test_search_equals_the_restatement(hip, pkg, which):
    case, want, _ = S.cached("search", which)
    _, _, res = hip.obmc_batch(search=search_args(pkg, case), wsrc=case["wsrc"], mask=case["mask"], fill=FILL)
    check_results(pkg, res, case, want)


def test_target_then_search_on_one_stream_without_synchronisation(hip, pkg):
    """stage 2 reads what stage 1 wrote, ordered by the stream alone"""
    case, want, _ = S.cached("search", "small")
    t = case["target"]
    got_w, got_m, res = hip.obmc_batch(t["plane"], t["nbr"], S.c_target_jobs(pkg, t["jobs"]), t["wm_samples"], search=search_args(pkg, case), fill=FILL)
    assert (got_w == case["wsrc"]).all() and (got_m == case["mask"]).all()
    check_results(pkg, res, case, want)


def test_empty_lists(hip, pkg):
    case, _, _ = S.cached("search", "small")
    t = case["target"]
    got_w, got_m, res = hip.obmc_batch(t["plane"], t["nbr"], S.c_target_jobs(pkg, []), 64, search=search_args(pkg, case, jobs=[]), fill=FILL)
    assert (got_w == FILL_WORD).all() and (got_m == FILL_WORD).all()
    assert (np.frombuffer(bytes(res), np.uint8) == FILL).all()   # nothing written


def test_bad_arguments_with_a_live_context(hip, pkg):
    """the refusals of tests/test_obmc_search_abi.py once more, with a context: refused the same, with a text that names the entry point"""
    buf = np.zeros(1 << 20, np.uint8)
    with hip.scope() as s:
        p = C.c_void_p(s.upload(buf).value + (1 << 19))
        for c in abi.TARGET_BAD[:6] + abi.SEARCH_BAD[:6]:
            kind = "target" if c in abi.TARGET_BAD else "search"
            assert abi.call(pkg, kind, hip.h, p, **c) == abi.BAD_ARG, c
            assert pkg.lib().svt_hip_last_error(hip.h).decode().startswith("svt_hip_obmc_%s_batch_dev: " % kind)
