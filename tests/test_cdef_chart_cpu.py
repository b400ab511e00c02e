"""The direction-chart frames (cdef_common.make_chart_frame) that the CDEF GPU tests run on: what they cover is a checked condition, not a hope.
Oracle only (orc_cdef_find_dir, pinned to svt_cdef_find_dir_c by test_oracle_vs_ref.py); no GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import ptr
import cdef_common as cc

# (w, h), bd, seed: exactly the frames of test_cdef_gpu.py's chart tests
CHART_CASES = [(size, bd, cc.CHART_SEED) for size in cc.CHART_SIZES for bd in (8, 10)]


def chart_stats(orc, w, h, bd, seed):
    src, rec, skip8 = cc.make_chart_frame(w, h, bd, seed)
    o_dir, o_var = cc.orc_find_dir_frame(orc, rec[0], bd)
    cost, n_dir, n_var = cc.find_dir_costs(cc.luma_blocks(rec[0]).reshape(-1, 8, 8), bd - 8)
    live = skip8.reshape(-1) == 0
    top = cost.max(axis=1)
    tie = ((cost == top[:, None]).sum(axis=1) > 1) & (top > 0)      # an exact tie for the (non-zero) best cost
    return dict(rec=rec, src=src, skip8=skip8, o_dir=o_dir.reshape(-1), o_var=o_var.reshape(-1), n_dir=n_dir, n_var=n_var, live=live, tie=tie)


@pytest.mark.parametrize("size,bd,seed", CHART_CASES)
def test_chart_coverage(orc, size, bd, seed):
    w, h = size
    s = chart_stats(orc, w, h, bd, seed)
    # the numpy statement of the eight costs agrees with the oracle on every block, ties included
    assert np.array_equal(s["n_dir"], s["o_dir"]) and np.array_equal(s["n_var"], s["o_var"])
    live = s["live"]
    d, v = s["o_dir"][live], s["o_var"][live]
    per_dir = np.bincount(d, minlength=8)
    flat = int((v == 0).sum())
    i_seen = sorted(set(cc.strength_i(v[v != 0]).tolist()))
    ties = int((s["tie"][live] & (d != 0)).sum())
    print(f"chart {w}x{h} {bd}-bit seed {seed}: live {int(live.sum())}, per direction {per_dir.tolist()}, var == 0: {flat}, i: {i_seen}, "
          f"ties won by a direction != 0: {ties}")
    mx = (1 << bd) - 1
    for pli, p in enumerate(s["rec"]):   # 0 and max within 2 samples of each picture edge: the clamps meet CDEF_VERY_LARGE neighbours at both ends of the range
        for name, strip in (("top", p[:2]), ("bottom", p[-2:]), ("left", p[:, :2]), ("right", p[:, -2:])):
            assert (strip == 0).any() and (strip == mx).any(), (pli, name)
    sk = s["skip8"]
    assert not (sk[0, 0] or sk[0, -1] or sk[-1, 0] or sk[-1, -1])
    fb_live = [int((sk[8 * r:8 * r + 8, 8 * c:8 * c + 8] == 0).sum()) for r in range((h + 63) // 64) for c in range((w + 63) // 64)]
    assert 1 in fb_live
    # anti-correlated and identical regions of the source
    assert np.array_equal(s["src"][0][:h // 3, :w // 3], mx - s["rec"][0][:h // 3, :w // 3])
    assert np.array_equal(s["src"][0][h // 3:2 * h // 3, 2 * w // 3:], s["rec"][0][h // 3:2 * h // 3, 2 * w // 3:])
    if w * h < 8 * 8 * 4 * len(cc.CHART_CYCLE):
        return                          # too small to hold the kind cycle often enough: exempt from the counts
    assert 0 in fb_live                 # one filter block without a live block
    assert per_dir.min() >= 10, per_dir
    assert flat >= 20
    assert i_seen == list(range(13)), i_seen
    assert ties >= 10


def test_chart_cells_decide_what_they_claim(orc):
    """One cell of every kind, as the per-call tests take them (cdef_common.chart_kind_cells).  A line sum weighs 840 / (samples on the line), so
    840 * sum(x^2) bounds every cost and a cell constant along direction d reaches it: d wins.  Tie cells tie exactly between d and 8 - d at the
    maximum and the lower index wins; flat cells have eight equal costs."""
    for bd in (8, 10):
        seen = set()
        for kind, cell in cc.chart_kind_cells(bd):
            assert cell.shape == (8, 8) and cell.min() >= 0 and cell.max() < (1 << bd), kind
            cost, best, var = cc.find_dir_costs(cell[None], bd - 8)
            cost, best, var = cost[0], int(best[0]), int(var[0])
            v = C.c_int32(0)
            assert (orc.orc_cdef_find_dir(ptr(np.ascontiguousarray(cell.astype(np.uint16))), 8, C.byref(v), bd - 8), v.value) == (best, var), kind
            x = (cell >> (bd - 8)) - 128
            bound = 840 * int((x * x).sum())
            assert cost.max() <= bound
            if kind[0] in ("bin", "lvl"):
                assert cost[kind[1]] == bound and best == kind[1] and var > 0, kind
            elif kind[0] == "tie":
                assert cost[kind[1]] == cost[8 - kind[1]] == cost.max() and best == kind[1], kind
                assert var == 0 if kind[1] == 2 else var > 0, kind     # 2 ties with its own orthogonal direction 6: a directed block of variance 0
            elif kind[0] == "flat":
                assert (cost == cost[0]).all() and (best, var) == (0, 0), kind
            seen.add(best)
        assert seen == set(range(8))
