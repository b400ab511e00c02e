"""OBMC in mode decision, restated in numpy / plain Python from the reference's text, pass by pass and probe by probe in its order (file:line under Source/Lib):
calc_target_weighted_pred with its two visitors (Encoder/Codec/EbEncInterPrediction.c:2376-2437, :2196-2256), foreach_overlappable_nb_above / _left (:918-996),
single_motion_search (Encoder/Codec/EbModeDecision.c:2951-3036), svt_av1_obmc_full_pixel_search with obmc_refining_search_sad and get_obmc_mvpred_var
(Encoder/Codec/av1me.c:776-855), svt_av1_find_best_obmc_sub_pixel_tree_up (:1069-1254) on upsampled_obmc_pref_error (:973-1035) = svt_aom_upsampled_pred_c
(Encoder/C_DEFAULT/variance.c:212-269) + svt_aom_obmc_variance{W}x{H}_c (:270-299), svt_aom_obmc_sad{W}x{H}_c (sad_av1.c:18-38), mv_err_cost / mvsad_err_cost
(av1me.c:273-290) and svt_av1_mv_bit_cost (EbRateDistortionCost.c:85-99).  The library computes the target per sample and a step's probes before its decisions
(csrc/obmc_search.h); here nothing is rearranged.  Plus the case lists the CPU, ABI and GPU tests share; tests/test_obmc_search_ref_cpu.py asserts what they contain."""
import ctypes as C
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obmc_search.npz")
BLOCK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BLOCK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]
SIZES = [b for b in range(22) if min(BLOCK_W[b], BLOCK_H[b]) >= 8]   # is_motion_variation_allowed_bsize
SMALL_SIZES = [b for b in SIZES if max(BLOCK_W[b], BLOCK_H[b]) <= 64]
BIG_SIZES = [b for b in SIZES if b not in SMALL_SIZES]
BSIZE_OF = {(BLOCK_W[b], BLOCK_H[b]): b for b in range(22)}
# the specification's Obmc_Mask_N
OBMC_MASK = {1: [64], 2: [45, 64], 4: [39, 50, 59, 64], 8: [36, 42, 48, 53, 57, 61, 64, 64], 16: [34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64],
             32: [33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64],
             64: [33, 34, 35, 35, 36, 37, 38, 39, 40, 40, 41, 42, 43, 44, 44, 44, 45, 46, 47, 47, 48, 49, 50, 51, 51, 51, 52, 52, 53, 54, 55, 56,
                  56, 56, 57, 57, 58, 58, 59, 60, 60, 60, 60, 60, 61, 62, 62, 62, 62, 62, 63, 63, 63, 63, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64]}
# EIGHTTAP_REGULAR at the eight 1/8 positions
TAPS = np.array([[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 76, 76, -14, 2, 0],
                 [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -10, 38, 110, -14, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0]], np.int64)
MV_VALS, MV_MAX = 32767, 16383
INT_MAX, U32 = (1 << 31) - 1, (1 << 32) - 1
MAX_FULL_PEL_VAL, MV_LOW, MV_UPP, INTERP_EXTEND = 1023, -(1 << 14), 1 << 14, 4
MAX_NEIGHBOR_OBMC = [0, 1, 2, 3, 4, 4]
TARGET_FIELDS = ("bsize", "x", "y", "n_above", "above_rel", "above_len", "n_left", "left_rel", "left_len", "above_off", "above_stride", "left_off", "left_stride", "wm_off")
JOB_FIELDS = ("bsize", "mi_row", "mi_col", "wm_off", "mv_row", "mv_col", "ref_mv_row", "ref_mv_col", "sad_per_bit", "error_per_bit", "allow_hp")
RESULT_FIELDS = ("status", "full_row", "full_col", "refining", "steps", "bestsme", "row", "col", "besterr", "distortion", "sse", "rate_mv")


def to_int(v):
    """(int) of a 64-bit value, as the reference's compilers give it"""
    v &= U32
    return v - (1 << 32) if v > INT_MAX else v


# ------------------------------------------------------------------------------------------------------------------ the neighbour lists
def neighbours(sb_side, flags, n4, pos, end):
    """foreach_overlappable_nb_above / _left on one side: sb_side[i] = mi_size_wide / _high of the neighbour at unit i of the edge, flags[i] = is_neighbor_overlappable.
    -> [(rel, len)] as the visitor is called"""
    out = []
    nb_max = MAX_NEIGHBOR_OBMC[n4.bit_length() - 1]
    at, last = pos, min(pos + n4, end)
    while at < last and len(out) < nb_max:
        pick = at - pos
        step = min(sb_side[pick], 16)
        if step == 1:
            at &= ~1
            pick = at - pos + 1
            step = 2
        if flags[pick]:
            out.append((at - pos, min(n4, step)))
        at += step
    return out


# ------------------------------------------------------------------------------------------------------------------ the weighted target
def target(src, above, left, segs_above, segs_left, bw, bh):
    """calc_target_weighted_pred: `src` the block's source samples (bh x bw), `above` / `left` 2-D arrays addressed [row, column] from the block's corner.
    -> (wsrc, mask) as int32 bh x bw"""
    wsrc, mask = np.zeros((bh, bw), np.int64), np.full((bh, bw), 64, np.int64)
    overlap = min(bh, 64) >> 1
    m1d = OBMC_MASK[overlap]
    for rel, length in segs_above:
        for row in range(overlap):
            m0 = m1d[row]
            cols = slice(rel * 4, rel * 4 + length * 4)
            wsrc[row, cols] = (64 - m0) * above[row, cols].astype(np.int64)
            mask[row, cols] = m0
    wsrc *= 64
    mask *= 64
    overlap = min(bw, 64) >> 1
    m1d = OBMC_MASK[overlap]
    for rel, length in segs_left:
        for row in range(rel * 4, rel * 4 + length * 4):
            for col in range(overlap):
                m0 = m1d[col]
                wsrc[row, col] = (wsrc[row, col] >> 6) * m0 + (int(left[row, col]) << 6) * (64 - m0)
                mask[row, col] = (mask[row, col] >> 6) * m0
    wsrc = src.astype(np.int64) * 4096 - wsrc
    return wsrc.astype(np.int32), mask.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the leaves
def obmc_sad(pre, wsrc, mask):
    return int(((np.abs(wsrc.astype(np.int64) - pre.astype(np.int64) * mask) + 2048) >> 12).sum()) & U32


def obmc_variance(pre, wsrc, mask):
    """-> (variance, sse) as unsigned 32-bit values"""
    v = wsrc.astype(np.int64) - pre.astype(np.int64) * mask
    d = np.where(v < 0, -((-v + 2048) >> 12), (v + 2048) >> 12)
    total, sse = int(d.sum()), int((d * d).sum()) & U32
    return (sse - ((total * total) // d.size & U32)) & U32, sse   # sum * sum >= 0: // is C's division


def clip_round7(v):
    return np.clip((v + 64) >> 7, 0, 255)


def upsampled_pred(plane, y, x, bw, bh, sx, sy):
    """svt_aom_upsampled_pred_c with USE_8_TAPS: the block at [y, x] of `plane` (an array that holds the border), sub-pel position (sx, sy) in 1/8 sample"""
    p = plane.astype(np.int64)
    if not sx and not sy:
        return p[y:y + bh, x:x + bw]
    if not sy:
        return clip_round7(sum(TAPS[sx][k] * p[y:y + bh, x + k - 3:x + k - 3 + bw] for k in range(8)))
    if not sx:
        return clip_round7(sum(TAPS[sy][k] * p[y + k - 3:y + k - 3 + bh, x:x + bw] for k in range(8)))
    temp = clip_round7(sum(TAPS[sx][k] * p[y - 3:y + bh + 4, x + k - 3:x + k - 3 + bw] for k in range(8)))   # intermediate_height = bh + 7
    return clip_round7(sum(TAPS[sy][k] * temp[k:k + bh] for k in range(8)))


def mv_cost(d_row, d_col, jc, cc):
    joint = (0 if d_col == 0 else 1) if d_row == 0 else (2 if d_col == 0 else 3)
    return int(jc[joint]) + int(cc[0][MV_MAX + d_row]) + int(cc[1][MV_MAX + d_col])


def mv_err_cost(row, col, ref_row, ref_col, jc, cc, error_per_bit):
    return to_int((mv_cost(row - ref_row, col - ref_col, jc, cc) * error_per_bit + (1 << 13)) >> 14)


def mvsad_err_cost(row, col, fref_row, fref_col, jc, cc, sad_per_bit):
    return ((((mv_cost((row - fref_row) * 8, (col - fref_col) * 8, jc, cc) & U32) * sad_per_bit & U32) + 256) & U32) >> 9


def mv_bit_cost(row, col, ref_row, ref_col, jc, cc, weight=108):
    clamp = lambda v: max(MV_LOW, min(MV_UPP, v))
    return (mv_cost(clamp(row - ref_row), clamp(col - ref_col), jc, cc) * weight + 64) >> 7


# ------------------------------------------------------------------------------------------------------------------ limits
def block_limits(job, mi_rows, mi_cols):
    """-> (col_min, col_max, row_min, row_max) of single_motion_search"""
    mi_w, mi_h = BLOCK_W[job["bsize"]] // 4, BLOCK_H[job["bsize"]] // 4
    return (-((job["mi_col"] + mi_w) * 4 + INTERP_EXTEND), (mi_cols - job["mi_col"]) * 4 + INTERP_EXTEND, -((job["mi_row"] + mi_h) * 4 + INTERP_EXTEND),
            (mi_rows - job["mi_row"]) * 4 + INTERP_EXTEND)


def search_range(lim, ref_row, ref_col):
    """svt_av1_set_mv_search_range"""
    col_min = max((ref_col >> 3) - MAX_FULL_PEL_VAL + (1 if ref_col & 7 else 0), (MV_LOW >> 3) + 1)
    row_min = max((ref_row >> 3) - MAX_FULL_PEL_VAL + (1 if ref_row & 7 else 0), (MV_LOW >> 3) + 1)
    col_max, row_max = min((ref_col >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1), min((ref_row >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1)
    return max(lim[0], col_min), min(lim[1], col_max), max(lim[2], row_min), min(lim[3], row_max)


def subpel_range(lim, ref_row, ref_col):
    """set_subpel_mv_search_range -> (minc, maxc, minr, maxr)"""
    max_mv = MAX_FULL_PEL_VAL * 8
    return (max(MV_LOW + 1, lim[0] * 8, ref_col - max_mv), min(MV_UPP - 1, lim[1] * 8, ref_col + max_mv), max(MV_LOW + 1, lim[2] * 8, ref_row - max_mv),
            min(MV_UPP - 1, lim[3] * 8, ref_row + max_mv))


def plane_covers(job, lim, width, height, pad_w, pad_h):
    """the border covers what the walk could read under the narrowed limits `lim`: the limits, one more whole sample, the filter's -3 .. +4"""
    bw, bh, x0, y0 = BLOCK_W[job["bsize"]], BLOCK_H[job["bsize"]], job["mi_col"] * 4, job["mi_row"] * 4
    return (x0 + lim[0] - 4 >= -pad_w and x0 + lim[1] + 1 + bw - 1 + 4 <= width + pad_w - 1 and y0 + lim[2] - 4 >= -pad_h and
            y0 + lim[3] + 1 + bh - 1 + 4 <= height + pad_h - 1)


# ------------------------------------------------------------------------------------------------------------------ the search
NOTHING = dict(full_row=0, full_col=0, refining=INT_MAX, steps=0, bestsme=INT_MAX, row=0, col=0, besterr=INT_MAX, distortion=0, sse=0, rate_mv=0)
NEIGHBORS = ((-1, 0), (0, -1), (0, 1), (1, 0))
SEARCH_STEPS = ((0, -4), (0, 4), (-4, 0), (4, 0), (0, -2), (0, 2), (-2, 0), (2, 0), (0, -1), (0, 1), (-1, 0), (1, 0))


def search(job, padded, pad_w, pad_h, mi_rows, mi_cols, wsrc, mask, jc, cc, info=None):
    """single_motion_search of one job.  `padded` holds the picture with its border; wsrc / mask are the job's bh x bw arrays.  -> the result as a dict; `info`
    (a dict) receives what the walk met."""
    info = {} if info is None else info
    info.update(sites=[], excluded=0, clamped=False, cost_rejects=0, ties=0, best_idx=[], third=[], out_axis=0, out_diag=0, out_second=0, rewrites=set(), n_sads=0, n_probes=0)
    bw, bh = BLOCK_W[job["bsize"]], BLOCK_H[job["bsize"]]
    y0, x0 = pad_h + job["mi_row"] * 4, pad_w + job["mi_col"] * 4
    ref_row, ref_col, epb = job["ref_mv_row"], job["ref_mv_col"], job["error_per_bit"]
    lim0 = block_limits(job, mi_rows, mi_cols)
    lim = search_range(lim0, ref_row, ref_col)
    if lim[1] < lim[0] or lim[3] < lim[2]:
        return dict(NOTHING, status=1)
    def sad_at(r, c):
        info["n_sads"] += 1
        return obmc_sad(padded[y0 + r:y0 + r + bh, x0 + c:x0 + c + bw], wsrc, mask)

    # svt_av1_obmc_full_pixel_search
    row, col = job["mv_row"] >> 3, job["mv_col"] >> 3
    crow, ccol = max(lim[2], min(lim[3], row)), max(lim[0], min(lim[1], col))
    info["clamped"] = (crow, ccol) != (row, col)
    row, col = crow, ccol
    frow, fcol = ref_row >> 3, ref_col >> 3
    best = (sad_at(row, col) + mvsad_err_cost(row, col, frow, fcol, jc, cc, job["sad_per_bit"])) & U32
    steps = 0
    for _ in range(8):
        best_site = -1
        for j, (dr, dc) in enumerate(NEIGHBORS):
            r, c = row + dr, col + dc
            if not (lim[0] <= c <= lim[1] and lim[2] <= r <= lim[3]):
                info["excluded"] += 1
                continue
            sad = sad_at(r, c)
            if sad < best:
                sad = (sad + mvsad_err_cost(r, c, frow, fcol, jc, cc, job["sad_per_bit"])) & U32
                if sad < best:
                    best, best_site = sad, j
                else:
                    info["cost_rejects"] += 1
                    info["ties"] += sad == best
            else:
                info["ties"] += sad == best
        if best_site == -1:
            break
        info["sites"].append(best_site)
        row, col = row + NEIGHBORS[best_site][0], col + NEIGHBORS[best_site][1]
        steps += 1
    res = dict(status=0, full_row=row, full_col=col, refining=to_int(best), steps=steps, bestsme=to_int(best), row=row, col=col, besterr=INT_MAX, distortion=0, sse=0)

    def probe(r, c):
        info["n_probes"] += 1
        pred = upsampled_pred(padded, y0 + (r >> 3), x0 + (c >> 3), bw, bh, c & 7, r & 7)
        return obmc_variance(pred, wsrc, mask)

    cost = lambda r, c: mv_err_cost(r, c, ref_row, ref_col, jc, cc, epb) & U32
    if res["bestsme"] < INT_MAX:
        res["bestsme"] = to_int(probe(row * 8, col * 8)[0] + cost(row * 8, col * 8))
    if res["bestsme"] < INT_MAX:
        # svt_av1_find_best_obmc_sub_pixel_tree_up
        minc, maxc, minr, maxr = subpel_range(lim0, ref_row, ref_col)
        inside = lambda r, c: minc <= c <= maxc and minr <= r <= maxr
        br, bc, hstep, best_idx = row * 8, col * 8, 4, -1
        var, sse1 = probe(br, bc)
        besterr, distortion = (var + cost(br, bc)) & U32, var
        cost_array = [0] * 5
        for it in range(3 if job["allow_hp"] else 2):
            for idx in range(4):
                tr, tc = br + SEARCH_STEPS[4 * it + idx][0], bc + SEARCH_STEPS[4 * it + idx][1]
                if inside(tr, tc):
                    var, sse = probe(tr, tc)
                    cost_array[idx] = (var + cost(tr, tc)) & U32
                    if cost_array[idx] < besterr:
                        best_idx, besterr, distortion, sse1 = idx, cost_array[idx], var, sse
                else:
                    cost_array[idx] = INT_MAX
                    info["out_axis"] += 1
            kc = -hstep if cost_array[0] <= cost_array[1] else hstep
            kr = -hstep if cost_array[2] <= cost_array[3] else hstep
            tc, tr = bc + kc, br + kr
            if inside(tr, tc):
                var, sse = probe(tr, tc)
                cost_array[4] = (var + cost(tr, tc)) & U32
                if cost_array[4] < besterr:
                    best_idx, besterr, distortion, sse1 = 4, cost_array[4], var, sse
            else:
                cost_array[4] = INT_MAX
                info["out_diag"] += 1
            if 0 <= best_idx < 4:
                br, bc = br + SEARCH_STEPS[4 * it + best_idx][0], bc + SEARCH_STEPS[4 * it + best_idx][1]
            elif best_idx == 4:
                br, bc = tr, tc
            info["best_idx"].append(best_idx)
            if best_idx != -1:   # SECOND_LEVEL_CHECKS_BEST(1)
                br0, bc0 = br, bc
                if tr == br and tc != bc:
                    kc = bc - tc
                    info["rewrites"].add("kc")
                elif tr != br and tc == bc:
                    kr = br - tr
                    info["rewrites"].add("kr")
                checks = [(br0 + kr, bc0), (br0, bc0 + kc)]
                k = 0
                while k < len(checks):
                    r, c = checks[k]
                    if inside(r, c):
                        var, sse = probe(r, c)
                        v = cost(r, c)
                        if (v + var) & U32 < besterr:
                            besterr, br, bc, distortion, sse1 = (v + var) & U32, r, c, var, sse
                    else:
                        info["out_second"] += 1
                    k += 1
                    if k == 2:
                        moved = br0 != br or bc0 != bc
                        info["third"].append(moved)
                        if moved:
                            checks.append((br0 + kr, bc0 + kc))
            hstep >>= 1
            best_idx = -1
        res.update(row=br, col=bc, besterr=besterr, distortion=to_int(distortion), sse=sse1)
    res["rate_mv"] = mv_bit_cost(res["row"], res["col"], ref_row, ref_col, jc, cc)
    return res


# ------------------------------------------------------------------------------------------------------------------ content
def cost_tables(seed=3):
    """MV cost tables of the shape the encoder's have: the cost grows with the class of |d|, a few bits apart between neighbours.  -> (joint[4], comp[2][32767])"""
    rng = np.random.default_rng(seed)
    d = np.abs(np.arange(-MV_MAX, MV_MAX + 1))
    comp = np.stack([(900 * (1 + np.log2(1 + d))).astype(np.int64) + rng.integers(0, 64, d.size) for _ in range(2)])
    comp[:, MV_MAX] = 0
    return np.array([300, 900, 950, 1400], np.int32), comp.astype(np.int32)


def smooth_picture(h, w, seed):
    """a picture whose SAD surface slopes towards the true displacement over several samples: low-pass noise plus a little texture"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (h // 8 + 3, w // 8 + 3)).astype(np.float64)
    yy, xx = np.arange(h) / 8.0, np.arange(w) / 8.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
    a, b, c, d = coarse[y0][:, x0], coarse[y0][:, x0 + 1], coarse[y0 + 1][:, x0], coarse[y0 + 1][:, x0 + 1]
    img = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
    return np.clip(img + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)


def pad_picture(pic, pad_w, pad_h):
    """generate_padding: the border repeats the nearest picture sample"""
    return np.pad(pic, ((pad_h, pad_h), (pad_w, pad_w)), mode="edge")


def centre(bsize, W, H):
    """(mi_row, mi_col), both even, of a block of this size near the middle of a W x H picture"""
    return (H - BLOCK_H[bsize]) // 16 * 2, (W - BLOCK_W[bsize]) // 16 * 2


# ------------------------------------------------------------------------------------------------------------------ the target case list
def _side(kind, n4, rng):
    """(sides, flags) of the n4 units along an edge for a named layout; sides in 4-sample units"""
    if kind == "none":
        return None
    if kind == "one":          # one neighbour as long as the block (or longer)
        return [max(n4, 2)] * n4, [1] * n4
    if kind == "halves":
        return [n4 // 2] * n4, [1] * n4
    if kind == "quarters":
        return [max(n4 // 4, 2)] * n4, [1] * n4
    if kind == "eighths":      # more neighbours than nb_max allows on the sides that have them
        return [2] * n4, [1] * n4
    if kind == "gap":          # overlappable, not, overlappable ...
        side = max(n4 // 4, 2)
        return [side] * n4, [0 if (i // side) % 2 else 1 for i in range(n4)]
    if kind == "pairs":        # 4-wide neighbours: the odd one of a pair decides
        return [1] * n4, [(i // 2) % 2 if i % 2 else 1 - (i // 2) % 2 for i in range(n4)]
    if kind == "blocked":
        return [max(n4 // 2, 2)] * n4, [0] * n4
    if kind == "random":
        sides, flags, i = [], [], 0
        while i < n4:
            s = int(rng.choice([1, 2, 4, 8, 16, 32]))
            while i and s > 1 and (i % s or s > n4 - i):   # a neighbour is aligned to its size; only the first may reach beyond the block
                s //= 2
            sides += [s] * s
            flags += [int(rng.integers(0, 2))] * s
            i += s
        return sides[:n4], flags[:n4]
    raise ValueError(kind)


def target_specs(which):
    """[dict(bsize, x, y, above, left, mi_cols, mi_rows, seed)]: `which` = "small" (a 96 x 64 picture, sizes up to 64 x 64) or "big" (128 x 128, the 128-wide sizes)"""
    W, H = (96, 64) if which == "small" else (128, 128)
    specs, seed = [], 0

    def add(bsize, x, y, above, left, mi_cols=None, mi_rows=None):
        nonlocal seed
        seed += 1
        specs.append(dict(bsize=bsize, x=x, y=y, above=above, left=left, mi_cols=W // 4 if mi_cols is None else mi_cols, mi_rows=H // 4 if mi_rows is None else mi_rows, seed=seed))

    if which == "big":
        for b in BIG_SIZES:
            for above, left in (("quarters", "eighths"), ("random", "halves"), ("gap", "pairs")):
                add(b, 0, 0, above, left)
        add(15, 0, 0, "quarters", "quarters", mi_cols=20, mi_rows=28)
        return specs
    for b in SMALL_SIZES:   # one job per shape, every layout on the four named shapes
        mr, mc = centre(b, W, H)
        add(b, mc * 4, mr * 4, "halves", "halves")
    kinds = ("none", "one", "halves", "quarters", "eighths", "gap", "pairs", "blocked", "random")
    for b in (BSIZE_OF[8, 8], BSIZE_OF[8, 32], BSIZE_OF[32, 8], BSIZE_OF[16, 16], BSIZE_OF[32, 32]):
        for above in kinds:
            for left in (kinds if b == BSIZE_OF[16, 16] else ("one", "random") if b == BSIZE_OF[32, 32] else ("none", "one", "eighths", "random")):
                add(b, 8, 8, above, left)
    for above, left in (("eighths", "gap"), ("random", "eighths"), ("none", "quarters"), ("pairs", "none")):
        add(BSIZE_OF[64, 64], 0, 0, above, left)
    # cut by the picture's last column / row: the picture ends inside the block
    add(BSIZE_OF[32, 32], 64, 32, "eighths", "eighths", mi_cols=(64 + 12) // 4, mi_rows=(32 + 20) // 4)
    add(BSIZE_OF[16, 16], 80, 48, "pairs", "pairs", mi_cols=(80 + 4) // 4 + 0, mi_rows=(48 + 12) // 4)
    add(BSIZE_OF[64, 64], 32, 0, "quarters", "quarters", mi_cols=(32 + 40) // 4, mi_rows=9)
    return specs


def build_target_case(which):
    """-> dict(plane, nbr, jobs [dict of TARGET_FIELDS], segs [(above, left)], wm_samples, specs)"""
    specs = target_specs(which)
    W, H = (96, 64) if which == "small" else (128, 128)
    plane = smooth_picture(H, W, 100 + len(specs))
    pool, jobs, segs, wm = [], [], [], 0
    off = 0
    for s in specs:
        rng = np.random.default_rng(1000 + s["seed"])
        b = s["bsize"]
        bw, bh = BLOCK_W[b], BLOCK_H[b]
        n4w, n4h = bw // 4, bh // 4
        a, l = _side(s["above"], n4w, rng), _side(s["left"], n4h, rng)
        sa = neighbours(a[0], a[1], n4w, s["x"] // 4, s["mi_cols"]) if a else []
        sl = neighbours(l[0], l[1], n4h, s["y"] // 4, s["mi_rows"]) if l else []
        ov_a, ov_l = min(bh, 64) >> 1, min(bw, 64) >> 1
        # the neighbour predictions: the above area with a stride wider than the block, the left area as a column strip
        a_stride, l_stride = bw + 8 * (s["seed"] % 3), ov_l + 4 * (s["seed"] % 2)
        above = rng.integers(0, 256, (ov_a, a_stride)).astype(np.uint8)
        left = rng.integers(0, 256, (bh, l_stride)).astype(np.uint8)
        job = dict(bsize=b, x=s["x"], y=s["y"], n_above=len(sa), above_rel=[r for r, _ in sa] + [0] * (4 - len(sa)), above_len=[n for _, n in sa] + [0] * (4 - len(sa)),
                   n_left=len(sl), left_rel=[r for r, _ in sl] + [0] * (4 - len(sl)), left_len=[n for _, n in sl] + [0] * (4 - len(sl)), above_off=off, above_stride=a_stride,
                   left_off=off + above.size, left_stride=l_stride, wm_off=wm)
        pool += [above.reshape(-1), left.reshape(-1)]
        off += above.size + left.size
        wm += bw * bh
        jobs.append(job)
        segs.append((sa, sl, a, l))
    return dict(plane=plane, nbr=np.concatenate(pool), jobs=jobs, segs=segs, wm_samples=wm, specs=specs)


def run_target_case(case):
    """the restatement on every job -> (wsrc, mask) flat int32 arrays of wm_samples"""
    wsrc, mask = np.zeros(case["wm_samples"], np.int32), np.zeros(case["wm_samples"], np.int32)
    nbr = case["nbr"]
    for j, (sa, sl, _, _) in zip(case["jobs"], case["segs"]):
        bw, bh = BLOCK_W[j["bsize"]], BLOCK_H[j["bsize"]]
        ov_a, ov_l = min(bh, 64) >> 1, min(bw, 64) >> 1
        above = nbr[j["above_off"]:j["above_off"] + ov_a * j["above_stride"]].reshape(ov_a, j["above_stride"])
        left = nbr[j["left_off"]:j["left_off"] + bh * j["left_stride"]].reshape(bh, j["left_stride"])
        w, m = target(case["plane"][j["y"]:j["y"] + bh, j["x"]:j["x"] + bw], above, left, sa, sl, bw, bh)
        wsrc[j["wm_off"]:j["wm_off"] + bw * bh], mask[j["wm_off"]:j["wm_off"] + bw * bh] = w.reshape(-1), m.reshape(-1)
    return wsrc, mask


# ------------------------------------------------------------------------------------------------------------------ the search case list
def search_specs(which):
    """[dict(bsize, mi_row, mi_col, shift (dy, dx): the source is the reference displaced by it, mv, ref_mv, sad_per_bit, error_per_bit, allow_hp, style, seed)]"""
    W, H = (96, 64) if which == "small" else (128, 128)
    specs, seed = [], 0

    def add(bsize, mi_row, mi_col, shift=(0, 0), mv=(0, 0), ref_mv=(0, 0), sad_per_bit=40, error_per_bit=60, allow_hp=1, style="smooth"):
        nonlocal seed
        seed += 1
        specs.append(dict(bsize=bsize, mi_row=mi_row, mi_col=mi_col, shift=shift, mv=mv, ref_mv=ref_mv, sad_per_bit=sad_per_bit, error_per_bit=error_per_bit,
                          allow_hp=allow_hp, style=style, seed=seed))

    if which == "big":
        for i, b in enumerate(BIG_SIZES):
            add(b, 0, 0, shift=(2, -3), mv=(8, -8), allow_hp=1)
            add(b, 0, 0, shift=(-1, 1), mv=(-4, 20), ref_mv=(-9, 13), allow_hp=i % 2)
        return specs
    for i, b in enumerate(SMALL_SIZES):   # one job per shape
        add(b, *centre(b, W, H), shift=(1 + i % 3, -2 + i % 4), mv=(3, -5), ref_mv=(6, -2), allow_hp=i % 2)
    named = (BSIZE_OF[8, 8], BSIZE_OF[8, 32], BSIZE_OF[32, 8], BSIZE_OF[16, 16])
    for k, b in enumerate(named):
        bw, bh = BLOCK_W[b], BLOCK_H[b]
        mr, mc = centre(b, W, H)
        # the source displaced towards each of the four sides: every site wins; far displacements use all eight steps
        for shift in ((-3, 0), (3, 0), (0, -3), (0, 3), (-9, 0), (0, 10), (6, 6), (-5, 7), (1, 1), (0, 0)):
            for hp in (0, 1):
                add(b, mr, mc, shift=shift, mv=(0, 0), ref_mv=(shift[0] * 8 + 3, shift[1] * 8 - 2), allow_hp=hp, sad_per_bit=8, error_per_bit=20 + 40 * hp)
        # a walk of 0 steps: start at the displacement; sub-pel displacements of the reference (style "subpel": the source is a sub-pel prediction)
        for frac in ((0, 0), (4, 0), (0, 4), (4, 4), (2, 6), (6, 2), (1, 3), (3, 7), (7, 5), (5, 1), (2, 0), (0, 6), (6, 6), (3, 3)):
            for hp in (0, 1):
                add(b, mr, mc, shift=(16 + frac[0], -8 + frac[1]), mv=(16, -8), ref_mv=(12, -4), allow_hp=hp, style="subpel", error_per_bit=30)
        # the cost decides: a high price per bit and a start away from ref_mv
        for spb in (600, 3000, 20000):
            add(b, mr, mc, shift=(2, 2), mv=(-16, -16), ref_mv=(-16, -16), sad_per_bit=spb, error_per_bit=400)
            add(b, mr, mc, shift=(-1, 2), mv=(0, 0), ref_mv=(40, -40), sad_per_bit=spb, error_per_bit=2000)
        # flat content: every sad ties
        add(b, mr, mc, style="flat")
        add(b, mr, mc, mv=(24, 24), ref_mv=(24, 24), style="flat", sad_per_bit=0, error_per_bit=0)
        # at and beyond the limits: the start is clamped, sites and probes fall outside
        n4w, n4h = bw // 4, bh // 4
        lo_r, lo_c, hi_r, hi_c = -((mr + n4h) * 4 + 4), -((mc + n4w) * 4 + 4), (H // 4 - mr) * 4 + 4, (W // 4 - mc) * 4 + 4
        for mv in ((lo_r * 8 - 40, 0), (0, lo_c * 8 - 8), (hi_r * 8 + 16, hi_c * 8 + 16), (lo_r * 8, lo_c * 8), (hi_r * 8, 0), (0, hi_c * 8), (lo_r * 8 + 8, hi_c * 8 - 8)):
            for hp in (0, 1):
                add(b, mr, mc, mv=mv, ref_mv=(mv[0] // 2, mv[1] // 2), allow_hp=hp, style="edge", sad_per_bit=4 + k, error_per_bit=10)
                add(b, mr, mc, mv=mv, ref_mv=(mv[0] // 2 + 3, mv[1] // 2 - 3), allow_hp=hp, style="edge", sad_per_bit=1, error_per_bit=1)
        # a price so high that a probe inside the range costs more than INT_MAX (the vector cost alone, about 25 000 * 2^17): the comparison of an axis pair then
        # prefers the side that is outside, and the diagonal goes there.  ref_mv is as far away as the limits allow without being narrowed
        for hp in (0, 1):
            add(b, mr, mc, mv=(lo_r * 8, lo_c * 8), ref_mv=(7700, 7700), allow_hp=hp, style="edge", sad_per_bit=2, error_per_bit=INT_MAX - 1000 * k)
            add(b, mr, mc, mv=(hi_r * 8, hi_c * 8), ref_mv=(-7700, -7700), allow_hp=hp, style="edge", sad_per_bit=2, error_per_bit=INT_MAX - 1000 * k)
        add(b, 0, 0, shift=(1, -1), mv=(9, -9), ref_mv=(5, 5), allow_hp=k % 2)
    add(BSIZE_OF[16, 16], 2, 2, ref_mv=(32767, 32767))   # limits that the narrowing empties: status 1
    add(BSIZE_OF[8, 8], 2, 2, ref_mv=(-32768, 0))
    return specs


def build_search_case(which):
    """-> dict(padded, pad_w, pad_h, width, height, mi_rows, mi_cols, wsrc, mask (flat), jobs [dict of JOB_FIELDS], jc, cc, specs, target).  `target` is a case of
    stage 1 (as build_target_case makes them) whose job k produces the wsrc / mask of search job k at the same wm_off: the sources stacked in one plane as wide as
    the widest block, neighbour predictions near the source; wsrc / mask are the restatement's output on it."""
    specs = search_specs(which)
    W, H = (96, 64) if which == "small" else (128, 128)
    pad = 80 if which == "small" else 144
    pic = smooth_picture(H, W, 7 if which == "small" else 8)
    padded = pad_picture(pic, pad, pad)
    jc, cc = cost_tables()
    width = max(BLOCK_W[s["bsize"]] for s in specs)
    jobs, tjobs, segs, rows, pool, wm, off, y = [], [], [], [], [], 0, 0, 0
    for s in specs:
        rng = np.random.default_rng(5000 + s["seed"])
        b = s["bsize"]
        bw, bh = BLOCK_W[b], BLOCK_H[b]
        y0, x0 = pad + s["mi_row"] * 4, pad + s["mi_col"] * 4
        dy, dx = s["shift"]
        if s["style"] == "flat":
            src = np.full((bh, bw), 77, np.uint8)
        elif s["style"] == "subpel":
            src = upsampled_pred(padded, y0 + (dy >> 3), x0 + (dx >> 3), bw, bh, dx & 7, dy & 7).astype(np.uint8)
        elif s["style"] == "edge":
            src = rng.integers(0, 256, (bh, bw)).astype(np.uint8)
        else:
            src = np.clip(padded[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw].astype(np.int64) + rng.integers(-3, 4, (bh, bw)), 0, 255).astype(np.uint8)
        near = lambda: np.clip(src.astype(np.int64) + rng.integers(-12, 13, (bh, bw)), 0, 255).astype(np.uint8)
        n4w, n4h = bw // 4, bh // 4
        sa = [] if s["seed"] % 5 == 0 else [(0, n4w)] if s["seed"] % 2 else [(0, n4w // 2), (n4w // 2, n4w // 2)]
        sl = [] if s["seed"] % 7 == 0 else [(0, n4h)]
        ov_a, ov_l = min(bh, 64) >> 1, min(bw, 64) >> 1
        above, left = near()[:ov_a], np.ascontiguousarray(near()[:, :ov_l])
        strip = np.zeros((bh, width), np.uint8)
        strip[:, :bw] = src
        rows.append(strip)
        tjobs.append(dict(bsize=b, x=0, y=y, n_above=len(sa), above_rel=[r for r, _ in sa] + [0] * (4 - len(sa)), above_len=[n for _, n in sa] + [0] * (4 - len(sa)),
                          n_left=len(sl), left_rel=[r for r, _ in sl] + [0] * (4 - len(sl)), left_len=[n for _, n in sl] + [0] * (4 - len(sl)), above_off=off,
                          above_stride=bw, left_off=off + above.size, left_stride=ov_l, wm_off=wm))
        segs.append((sa, sl, None, None))
        pool += [above.reshape(-1), left.reshape(-1)]
        off += above.size + left.size
        jobs.append(dict(bsize=b, mi_row=s["mi_row"], mi_col=s["mi_col"], wm_off=wm, mv_row=s["mv"][0], mv_col=s["mv"][1], ref_mv_row=s["ref_mv"][0], ref_mv_col=s["ref_mv"][1],
                         sad_per_bit=s["sad_per_bit"], error_per_bit=s["error_per_bit"], allow_hp=s["allow_hp"]))
        wm += bw * bh
        y += bh
    tcase = dict(plane=np.concatenate(rows), nbr=np.concatenate(pool), jobs=tjobs, segs=segs, wm_samples=wm, specs=specs)
    wsrc, mask = run_target_case(tcase)
    return dict(padded=padded, pad_w=pad, pad_h=pad, width=W, height=H, mi_rows=H // 4, mi_cols=W // 4, wsrc=wsrc, mask=mask, jobs=jobs, jc=jc, cc=cc, specs=specs, target=tcase)


def picture_view(case):
    """the picture inside its padded plane, as the bindings take it"""
    return case["padded"][case["pad_h"]:case["pad_h"] + case["height"], case["pad_w"]:case["pad_w"] + case["width"]]


def run_search_case(case, infos=None):
    out = []
    for k, j in enumerate(case["jobs"]):
        n = BLOCK_W[j["bsize"]] * BLOCK_H[j["bsize"]]
        shape = (BLOCK_H[j["bsize"]], BLOCK_W[j["bsize"]])
        w, m = case["wsrc"][j["wm_off"]:j["wm_off"] + n].reshape(shape), case["mask"][j["wm_off"]:j["wm_off"] + n].reshape(shape)
        out.append(search(j, case["padded"], case["pad_w"], case["pad_h"], case["mi_rows"], case["mi_cols"], w, m, case["jc"], case["cc"], None if infos is None else infos[k]))
    return out


@functools.lru_cache(maxsize=None)
def cached(kind, which):
    """the cases and the restatement's results, made once per process: ("target" | "search", "small" | "big") -> (case, results, infos)"""
    if kind == "target":
        case = build_target_case(which)
        return case, run_target_case(case), None
    case = build_search_case(which)
    infos = [{} for _ in case["jobs"]]
    return case, run_search_case(case, infos), infos


def flat_target_job(j):
    """a target job as the int32 row tests/golden/obmc_search.npz keeps"""
    return [v for f in TARGET_FIELDS for v in (j[f] if isinstance(j[f], list) else [j[f]])]


def input_crcs(which):
    """CRC-32 of the samples the recorded results were made from: the target case's source plane and neighbour pool, the search case's padded plane, wsrc, mask and
    both cost tables.  The golden file keeps jobs, these and the results; the samples are made again here from their seeds."""
    import zlib
    t, _, _ = cached("target", which)
    c, _, _ = cached("search", which)
    parts = (t["plane"], t["nbr"], c["padded"], c["wsrc"], c["mask"], c["jc"], c["cc"])
    return [zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in parts]


# ------------------------------------------------------------------------------------------------------------------ ctypes
def c_target_jobs(pkg, jobs):
    arr = (pkg.ObmcTargetJob * max(len(jobs), 1))()
    for a, j in zip(arr, jobs):
        for f in TARGET_FIELDS:
            if isinstance(j[f], list):
                getattr(a, f)[:] = j[f]
            else:
                setattr(a, f, j[f])
    return (pkg.ObmcTargetJob * len(jobs)).from_buffer(arr) if jobs else (pkg.ObmcTargetJob * 0)()


def c_search_jobs(pkg, jobs):
    arr = (pkg.ObmcSearchJob * max(len(jobs), 1))()
    for a, j in zip(arr, jobs):
        for f in JOB_FIELDS:
            setattr(a, f, j[f])
    return (pkg.ObmcSearchJob * len(jobs)).from_buffer(arr) if jobs else (pkg.ObmcSearchJob * 0)()


def results_as_dicts(res, n):
    return [{f: int(getattr(res[i], f)) for f in RESULT_FIELDS} for i in range(n)]
