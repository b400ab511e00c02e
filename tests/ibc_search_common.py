"""The intra-block-copy full-pel search restated in numpy, and the case lists of the tests around it (tests/test_ibc_search_ref_cpu.py pins the restatement to
the reference's recorded results and asserts what the case lists exist for; tests/test_ibc_search_gpu.py and the host-form tests compare the library with it).
The scalar forms follow the reference line for line, both branches of all_in and the four-at-a-time column loop included.  File:line under Source/Lib:
  Encoder/Codec/av1me.c:284-290    mvsad_err_cost
  Encoder/Codec/av1me.c:292-318    svt_av1_init3smotion_compensation
  Encoder/Codec/av1me.c:346-435    exhuastive_mesh_search
  Encoder/Codec/av1me.c:437-573    svt_av1_diamond_search_sad_c
  Encoder/Codec/av1me.c:578-643    full_pixel_diamond
  Encoder/Codec/av1me.c:650-710    full_pixel_exhaustive
  Encoder/Codec/av1me.c:712-775    svt_av1_refining_search_sad
  Encoder/Codec/av1me.c:1306-1411  svt_av1_full_pixel_search, case NSTEP and the hash tail
  Encoder/Codec/EbModeDecision.c:4486-4490, :4523   the caller's `continue` and av1_is_dv_valid"""
import numpy as np

import ibc_hash_common as H

INT_MAX = H.INT32_MAX
MAX_MVSEARCH_STEPS, MAX_FIRST_STEP, MAX_MESH_STEP = 11, 1024, 4
MIN_RANGE, MAX_RANGE, MIN_INTERVAL = 7, 256, 1
JOB_FIELDS = ("x_pos", "y_pos", "block_w", "block_h", "intra", "col_min", "col_max", "row_min", "row_max", "ref_mv_row", "ref_mv_col", "mvp_row", "mvp_col", "step_param",
              "sad_per_bit", "error_per_bit", "exhaustive_allowed", "ibc_shift", "use_hash", "mi_row_start", "mi_row_end", "mi_col_start", "mi_col_end", "mib_size_log2")
RESULT_FIELDS = ("status", "dia_passes", "dia_refined", "dia_var", "dia_row", "dia_col", "mesh_ran", "mesh_passes", "mesh_var", "mesh_row", "mesh_col", "hash", "source", "var",
                 "best_row", "best_col", "dv_valid")
SHAPES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128),
          (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]   # (w, h), BlockSize order
PATTERNS = dict(full=[(256, 1), (256, 1)], two=[(64, 4), (16, 1)], four=[(64, 8), (28, 4), (15, 1), (7, 1)], invalid=[(300, 1), (16, 1)],
                deep=[(64, 8), (28, 4), (15, 2), (7, 1)])

# svt_av1_init3smotion_compensation: ss[0] the centre, then 11 steps of 8 sites
SS = [(0, 0)]
_len = MAX_FIRST_STEP
while _len > 0:
    SS += [(-_len, 0), (_len, 0), (0, -_len), (0, _len), (-_len, -_len), (-_len, _len), (_len, -_len), (_len, _len)]
    _len //= 2
SS_COUNT, SEARCHES_PER_STEP = len(SS), 8


def u32(v):
    return v & 0xFFFFFFFF


class X:
    """what the reference keeps in IntraBcContext for one job: the plane (source and reference), the limits, the cost tables; counts its SAD calls"""

    def __init__(self, plane, bd, j, jc, cc):
        self.p = plane if plane.dtype == np.int32 else plane.astype(np.int32)
        self.bd, self.j, self.jc, self.cc = bd, j, jc, cc
        self.x0, self.y0, self.bw, self.bh = j["x_pos"], j["y_pos"], j["block_w"], j["block_h"]
        self.what = self.p[self.y0:self.y0 + self.bh, self.x0:self.x0 + self.bw]
        self.n_sad = 0

    def block(self, row, col):
        y, x = self.y0 + row, self.x0 + col
        assert 0 <= y <= self.p.shape[0] - self.bh and 0 <= x <= self.p.shape[1] - self.bw, "a vector outside the picture"
        return self.p[y:y + self.bh, x:x + self.bw]

    def sdf(self, row, col):
        self.n_sad += 1
        return int(np.abs(self.what - self.block(row, col)).sum())

    def is_mv_in(self, row, col):
        j = self.j
        return j["col_min"] <= col <= j["col_max"] and j["row_min"] <= row <= j["row_max"]

    def clamp(self, row, col):
        j = self.j
        return min(max(row, j["row_min"]), j["row_max"]), min(max(col, j["col_min"]), j["col_max"])


def mv_cost(d_row, d_col, jc, cc):
    joint = (0 if d_col == 0 else 1) if d_row == 0 else (2 if d_col == 0 else 3)
    return int(jc[joint]) + int(cc[0][H.MV_MAX + d_row]) + int(cc[1][H.MV_MAX + d_col])


def mvsad_err_cost(x, row, col, ref_row, ref_col, sad_per_bit):
    """(row, col) and the reference in whole samples; the product is unsigned"""
    return u32(u32(u32(mv_cost((row - ref_row) * 8, (col - ref_col) * 8, x.jc, x.cc)) * sad_per_bit) + 256) >> 9


def get_mvpred_var(x, row, col):
    """svt_av1_get_mvpred_var(x, best_mv, center_mv = ref_mv, vfp, 1)"""
    j = x.j
    cost = H.mv_err_cost(row * 8 - j["ref_mv_row"], col * 8 - j["ref_mv_col"], x.jc, x.cc, j["error_per_bit"])
    return H._as_int32(H.variance(x.what, x.block(row, col), x.bd) + cost)


def diamond_search_sad(x, mvp, search_param, sad_per_bit):
    """svt_av1_diamond_search_sad_c -> (bestsad, best_mv, num00)"""
    j = x.j
    ss = SS[search_param * SEARCHES_PER_STEP:]
    tot_steps = SS_COUNT // SEARCHES_PER_STEP - search_param
    fc_row, fc_col = j["ref_mv_row"] >> 3, j["ref_mv_col"] >> 3
    ref_row, ref_col = x.clamp(*mvp)
    num00, best_site, last_site = 0, 0, 0
    best_row, best_col = ref_row, ref_col
    bestsad = x.sdf(best_row, best_col) + mvsad_err_cost(x, best_row, best_col, fc_row, fc_col, sad_per_bit)
    i = 1
    for step in range(tot_steps):
        all_in = ((best_row + ss[i][0]) > j["row_min"] and (best_row + ss[i + 1][0]) < j["row_max"] and (best_col + ss[i + 2][1]) > j["col_min"] and
                  (best_col + ss[i + 3][1]) < j["col_max"])
        if all_in:
            for _ in range(0, SEARCHES_PER_STEP, 4):
                sad_array = [x.sdf(best_row + ss[i + t][0], best_col + ss[i + t][1]) for t in range(4)]
                for t in range(4):
                    if sad_array[t] < bestsad:
                        this = (best_row + ss[i][0], best_col + ss[i][1])
                        sad_array[t] += mvsad_err_cost(x, this[0], this[1], fc_row, fc_col, sad_per_bit)
                        if sad_array[t] < bestsad:
                            bestsad, best_site = sad_array[t], i
                    i += 1
        else:
            for _ in range(SEARCHES_PER_STEP):
                this = (best_row + ss[i][0], best_col + ss[i][1])
                if x.is_mv_in(*this):
                    thissad = x.sdf(*this)
                    if thissad < bestsad:
                        thissad += mvsad_err_cost(x, this[0], this[1], fc_row, fc_col, sad_per_bit)
                        if thissad < bestsad:
                            bestsad, best_site = thissad, i
                i += 1
        if best_site != last_site:
            best_row += ss[best_site][0]
            best_col += ss[best_site][1]
            last_site = best_site
        elif (best_row, best_col) == (ref_row, ref_col):
            num00 += 1
    return bestsad, (best_row, best_col), num00


def refining_search_sad(x, mv, error_per_bit, search_range):
    """svt_av1_refining_search_sad -> (best_sad, mv, rounds that moved)"""
    j = x.j
    neighbors = [(-1, 0), (0, -1), (0, 1), (1, 0)]
    fc_row, fc_col = j["ref_mv_row"] >> 3, j["ref_mv_col"] >> 3
    row, col = mv
    best_sad = x.sdf(row, col) + mvsad_err_cost(x, row, col, fc_row, fc_col, error_per_bit)
    moved = 0
    for _ in range(search_range):
        best_site = -1
        all_in = (row - 1) > j["row_min"] and (row + 1) < j["row_max"] and (col - 1) > j["col_min"] and (col + 1) < j["col_max"]
        if all_in:
            sads = [x.sdf(row + n[0], col + n[1]) for n in neighbors]
            for k in range(4):
                if sads[k] < best_sad:
                    sads[k] += mvsad_err_cost(x, row + neighbors[k][0], col + neighbors[k][1], fc_row, fc_col, error_per_bit)
                    if sads[k] < best_sad:
                        best_sad, best_site = sads[k], k
        else:
            for k in range(4):
                m = (row + neighbors[k][0], col + neighbors[k][1])
                if x.is_mv_in(*m):
                    sad = x.sdf(*m)
                    if sad < best_sad:
                        sad += mvsad_err_cost(x, m[0], m[1], fc_row, fc_col, error_per_bit)
                        if sad < best_sad:
                            best_sad, best_site = sad, k
        if best_site == -1:
            break
        row += neighbors[best_site][0]
        col += neighbors[best_site][1]
        moved += 1
    return best_sad, (row, col), moved


def full_pixel_diamond(x, mvp_full, step_param, sadpb, further_steps, do_refine, info):
    """-> (bestsme, best_mv); info collects passes, skipped, cleared (do_refine set to 0), refined, refine_moved"""
    mvp_full = x.clamp(*mvp_full)   # the first call clamps mvp_full in place: every later pass starts from the clamped vector
    bestsme, temp_mv, n = diamond_search_sad(x, mvp_full, step_param, sadpb)
    num00 = 0
    info.update(passes=1, skipped=0, cleared=0, refined=0, refine_moved=0, pass_results=[(bestsme, temp_mv, n)])
    if bestsme < INT_MAX:
        bestsme = get_mvpred_var(x, *temp_mv)
    best_mv = temp_mv
    if n > further_steps:
        do_refine = 0
        info["cleared"] = 1
    while n < further_steps:
        n += 1
        if num00:
            num00 -= 1
            info["skipped"] += 1
        else:
            thissme, temp_mv, num00 = diamond_search_sad(x, mvp_full, step_param + n, sadpb)
            info["passes"] += 1
            info["pass_results"].append((thissme, temp_mv, num00))
            if thissme < INT_MAX:
                thissme = get_mvpred_var(x, *temp_mv)
            if num00 > further_steps - n:
                do_refine = 0
                info["cleared"] = 1
            if thissme < bestsme:
                bestsme, best_mv = thissme, temp_mv
    if do_refine:
        thissme, mv, moved = refining_search_sad(x, best_mv, sadpb, 8)
        info.update(refined=1, refine_moved=moved, refine_result=(thissme, mv))
        if thissme < INT_MAX:
            thissme = get_mvpred_var(x, *mv)
        if thissme < bestsme:
            bestsme, best_mv = thissme, mv
    return bestsme, best_mv


def mesh_window(x, centre, rng, step):
    """the clamped centre and start / end of rows and columns, relative to it"""
    j = x.j
    fc = x.clamp(*centre)
    return (fc, max(-rng, j["row_min"] - fc[0]), max(-rng, j["col_min"] - fc[1]), min(rng, j["row_max"] - fc[0]), min(rng, j["col_max"] - fc[1]))


def exhuastive_mesh_search(x, ref_mv, centre, rng, step, sad_per_bit, visited=None):
    """the literal loop -> (best_sad, best_mv).  ref_mv in whole samples.  visited, a list, receives every vector a SAD was taken of, in order"""
    assert step >= 1
    col_step = step if step > 1 else 4
    fc, start_row, start_col, end_row, end_col = mesh_window(x, centre, rng, step)
    best_mv = fc
    best_sad = x.sdf(*fc) + mvsad_err_cost(x, fc[0], fc[1], ref_mv[0], ref_mv[1], sad_per_bit)
    note = visited.append if visited is not None else (lambda m: None)

    def try_mv(m):
        nonlocal best_sad, best_mv
        note(m)
        sad = x.sdf(*m)
        if sad < best_sad:
            sad += mvsad_err_cost(x, m[0], m[1], ref_mv[0], ref_mv[1], sad_per_bit)
            if sad < best_sad:
                best_sad, best_mv = sad, m

    for r in range(start_row, end_row + 1, step):
        for c in range(start_col, end_col + 1, col_step):
            if step > 1:
                try_mv((fc[0] + r, fc[1] + c))
            elif c + 3 <= end_col:
                for i in range(4): try_mv((fc[0] + r, fc[1] + c + i))
            else:
                for i in range(end_col - c): try_mv((fc[0] + r, fc[1] + c + i))
    return best_sad, best_mv


def mesh_columns(start_col, end_col, step):
    """the columns, relative to the centre, the loop above examines in a row"""
    n = end_col - start_col + 1
    if step > 1: return list(range(start_col, end_col + 1, step))
    return list(range(start_col, end_col + 1 if n % 4 == 0 else end_col))


def mesh_search_vectorised(x, ref_mv, centre, rng, step, sad_per_bit, visited=None):
    """the same result from all totals at once: the first strict minimum of sad + cost in scan order, the clamped centre first"""
    fc, start_row, start_col, end_row, end_col = mesh_window(x, centre, rng, step)
    best_sad = x.sdf(*fc) + mvsad_err_cost(x, fc[0], fc[1], ref_mv[0], ref_mv[1], sad_per_bit)
    rows, cols = np.arange(start_row, end_row + 1, step) + fc[0], np.array(mesh_columns(start_col, end_col, step), np.int64) + fc[1]
    if len(rows) == 0 or len(cols) == 0: return best_sad, fc
    sad = np.zeros((len(rows), len(cols)), np.int64)
    for dy in range(x.bh):
        for dx in range(x.bw):
            sad += np.abs(x.p[np.ix_(x.y0 + rows + dy, x.x0 + cols + dx)] - x.what[dy, dx])
    x.n_sad += sad.size
    d_row, d_col = (rows - ref_mv[0]) * 8, (cols - ref_mv[1]) * 8
    joint = np.where(d_row[:, None] == 0, np.where(d_col[None, :] == 0, 0, 1), np.where(d_col[None, :] == 0, 2, 3))
    cost = x.jc.astype(np.int64)[joint] + x.cc[0].astype(np.int64)[H.MV_MAX + d_row][:, None] + x.cc[1].astype(np.int64)[H.MV_MAX + d_col][None, :]
    cost = ((((cost & 0xFFFFFFFF) * sad_per_bit) & 0xFFFFFFFF) + 256 & 0xFFFFFFFF) >> 9
    total = (sad + cost).ravel()
    k = int(np.argmin(total))   # the first of the smallest: row-major is the scan's order
    if visited is not None: visited.extend((int(r), int(c)) for r in rows for c in cols)
    if int(total[k]) < best_sad: return int(total[k]), (int(rows[k // len(cols)]), int(cols[k % len(cols)]))
    return best_sad, fc


def full_pixel_exhaustive(x, centre, sadpb, patterns, info, mesh=exhuastive_mesh_search):
    """-> (bestsme, dst_mv); patterns [(range, interval)] * 4; info["mesh_passes"] collects (range, interval, centre, best_sad, best_mv) per scan"""
    j = x.j
    temp_mv = centre
    f_ref_mv = (j["ref_mv_row"] >> 3, j["ref_mv_col"] >> 3)
    rng, interval = patterns[0]
    info["mesh_passes"] = []
    if rng < MIN_RANGE or rng > MAX_RANGE or interval < MIN_INTERVAL or interval > rng:
        return INT_MAX, (0, 0)
    baseline_interval_divisor = rng // interval
    rng = max(rng, (5 * max(abs(temp_mv[0]), abs(temp_mv[1]))) // 4)
    rng = min(rng, MAX_RANGE)
    interval = max(interval, rng // baseline_interval_divisor)

    def scan(r, s):
        nonlocal temp_mv
        best, mv = mesh(x, f_ref_mv, temp_mv, r, s, sadpb)
        info["mesh_passes"].append((r, s, x.clamp(*temp_mv), best, mv))
        temp_mv = mv
        return best

    bestsme = scan(rng, interval)
    if interval > MIN_INTERVAL and rng > MIN_RANGE:
        for i in range(1, MAX_MESH_STEP):
            bestsme = scan(*patterns[i])
            if patterns[i][1] == 1: break
    if bestsme < INT_MAX:
        bestsme = get_mvpred_var(x, *temp_mv)
    return bestsme, temp_mv


def ilog2(v):
    return v.bit_length() - 1


def exhaustive_thr(j):
    return (((1 << 25) >> (10 - (ilog2(j["block_w"] // 4) + ilog2(j["block_h"] // 4)))) << j["ibc_shift"])


def dv_rule(j, row, col):
    """av1_is_dv_valid of the whole-sample vector for a block_w x block_h block: ibc_hash_common.dv_rule with both sides and is_chroma_reference at 4:2:0"""
    bw, bh = j["block_w"], j["block_h"]
    mi_row, mi_col = j["y_pos"] // 4, j["x_pos"] // 4
    dv_row, dv_col = 8 * row, 8 * col
    src_top, tile_top = mi_row * 32 + dv_row, j["mi_row_start"] * 32
    if src_top < tile_top: return 1
    src_left, tile_left = mi_col * 32 + dv_col, j["mi_col_start"] * 32
    if src_left < tile_left: return 2
    src_bottom, tile_bottom = (mi_row * 4 + bh) * 8 + dv_row, j["mi_row_end"] * 32
    if src_bottom > tile_bottom: return 3
    src_right, tile_right = (mi_col * 4 + bw) * 8 + dv_col, j["mi_col_end"] * 32
    if src_right > tile_right: return 4
    if ((mi_row & 1) or not ((bh // 4) & 1)) and ((mi_col & 1) or not ((bw // 4) & 1)):
        if bw < 8 and src_left < tile_left + 32: return 5
        if bh < 8 and src_top < tile_top + 32: return 6
    log2 = j["mib_size_log2"]
    sb_size = (1 << log2) * 4
    active_sb_row, active_sb64_col = mi_row >> log2, (mi_col * 4) >> 6
    src_sb_row, src_sb64_col = H._cdiv((src_bottom >> 3) - 1, sb_size), ((src_right >> 3) - 1) >> 6
    total = ((j["mi_col_end"] - j["mi_col_start"] - 1) >> 4) + 1
    if src_sb_row * total + src_sb64_col >= active_sb_row * total + active_sb64_col - 4: return 7
    gradient = 1 + 4 + (sb_size > 64)
    if src_sb_row > active_sb_row or src_sb64_col >= active_sb64_col - 4 + gradient * (active_sb_row - src_sb_row): return 8
    if sb_size == 64:
        if src_sb64_col > active_sb64_col + (active_sb_row - src_sb_row): return 9
    elif (((src_right >> 3) - 1) >> 7) > ((mi_col * 4) >> 7) + (active_sb_row - src_sb_row): return 9
    return 0


def job_status(j, w, h, have_tables):
    if (j["block_w"], j["block_h"]) not in SHAPES or j["x_pos"] < 0 or j["y_pos"] < 0 or j["x_pos"] > w - j["block_w"] or j["y_pos"] > h - j["block_h"]: return -1
    if not 0 <= j["step_param"] <= 10 or j["sad_per_bit"] < 0 or j["error_per_bit"] < 0 or j["ibc_shift"] not in (0, 1): return -1
    if not 0 <= j["mib_size_log2"] <= 16 or not all(0 <= j[k] <= 1 << 20 for k in ("mi_row_start", "mi_row_end", "mi_col_start", "mi_col_end")): return -1
    if j["use_hash"] and not have_tables: return -1
    if j["col_max"] < j["col_min"] or j["row_max"] < j["row_min"]: return 1
    if j["x_pos"] + j["col_min"] < 0 or j["x_pos"] + j["col_max"] > w - j["block_w"] or j["y_pos"] + j["row_min"] < 0 or j["y_pos"] + j["row_max"] > h - j["block_h"]: return -1
    fr, fc = j["ref_mv_row"] >> 3, j["ref_mv_col"] >> 3
    if j["row_min"] - fr < -2047 or j["row_max"] - fr > 2047 or j["col_min"] - fc < -2047 or j["col_max"] - fc > 2047: return -1
    return 0


EMPTY_HASH = dict(count=0, n_matched=0, n_valid=0, found=0, best_cost=INT_MAX, best_row=0, best_col=0)


def empty_result(status):
    return dict(status=status, dia_passes=0, dia_refined=0, dia_var=INT_MAX, dia_row=0, dia_col=0, mesh_ran=0, mesh_passes=0, mesh_var=INT_MAX, mesh_row=0, mesh_col=0,
                hash=dict(EMPTY_HASH), source=0, var=INT_MAX, best_row=0, best_col=0, dv_valid=0)


def hash_job(j):
    return H.job(j["x_pos"], j["y_pos"], j["block_w"], j["intra"], limits=(j["col_min"], j["col_max"], j["row_min"], j["row_max"]), ref_mv=(j["ref_mv_row"], j["ref_mv_col"]),
                 epb=j["error_per_bit"], tile=(j["mi_row_start"], j["mi_row_end"], j["mi_col_start"], j["mi_col_end"]), log2=j["mib_size_log2"])


def full_search(plane, bd, table, jc, cc, patterns, j, info=None, mesh=None, p32=None):
    """svt_av1_full_pixel_search (method NSTEP) and the caller's last check for one job -> a result dict.  table (bucket_start, entries) or None; patterns
    [(range, interval)], padded with (0, 0); info, a dict, receives what the stages did; mesh: the scan to use (default: the literal loop for small scans)"""
    info = {} if info is None else info
    h, w = plane.shape
    status = job_status(j, w, h, table is not None)
    R = empty_result(status)
    if status: return R
    patterns = list(patterns) + [(0, 0)] * (MAX_MESH_STEP - len(patterns))
    x = X(p32 if p32 is not None else plane, bd, j, jc, cc)
    if mesh is None:
        mesh = lambda *a: (exhuastive_mesh_search if a[3] * a[3] // (a[4] * a[4]) <= 64 else mesh_search_vectorised)(*a)
    var, best_mv = full_pixel_diamond(x, (j["mvp_row"], j["mvp_col"]), j["step_param"], j["sad_per_bit"], MAX_MVSEARCH_STEPS - 1 - j["step_param"], 1, info)
    R.update(dia_passes=info["passes"], dia_refined=info["refined"], dia_var=var, dia_row=best_mv[0], dia_col=best_mv[1])
    info["thr"] = exhaustive_thr(j)
    if j["exhaustive_allowed"]:
        if var > info["thr"]:
            var_ex, mv_ex = full_pixel_exhaustive(x, best_mv, j["sad_per_bit"], patterns, info, mesh)
            R.update(mesh_ran=1, mesh_passes=len(info["mesh_passes"]), mesh_var=var_ex, mesh_row=mv_ex[0], mesh_col=mv_ex[1])
            if var_ex < var:
                var, best_mv = var_ex, mv_ex
                R["source"] = 1
    if j["block_w"] == j["block_h"] and j["use_hash"]:
        R["hash"] = H.search(plane, bd, table[0], table[1], jc, cc, hash_job(j))
        if R["hash"]["found"] and R["hash"]["best_cost"] < var:
            var, best_mv = R["hash"]["best_cost"], (R["hash"]["best_row"], R["hash"]["best_col"])
            R["source"] = 2
    info["n_sad"] = x.n_sad
    R.update(var=var, best_row=best_mv[0], best_col=best_mv[1], dv_valid=int(dv_rule(j, *best_mv) == 0))
    return R


# ---------------------------------------------------------------------------------------------------------------- jobs
def job(x, y, bw, bh, limits, w, h, ref_mv=(0, 0), mvp=None, step_param=0, spb=30, epb=40, ex=None, shift=0, use_hash=0, intra=1, tile=None, log2=4):
    """limits (col_min, col_max, row_min, row_max); mvp default ref_mv >> 3 as the caller sets it; ex default is_exhaustive_allowed's rule"""
    tile = tile or (0, (h + 3) // 4, 0, (w + 3) // 4)
    mvp = mvp if mvp is not None else (ref_mv[0] >> 3, ref_mv[1] >> 3)
    ex = int(bw == 4 or bh == 4) if ex is None else ex
    return dict(zip(JOB_FIELDS, (x, y, bw, bh, intra) + tuple(limits) + tuple(ref_mv) + tuple(mvp) + (step_param, spb, epb, ex, shift, use_hash) + tuple(tile) + (log2,)))


def picture_limits(x, y, bw, bh, w, h):
    """the widest limits that keep the block inside the picture"""
    return (-x, w - bw - x, -y, h - bh - y)


def open_limits(x, y, bw, bh, w, h):
    """the widest limits inside the picture that keep a candidate off the block itself (a SAD of 0 at the zero vector would end every search at once): everything
    above it, else everything to its left, else (a block that nearly fills the picture) everything but the zero vector's column"""
    if y >= bh: return (-x, w - bw - x, -y, -bh)
    if x >= bw: return (-x, -bw, -y, h - bh - y)
    return (1, w - bw - x, -y, h - bh - y) if x < w - bw else (-x, -1, -y, h - bh - y)


def caller_limits(x, y, bw, bh, w, h, direction, log2=4):
    """x->mv_limits as intra_bc_search builds them (EbModeDecision.c:4461-4476) for one tile that is the picture, cut to the picture"""
    mi_row, mi_col, sb = y // 4, x // 4, 1 << log2
    rows, cols = (h + 3) // 4, (w + 3) // 4
    if direction == "above":
        lim = (-mi_col * 4, (cols - mi_col) * 4 - bw, -mi_row * 4, ((mi_row >> log2) * sb - mi_row) * 4 - bh)
    else:
        lim = (-mi_col * 4, ((mi_col >> log2) * sb - mi_col) * 4 - bw, -mi_row * 4, (min(((mi_row >> log2) + 1) * sb, rows) - mi_row) * 4 - bh)
    pic = picture_limits(x, y, bw, bh, w, h)
    return (max(lim[0], pic[0]), min(lim[1], pic[1]), max(lim[2], pic[2]), min(lim[3], pic[3]))


def wide_strip(seed=11):
    """640 x 40: a noisy left part and a right part of blocks repeated from far left, so that a {256, 1} scan is bounded by its range, not by the limits"""
    rng = np.random.default_rng(seed)
    pic = rng.integers(0, 256, (40, 640)).astype(np.uint8)
    pic[:, 320:] = (pic[:, 320:] >> 3) + 100   # low contrast: nearby vectors give moderate SADs
    pic[8:24, 560:576] = pic[12:28, 330:346]   # a copy 230 columns to the left and 4 rows down
    return pic


def ramp(w=136, h=130, seed=12):
    """a smooth slope with a little noise: the SAD falls steadily towards a line far from where a walk starts, so short walks end while still moving"""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.clip((xs + 2 * ys) * 250 // (w + 2 * h) + np.random.default_rng(seed).integers(0, 3, (h, w)), 0, 255).astype(np.uint8)


def shape_jobs(pic, shapes, seed, per_shape=3, lo=64, wide=False, **kw):
    """jobs of the given shapes at positions on the 4-sample grid from `lo` on (so that the superblock above and the one to the left exist), with both of the
    caller's limits, or with the widest limits the picture allows"""
    h, w = pic.shape
    rng = np.random.default_rng(seed)
    jobs = []
    for bw, bh in shapes:
        if bw > w or bh > h: continue
        for k in range(per_shape):
            x0, y0 = min(lo, w - bw) // 4, min(max(lo, bh) if wide else lo, h - bh) // 4
            x, y = int(rng.integers(x0, (w - bw) // 4 + 1)) * 4, int(rng.integers(y0, (h - bh) // 4 + 1)) * 4
            ref = (int(rng.integers(-6, 1)) * 8, int(rng.integers(-6, 1)) * 8) if k else (0, 0)
            args = dict(ref_mv=ref, shift=k & 1, use_hash=int(bw == bh), step_param=(0, 0, 3, 6)[k % 4])
            args.update(kw)
            for lim in ([open_limits(x, y, bw, bh, w, h)] if wide else [caller_limits(x, y, bw, bh, w, h, d) for d in ("above", "left")]):
                jobs.append(job(x, y, bw, bh, lim, w, h, **args))
    return jobs


def glyph_jobs(pic, seed, n=40, **kw):
    """square blocks that start on a glyph of ibc_hash_common.text_like (off the 4-sample grid), both limits: equal glyphs elsewhere are what the hash finds"""
    h, w = pic.shape
    rng = np.random.default_rng(seed)
    jobs = []
    for k in range(n):
        s = (4, 8, 8, 16)[k % 4]
        x, y = 4 + 6 * int(rng.integers(11, (w - 24) // 6)), 4 + 10 * int(rng.integers(7, (h - 24) // 10))
        for d in ("above", "left"):
            jobs.append(job(x, y, s, s, caller_limits(x, y, s, s, w, h, d), w, h, use_hash=1, shift=k & 1, **kw))
    return jobs


def cases():
    """[dict(name, pic (8-bit), jobs, patterns, zero)]; every list is small enough for the literal loops except the `full` scans, which take the vectorised one"""
    out = []
    # text: repeated glyphs: the hash wins, the diamond gets stuck, the mesh finds copies; every shape, both limits
    pic = H.text_like(352, 240)
    out.append(dict(name="text_shapes", pic=pic, jobs=shape_jobs(pic, SHAPES, 1, per_shape=3), patterns=PATTERNS["two"], zero=False))
    out.append(dict(name="text_glyphs", pic=pic, jobs=glyph_jobs(pic, 2), patterns=PATTERNS["two"], zero=False))
    small = [(4, 4), (4, 8), (8, 4), (4, 16), (16, 4), (8, 8), (16, 16)]
    out.append(dict(name="text_four", pic=pic, jobs=shape_jobs(pic, small, 3, per_shape=4, ex=1), patterns=PATTERNS["four"], zero=False))
    out.append(dict(name="text_invalid", pic=pic, jobs=shape_jobs(pic, small[:5], 4, per_shape=2), patterns=PATTERNS["invalid"], zero=False))
    # noise: large variances: the threshold is passed at shift 0 and 1 for the larger 4-wide shapes, the diamond wanders
    pic = H.noise(136, 130, seed=8)
    out.append(dict(name="noise", pic=pic, jobs=shape_jobs(pic, SHAPES, 5, per_shape=2), patterns=PATTERNS["two"], zero=False))
    out.append(dict(name="noise_open", pic=pic, jobs=shape_jobs(pic, SHAPES, 9, per_shape=1, lo=0, wide=True, intra=0), patterns=PATTERNS["two"], zero=False))
    out.append(dict(name="noise_full", pic=pic, jobs=shape_jobs(pic, small[:5], 2, per_shape=3), patterns=PATTERNS["full"], zero=False))
    out.append(dict(name="noise_four", pic=pic, jobs=shape_jobs(pic, small, 6, per_shape=3), patterns=PATTERNS["four"], zero=False))
    # tiled: period 8: many equal candidates, and with all-zero cost tables nothing but the scan order tells them apart
    pic = H.tiled(136, 130)
    out.append(dict(name="tiled_zero", pic=pic, jobs=shape_jobs(pic, small, 7, per_shape=3, ex=1, intra=0), patterns=PATTERNS["two"], zero=True))
    # flat: every SAD is 0: the cost alone decides
    pic = H.flat(72, 40)
    out.append(dict(name="flat", pic=pic, jobs=shape_jobs(pic, small, 8, per_shape=2, lo=0, wide=True, ex=1, intra=0), patterns=PATTERNS["full"], zero=False))
    # a slope: short walks (a large step_param) that are still moving when they end: the refinement moves, up to all 8 rounds
    pic = ramp()
    jobs = [j for sp in (7, 8, 9, 10) for j in shape_jobs(pic, small + [(32, 32)], 20 + sp, per_shape=2, lo=0, wide=True, step_param=sp, intra=0)]
    out.append(dict(name="ramp", pic=pic, jobs=jobs, patterns=PATTERNS["two"], zero=False))
    # the wide strip: the range, not the limits, bounds the scan
    pic = wide_strip()
    h, w = pic.shape
    jobs = [job(x, y, bw, bh, open_limits(x, y, bw, bh, w, h), w, h, shift=s) for (bw, bh) in ((4, 4), (4, 16), (16, 4)) for (x, y) in ((300, 20), (560, 24), (20, 16))
            for s in (0, 1)]
    out.append(dict(name="strip", pic=pic, jobs=jobs, patterns=PATTERNS["full"], zero=False))
    # four scans whose centre moves: the issue's own four patterns end after the third (its interval is 1)
    pic = H.noise(136, 130, seed=8)
    out.append(dict(name="noise_deep", pic=pic, jobs=shape_jobs(pic, small[:5], 13, per_shape=3), patterns=PATTERNS["deep"], zero=False))
    out += planted_cases()
    return out


THR_DIFFS = {32768: (1, 79, 13, -82), 32769: (1, 66, 7, 93)}   # k samples of a and m of b above a flat 100, the rest 0: sse - sum^2 / 16 is the key
COLS_ROWS, COLS_MIN = (-12, -6), -40                           # the limits of the planted jobs; the copy lies in row -8


def planted_cols_layout():
    """[(number of columns, the copy's column counted from col_max: 0 the last, 1 the one before)] of the planted_cols jobs, in order"""
    return [(n, back) for n in (16, 17, 18, 19) for back in (0, 1)]


def planted_cases():
    """pictures made for one condition each, flat but for what is planted:
      planted_cols  a block of noise and ONE exact copy of it, in the last column of a step-1 scan or in the one before, for every remainder of the number of
                    columns by 4: the reference never examines the last column unless the remainder is 0
      planted_thr   (all-zero cost tables) blocks whose variance against the flat page is exactly the threshold and one above; and a block with TWO exact copies,
                    (r1, c1) and (r2, c2) with r1 < r2 and c1 > c2: row-major order meets the first first, column-major order the second"""
    out = []
    layout = planted_cols_layout()
    rng = np.random.default_rng(21)
    pic = np.full((24 * len(layout), 72), 100, np.uint8)
    jobs = []
    for k, (n, back) in enumerate(layout):
        x, y = 48, 24 * k + 16
        blk = rng.integers(0, 256, (4, 4)).astype(np.uint8)
        col = COLS_MIN + n - 1 - back
        pic[y:y + 4, x:x + 4] = blk
        pic[y - 8:y - 4, x + col:x + col + 4] = blk
        jobs.append(job(x, y, 4, 4, (COLS_MIN, COLS_MIN + n - 1) + COLS_ROWS, 72, pic.shape[0], mvp=(COLS_ROWS[0], COLS_MIN), step_param=10, intra=0))   # the diamond starts in the far corner and cannot reach the copy
    out.append(dict(name="planted_cols", pic=pic, jobs=jobs, patterns=PATTERNS["full"], zero=False))
    pic = np.full((72, 72), 100, np.uint8)
    jobs = []
    for k, (thr, (ka, a, kb, b)) in enumerate(sorted(THR_DIFFS.items())):
        x, y = 48, 24 * k + 16
        d = np.array([a] * ka + [b] * kb + [0] * (16 - ka - kb)).reshape(4, 4)
        pic[y:y + 4, x:x + 4] = 100 + d
        jobs.append(job(x, y, 4, 4, (COLS_MIN, COLS_MIN + 19) + COLS_ROWS, 72, 72, intra=0))
    x, y = 48, 64
    blk = rng.integers(0, 256, (4, 4)).astype(np.uint8)
    pic[y:y + 4, x:x + 4] = blk
    for r, c in TIE_COPIES: pic[y + r:y + r + 4, x + c:x + c + 4] = blk
    jobs.append(job(x, y, 4, 4, (COLS_MIN, COLS_MIN + 19) + COLS_ROWS, 72, 72, intra=0))
    out.append(dict(name="planted_thr", pic=pic, jobs=jobs, patterns=PATTERNS["full"], zero=True))
    return out


TIE_COPIES = [(-12, -30), (-7, -38)]


BAD_JOBS = [dict(block_w=12), dict(block_w=128, block_h=32), dict(block_h=2), dict(block_w=256, block_h=256), dict(x_pos=-4), dict(y_pos=10 ** 6), dict(step_param=-1),
            dict(step_param=11), dict(sad_per_bit=-1), dict(error_per_bit=-1), dict(ibc_shift=2), dict(mib_size_log2=17), dict(mi_row_start=-1), dict(mi_col_end=(1 << 20) + 1),
            dict(col_min=-10 ** 6), dict(col_max=10 ** 6), dict(row_min=-10 ** 6), dict(row_max=10 ** 6), dict(ref_mv_row=8 * 3000), dict(ref_mv_col=-8 * 3000)]
EMPTY_JOBS = [dict(col_min=5, col_max=4), dict(row_min=1, row_max=0)]


def c_jobs(pkg, jobs):
    tab = (pkg.IbcFullSearchJob * len(jobs))()
    for i, j in enumerate(jobs):
        for k in JOB_FIELDS: setattr(tab[i], k, j[k])
    return tab


def c_results(res, n):
    out = []
    for i in range(n):
        r = {k: getattr(res[i], k) for k in RESULT_FIELDS if k != "hash"}
        r["hash"] = {k: getattr(res[i].hash, k) for k in H.RESULT_FIELDS}
        out.append(r)
    return out
