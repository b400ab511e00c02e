"""GPU: svt_hip_intra_predict_batch_dev, bit-exact against the reference's C predictors and edge operations (tests/intra_common.py: ref_predict)."""
import numpy as np
import pytest

import intra_common as ic

pytestmark = pytest.mark.gpu
CHUNK = 4096
BDS = [(np.uint8, 8), (np.uint16, 10), (np.uint16, 8)]   # (uint16, 8): 8-bit samples in 16-bit planes, what the encoder's 16-bit pipeline hands over for 8-bit video


def _check(hip, pkg, L, recs, jobs, bd, what):
    """Every block against the reference's predictors of the records' sample type (uint16: the high-bit-depth functions with this bd).  8-bit samples in 16-bit
    planes have a second witness, the same records as uint8: the reference's 8-bit functions give the same blocks (asserted here, on the CPU), and so does the device."""
    ic.prepare(L)
    assert len(jobs) == len(recs)
    wide = recs.dtype == np.uint16 and bd == 8
    lo, hi = 1 << 16, 0
    for s in range(0, len(jobs), CHUNK):
        blocks, _ = ic.run_batch(hip, pkg, recs[s:s + CHUNK], jobs[s:s + CHUNK], bd)
        if wide: blocks8, _ = ic.run_batch(hip, pkg, recs[s:s + CHUNK].astype(np.uint8), jobs[s:s + CHUNK], 8)
        for i, (j, got) in enumerate(zip(jobs[s:s + CHUNK], blocks)):
            exp = ic.ref_predict(L, recs[s + i], bd, j)
            assert (got == exp).all(), f"{what}: job {s + i} {j} differs at {np.argwhere(got != exp)[0].tolist()}"
            if wide:
                exp8 = ic.ref_predict(L, np.ascontiguousarray(recs[s + i].astype(np.uint8)), 8, j)
                assert exp8.dtype == np.uint8 and (exp == exp8).all(), f"{what}: job {s + i} {j}: the reference's 8-bit and high-bit-depth predictors differ"
                assert (got == blocks8[i]).all(), f"{what}: job {s + i} {j}: the device's (2, 8) and (1, 8) results differ"
                lo, hi = min(lo, int(exp.min())), max(hi, int(exp.max()))
    if wide: assert (lo, hi) == (0, 255), (what, lo, hi)


def _extremes(recs, dtype, bd):
    """8-bit samples in 16-bit planes: every ninth record all max, the next all 0, the next alternating 0 / max (the other formats keep their content)"""
    if dtype == np.uint16 and bd == 8:
        recs[::9] = 255; recs[1::9] = 0; recs[2::9, :, ::2] = 0; recs[2::9, :, 1::2] = 255
    return recs


def _records_for(rng, jobs_per_kind, dtype, bd, n_kinds):
    """`jobs_per_kind` random records per kind plus one all-zero and one all-max record; 8-bit samples in 16-bit planes: the first of each kind alternates 0 / max."""
    per = jobs_per_kind + 2
    recs = ic.random_records(rng, per * n_kinds, dtype, bd)
    if dtype == np.uint16 and bd == 8:
        recs[::per, :, ::2] = 0; recs[::per, :, 1::2] = 255
    recs[jobs_per_kind::per] = 0
    recs[jobs_per_kind + 1::per] = (1 << bd) - 1
    return recs, per


@pytest.mark.parametrize("dtype,bd", BDS)
def test_non_directional(hip, pkg, ref, dtype, bd):
    kinds = [dict(mode=0, dc_have=h) for h in range(4)] + [dict(mode=m) for m in (9, 10, 11, 12)]
    kinds = [dict(k, tx_size=t) for t in range(19) for k in kinds]
    recs, per = _records_for(np.random.default_rng(100 + bd), 4, dtype, bd, len(kinds))
    jobs = [ic.make_job(**k) for k in kinds for _ in range(per)]
    _check(hip, pkg, ref, recs, jobs, bd, "non-directional")


def directional_job(L, tx, mode, delta, filt_type):
    """The conditioning build_intra_predictors (Common/Codec/EbIntraPrediction.c) derives for a directional block with every neighbour available."""
    ic.prepare(L)
    w, h = ic.TX_WH[tx]
    ang = ic.ANGLE[mode] + 3 * delta
    need_above, need_left = ang < 180, ang > 90
    need_right, need_bottom = ang < 90, ang > 180
    j = dict(tx_size=tx, mode=mode, angle_delta=delta, start_m1=1)
    if ang != 90 and ang != 180:
        j["corner_filter"] = int(need_above and need_left and w + h >= 24)
        if need_above:
            j["strength_above"] = L.intra_edge_filter_strength(w, h, ang - 90, filt_type)
            j["npx_above"] = min(w + 1 + (h if need_right else 0), 129)
        if need_left:
            j["strength_left"] = L.intra_edge_filter_strength(h, w, ang - 180, filt_type)
            j["npx_left"] = min(h + 1 + (w if need_bottom else 0), 129)
    if need_above and L.use_intra_edge_upsample(w, h, ang - 90, filt_type):
        j["upsample_above"] = 1; j["up_npx_above"] = w + (h if need_right else 0)
    if need_left and L.use_intra_edge_upsample(h, w, ang - 180, filt_type):
        j["upsample_left"] = 1; j["up_npx_left"] = h + (w if need_bottom else 0)
    return ic.make_job(**j)


@pytest.mark.parametrize("dtype,bd", BDS)
def test_directional(hip, pkg, ref, dtype, bd):
    """8 base angles x 7 deltas x 19 sizes, edge filter / corner filter / up-sampling as the codec derives them (up-sampling wherever use_intra_edge_upsample
    allows it, for both filter types), V and H included."""
    rng = np.random.default_rng(200 + bd)
    kinds = [(t, m, d) for t in range(19) for m in range(1, 9) for d in range(-3, 4)]
    recs, per = _records_for(rng, 4, dtype, bd, len(kinds))
    jobs = [directional_job(ref, t, m, d, i & 1) for (t, m, d) in kinds for i in range(per)]
    assert sum(j["upsample_above"] for j in jobs) > 100 and sum(j["upsample_left"] for j in jobs) > 100
    assert {j["strength_above"] for j in jobs} == {0, 1, 2, 3} and sum(j["corner_filter"] for j in jobs) > 100
    _check(hip, pkg, ref, recs, jobs, bd, "directional")


@pytest.mark.parametrize("dtype,bd", BDS)
def test_edge_filter_alone(hip, pkg, ref, dtype, bd):
    """Strengths 1-3 over 5 .. 129 samples, seen through 64x64 predictions that copy (V: above 0..63, D45: above 1..127, H: left 0..63) or interpolate
    (D203: the left edge down to sample 127) the conditioned edge."""
    rng = np.random.default_rng(300 + bd)
    jobs = []
    for n in range(5, 130):
        for s in (1, 2, 3):
            for m1 in (0, 1):
                jobs.append(ic.make_job(tx_size=4, mode=1, strength_above=s, npx_above=n, start_m1=m1))
                jobs.append(ic.make_job(tx_size=4, mode=3, strength_above=s, npx_above=n, start_m1=m1))
                jobs.append(ic.make_job(tx_size=4, mode=2, strength_left=s, npx_left=n, start_m1=m1))
                jobs.append(ic.make_job(tx_size=4, mode=7, angle_delta=3, strength_left=s, npx_left=n, start_m1=m1))
    recs = _extremes(ic.random_records(rng, len(jobs), dtype, bd), dtype, bd)
    _check(hip, pkg, ref, recs, jobs, bd, "edge filter")


@pytest.mark.parametrize("dtype,bd", BDS)
def test_corner_and_upsample_alone(hip, pkg, ref, dtype, bd):
    rng = np.random.default_rng(400 + bd)
    jobs = []
    for t in (0, 1, 2, 5, 6, 7, 8):
        for m in (4, 5, 6):
            for d in (-3, 0, 3):
                jobs += [ic.make_job(tx_size=t, mode=m, angle_delta=d, corner_filter=1)] * 2
    for t in (0, 5, 6, 1):
        for n in (4, 8, 12, 16):
            for d in range(-3, 4):
                jobs.append(ic.make_job(tx_size=t, mode=3, angle_delta=d, upsample_above=1, up_npx_above=n))
                jobs.append(ic.make_job(tx_size=t, mode=8, angle_delta=d, upsample_above=1, up_npx_above=n))
                jobs.append(ic.make_job(tx_size=t, mode=7, angle_delta=d, upsample_left=1, up_npx_left=n))
                jobs.append(ic.make_job(tx_size=t, mode=4, angle_delta=d, upsample_above=1, up_npx_above=n, upsample_left=1, up_npx_left=n))
                jobs.append(ic.make_job(tx_size=t, mode=5, angle_delta=d, upsample_above=1, up_npx_above=n))
                jobs.append(ic.make_job(tx_size=t, mode=6, angle_delta=d, upsample_left=1, up_npx_left=n))
    recs = ic.random_records(rng, len(jobs), dtype, bd)
    recs[::7] = (1 << bd) - 1
    recs[3::7, :, ::2] = 0   # alternating extremes: the up-sampling filter overshoots and is clipped
    if dtype == np.uint16 and bd == 8: recs[5::7] = 0      # 8-bit samples in 16-bit planes carry all-0 records too
    _check(hip, pkg, ref, recs, jobs, bd, "corner / up-sampling")


@pytest.mark.parametrize("dtype,bd", BDS)
def test_mixed_batch_guard_and_empty(hip, pkg, ref, dtype, bd):
    """All sizes and modes in one launch in random order; a job with tx_size = 19 (and one with mode 13, one with angle_delta 4) leaves its destination
    untouched while every other job is right; njobs == 0 is accepted."""
    rng = np.random.default_rng(500 + bd)
    jobs = [directional_job(ref, t, m, int(rng.integers(-3, 4)), int(rng.integers(0, 2))) for t in range(19) for m in range(1, 9)]
    jobs += [ic.make_job(tx_size=t, mode=m, dc_have=int(rng.integers(0, 4))) for t in range(19) for m in (0, 9, 10, 11, 12)]
    order = rng.permutation(len(jobs))
    jobs = [jobs[i] for i in order]
    bad_at = {17: dict(tx_size=19), 101: dict(mode=13), 202: dict(angle_delta=4, mode=3)}
    good = list(jobs)
    for i, chg in bad_at.items():
        jobs[i] = dict(jobs[i]); jobs[i].update(chg)
    recs = _extremes(ic.random_records(rng, len(jobs), dtype, bd), dtype, bd)
    blocks, plane = ic.run_batch(hip, pkg, recs, jobs, bd)
    marker = 0x5A if dtype == np.uint8 else 0x2A5
    for i, (j, got) in enumerate(zip(jobs, blocks)):
        if i in bad_at:
            cell = plane[(i // 16) * 64:(i // 16) * 64 + 64, (i % 16) * 64:(i % 16) * 64 + 64]
            assert (cell == marker).all(), f"guarded job {i} wrote something"
        else:
            assert (got == ic.ref_predict(ref, recs[i], bd, good[i])).all(), f"job {i} {j}"
    # the same jobs in another order give the same blocks
    perm = rng.permutation(len(good))
    blocks2, _ = ic.run_batch(hip, pkg, recs[perm], [good[i] for i in perm], bd)
    for k, i in enumerate(perm):
        if i not in bad_at: assert (blocks2[k] == blocks[i]).all()
    blocks0, plane0 = ic.run_batch(hip, pkg, recs[:0], [], bd)
    assert blocks0 == [] and (plane0 == marker).all()


def test_bad_arguments_with_a_context(hip, pkg):
    L = pkg.lib()
    d = hip.empty(4096)
    f = lambda **k: L.svt_hip_intra_predict_batch_dev(hip.h, k.get("pix_bytes", 1), k.get("bd", 8), k.get("e", d), k.get("j", d), k.get("n", 0), k.get("dst", d),
                                                      k.get("stride", 64))
    try:
        assert f() == 0 and f(pix_bytes=2, bd=10) == 0 and f(pix_bytes=2, bd=8) == 0
        for bad in (dict(pix_bytes=3), dict(pix_bytes=0), dict(bd=12), dict(bd=10), dict(n=-1), dict(stride=0), dict(e=None), dict(j=None), dict(dst=None)):
            assert f(**bad) == 2, bad
    finally:
        hip.free(d)
