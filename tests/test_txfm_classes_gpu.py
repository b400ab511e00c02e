"""GPU: the mixed-size transform entry points cut a call into one launch per size class (svt-av1_amd/csrc/txfm_plan.h).  One call whose jobs interleave the classes
(64x64, 4x4, 32x8, 8x8, 16x4, 4x4, ...), holds 18 jobs of 4- and 8-point sizes (more than one launch of that class), an empty job and block counts that leave ragged
last workgroups (65 blocks of 4x4, 3 of 64x64) must reproduce the single-size entry points bit for bit (tests/test_txfm_gpu.py holds those against the oracle):
levels, dequantised coefficients where requested, eob, cul_level, the discarded energy of the 64-point sizes, and the reconstruction.  Every job reconstructs
into ONE plane pre-filled with a pattern and the whole plane is compared: a block lost between two launches, or a stray store, shows."""
import numpy as np
import pytest

import txfm_common as tc
from test_oracle_golden import T
from test_txfm_gpu import qparams_struct, run_fwd, run_inv

pytestmark = pytest.mark.gpu

Wp, Hp = 1024, 512
# (tx_size, blocks) in caller order: the classes interleaved, then 4- and 8-point sizes until that class has 18 jobs; job 13 is empty
JOBS = [(4, 3), (0, 65), (16, 5), (1, 33), (14, 17), (0, 7), (12, 3), (5, 40), (2, 17), (6, 9), (11, 5), (13, 20), (3, 9), (7, 0), (7, 19), (18, 6), (15, 11),
        (8, 21), (17, 5), (9, 10), (10, 7)] + [((0, 1, 5, 6)[k % 4], 1 + 11 * k) for k in range(13)]
assert sum(1 for ts, n in JOBS if n and max(tc.TXW[ts], tc.TXH[ts]) <= 8) == 18


def place():
    """-> per job the (x, y) of its blocks: shelves of jobs side by side, no two blocks of the plane overlap"""
    pos, x0, y0, shelf = [], 0, 0, 0
    for ts, n in JOBS:
        w, h = tc.TXW[ts], tc.TXH[ts]
        if x0 + n * w > Wp: x0, y0, shelf = 0, y0 + shelf, 0
        pos.append([(x0 + k * w, y0) for k in range(n)])
        x0 += n * w; shelf = max(shelf, h if n else 0)
    assert y0 + shelf <= Hp
    return pos


@pytest.fixture(scope="module", params=[(8, np.uint8), (8, np.uint16), (10, np.uint16)], ids=["u8-8", "u16-8", "u16-10"])
def case(request, hip, pkg):
    """the planes, the jobs' device inputs and what the single-size entry points give for every job; computed once per format, read by the three tests"""
    bd, dt = request.param
    rng = np.random.default_rng(4100 + bd + np.dtype(dt).itemsize)
    src = rng.integers(0, 1 << bd, (Hp, Wp)).astype(dt); pred = rng.integers(0, 1 << bd, (Hp, Wp)).astype(dt)
    yy, xx = np.mgrid[0:Hp, 0:Wp]
    fill = ((3 * xx + 7 * yy + 1) % ((1 << bd) - 1) + 1).astype(dt)      # what the reconstruction plane holds before the call: never 0
    qp = np.ascontiguousarray(T[f"qp/{bd}/60/0"]); variant = 0 if bd == 8 else 1
    c = dict(bd=bd, dt=dt, pix=np.dtype(dt).itemsize, d_src=hip.to_device(src), d_pred=hip.to_device(pred), fill=fill, jobs=[], keep=[])
    c["exp_rec"] = fill.copy()
    for (ts, n), pos in zip(JOBS, place()):
        w, h = tc.TXW[ts], tc.TXH[ts]
        tts = tc.legal_types(ts)
        descs = np.array([pkg.tx_desc(x, y, tts[k % len(tts)]) for k, (x, y) in enumerate(pos)], np.uint32)
        j = dict(ts=ts, n=n, nk=min(w, 32) * min(h, 32), scans=pkg.ScanTables(), qs=qparams_struct(pkg, qp, variant, tc.TX_SCALE[ts]), d_desc=hip.to_device(descs))
        c["keep"].append(j["d_desc"])
        for cls in range(3):
            if f"iscan/{ts}/{cls}" in T.files:
                p = hip.to_device(np.ascontiguousarray(T[f"iscan/{ts}/{cls}"])); c["keep"].append(p); j["scans"].iscan[cls] = p.value
        if n:
            j["exp"] = run_fwd(hip, pkg, ts, bd, src, pred, descs, qp, variant)
            rec = run_inv(hip, ts, bd, j["exp"]["dq"], pred, descs)
            for x, y in pos: c["exp_rec"][y:y + h, x:x + w] = rec[y:y + h, x:x + w]
        c["jobs"].append(j)
    assert not np.array_equal(c["exp_rec"], fill)
    yield c
    hip.free(c["d_src"], c["d_pred"], *c["keep"])


def outputs(hip, c, names):
    """fresh device outputs per job, pre-filled with 0x5A bytes -> [{name: pointer}]"""
    size = dict(co=lambda j: j["n"] * j["nk"] * 4, q=lambda j: j["n"] * j["nk"] * 4, dq=lambda j: j["n"] * j["nk"] * 4, eob=lambda j: j["n"] * 2,
                cul=lambda j: j["n"] * 4, en=lambda j: j["n"] * 8)
    return [{k: hip.to_device(np.full(max(size[k](j), 4), 0x5A, np.uint8)) for k in names} for j in c["jobs"]]


def compare(hip, c, outs, pairs, what):
    for i, (j, o) in enumerate(zip(c["jobs"], outs)):
        if not j["n"]: continue
        for k, e in pairs:
            if k not in o: continue
            exp = j["exp"][e]
            assert np.array_equal(hip.to_host(o[k], exp.shape, exp.dtype), exp), (what, e, "job", i, "tx_size", j["ts"])


def test_forward_and_inverse(hip, pkg, case):
    c = case
    outs = outputs(hip, c, ("co", "q", "dq", "eob", "cul", "en"))
    d_rec = hip.to_device(c["fill"])
    fj = (pkg.FwdTxJob * len(JOBS))(); ij = (pkg.InvTxJob * len(JOBS))()
    for i, (j, o) in enumerate(zip(c["jobs"], outs)):
        fj[i] = pkg.FwdTxJob(j["ts"], j["n"], c["d_src"].value, Wp, c["d_pred"].value, Wp, j["d_desc"].value, j["qs"], j["scans"], o["co"].value, o["q"].value,
                             o["dq"].value, o["eob"].value, o["cul"].value, o["en"].value)
        ij[i] = pkg.InvTxJob(j["ts"], j["n"], o["dq"].value, c["d_pred"].value, Wp, d_rec.value, Wp, j["d_desc"].value)
    hip.check(hip.L.svt_hip_fwd_txfm_quant_multi_dev(hip.h, c["pix"], fj, len(JOBS)), "fwd multi")
    compare(hip, c, outs, (("co", "coeff"), ("q", "q"), ("dq", "dq"), ("eob", "eob"), ("cul", "cul"), ("en", "energy")), "forward")
    hip.check(hip.L.svt_hip_inv_txfm_add_multi_dev(hip.h, c["pix"], c["bd"], ij, len(JOBS)), "inv multi")
    rec = hip.to_host(d_rec, (Hp, Wp), c["dt"])
    hip.free(d_rec, *[p for o in outs for p in o.values()])
    assert np.array_equal(rec, c["exp_rec"]), ("inverse", np.argwhere(rec != c["exp_rec"])[:4])


def test_fused(hip, pkg, case):
    c = case
    outs = outputs(hip, c, ("q", "dq", "eob", "cul", "en"))
    for i, o in enumerate(outs):
        if i % 2: hip.free(o.pop("dq"))            # every other job asks for no dequantised coefficients
    d_rec = hip.to_device(c["fill"])
    ej = (pkg.EncTxJob * len(JOBS))()
    for i, (j, o) in enumerate(zip(c["jobs"], outs)):
        ej[i].fwd = pkg.FwdTxJob(j["ts"], j["n"], c["d_src"].value, Wp, c["d_pred"].value, Wp, j["d_desc"].value, j["qs"], j["scans"], None, o["q"].value,
                                 o["dq"].value if "dq" in o else None, o["eob"].value, o["cul"].value, o["en"].value)
        ej[i].d_recon = d_rec.value; ej[i].recon_stride = Wp
    hip.check(hip.L.svt_hip_enc_txfm_multi_dev(hip.h, c["pix"], c["bd"], ej, len(JOBS)), "enc multi")
    compare(hip, c, outs, (("q", "q"), ("dq", "dq"), ("eob", "eob"), ("cul", "cul"), ("en", "energy")), "fused")
    rec = hip.to_host(d_rec, (Hp, Wp), c["dt"])
    hip.free(d_rec, *[p for o in outs for p in o.values()])
    assert np.array_equal(rec, c["exp_rec"]), ("fused reconstruction", np.argwhere(rec != c["exp_rec"])[:4])
