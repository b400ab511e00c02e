"""CPU: bench.py --dump-outputs on stand-in frame buffers (host tensors shaped as a Pipeline's): every output of every frame of the batch is written, exactly
(float32 / float64), within the size limit, larger arrays as the seeded sample manifest.json describes, and the same files on a second run."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _frame(seed, W=640, H=360):
    g = torch.Generator().manual_seed(seed)
    ri = lambda shape, hi, dt: torch.randint(0, hi, shape, generator=g, dtype=dt)
    n_sb = ((W + 63) // 64) * ((H + 63) // 64)
    cur = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
    P = types.SimpleNamespace(F=types.SimpleNamespace(seed=seed, w=W, h=H, cur=cur))
    P.d_sad, P.d_mv = ri((n_sb, 85), 1 << 20, torch.int32), ri((n_sb, 85), (1 << 31) - 1, torch.int32)
    P.d_mse, P.d_sel_gi = ri((2, n_sb, 64), 1 << 40, torch.int64), ri((n_sb,), 8, torch.int32)
    P.d_cy, P.d_cuv, P.d_fin = ri((n_sb,), 64, torch.uint8), ri((n_sb,), 64, torch.uint8), ri((88,), 16, torch.uint8)
    P.tx_jobs = [dict(q=ri((W * H // 2,), 1 << 16, torch.int32) - (1 << 15), eob=ri((W * H // 32,), 1024, torch.int16)) for _ in range(2)]
    P.d_ubest = [ri((6,), 16, torch.uint8) for _ in range(3)]
    P.d_ubx = [ri((6, 2), 128, torch.int32) for _ in range(3)]
    P.b_rest = [ri((p.shape[0] + 2 * bench.EXT, p.shape[1] + 64), 256, torch.uint8) for p in cur]
    return P


def test_dump_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 20)
    batch = [_frame(s) for s in (3, 4)]
    args = types.SimpleNamespace(steps=5, warmup=1)
    bench.dump_outputs(str(tmp_path / "a"), batch, args)
    bench.dump_outputs(str(tmp_path / "b"), batch, args)
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    npy = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert npy == sorted(k + ".npy" for k in man["arrays"]) and len(npy) == 2 * 18
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in npy) <= 1 << 20
    P = batch[1]
    src = {"me_mv": P.d_mv.numpy(), "cdef_mse": P.d_mse.numpy(), "coeff": torch.cat([j["q"] for j in P.tx_jobs]).numpy(),
           "restored_u": P.b_rest[1][bench.EXT:bench.EXT + 180, bench.EXT:bench.EXT + 320].numpy(), "sgr_xqd_v": P.d_ubx[2].numpy()}
    for k, ref in src.items():
        a, m = np.load(tmp_path / "a" / f"f1_{k}.npy"), man["arrays"][f"f1_{k}"]
        assert a.dtype in (np.float32, np.float64) and m["shape"] == list(ref.shape)
        if m["sample"] is None:
            assert np.array_equal(a, ref.astype(np.float64))
        else:
            idx = np.sort(np.random.default_rng(m["sample"]["seed"]).choice(ref.size, m["sample"]["count"], replace=False))
            assert np.array_equal(a, ref.reshape(-1)[idx].astype(np.float64))
    assert man["arrays"]["f1_me_mv"]["saved_dtype"] == "float64" and man["arrays"]["f1_coeff"]["saved_dtype"] == "float32"
    assert man["arrays"]["f1_coeff"]["sample"] is not None and man["arrays"]["f1_sgr_xqd_v"]["sample"] is None
    for f in npy:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
