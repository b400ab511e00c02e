"""CPU: how a mixed-size transform call is cut into launches (svt-av1_amd/csrc/txfm_plan.h), built for the host (tests/txfm_plan_host.cpp) and held against the
rules written out here: every job with blocks appears exactly once, in a launch of its own size class; at most 16 jobs per launch; the caller's order is kept within
a class; first_wg are the prefix sums of ceil(nblk / teams).  The partition itself is read from the program (it is chosen by measurement, docs/kernels/transforms.md);
what is held here is that it is a partition by max(W, H) and that the class of the 4- and 8-point sizes holds no 32- or 64-point size."""
import os
import subprocess

import pytest

from conftest import ROOT

TXW = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TXH = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
LONG = [max(w, h) for w, h in zip(TXW, TXH)]
TEAMS = [2 if (w, h) == (64, 64) else 256 // max(w, h) for w, h in zip(TXW, TXH)]
MAX_JOBS = 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("txfm_plan") / "txfm_plan_host"
    subprocess.check_call(["c++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "txfm_plan_host.cpp"), "-o", str(path)])
    return str(path)


@pytest.fixture(scope="module")
def classes(exe):
    """class of every size, as the header has it"""
    cls = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        _, ts, c, teams = line.split()
        cls[int(ts)] = int(c)
        assert int(teams) == TEAMS[int(ts)], line
    assert sorted(cls) == list(range(19))
    return cls


def plan(exe, jobs):
    out = []
    for line in subprocess.check_output([exe] + [f"{ts}:{n}" for ts, n in jobs], text=True).splitlines():
        f = line.split()
        assert f[0] == "launch" and f[3] == "jobs"
        cls, n = int(f[1]), int(f[2])
        assert f[4 + n] == "wg" and len(f) == 4 + n + 1 + n + 1, line
        out.append((cls, [int(v) for v in f[4:4 + n]], [int(v) for v in f[5 + n:]]))
    return out


def check(exe, classes, jobs):
    """the rules, for one job list -> the launches"""
    launches = plan(exe, jobs)
    seen = []
    for cls, idx, first_wg in launches:
        assert 1 <= len(idx) <= MAX_JOBS
        assert idx == sorted(idx)                                   # caller order inside a launch
        assert first_wg[0] == 0
        for k, j in enumerate(idx):
            ts, n = jobs[j]
            assert n > 0 and classes[ts] == cls, (j, ts, n, cls)
            assert first_wg[k + 1] - first_wg[k] == -(-n // TEAMS[ts]), (j, ts, n)
        seen += idx
    assert sorted(seen) == [j for j, (ts, n) in enumerate(jobs) if n > 0]   # exactly once, nothing without blocks
    for c in set(classes.values()):                                 # caller order across the launches of a class
        mine = [j for cls, idx, _ in launches if cls == c for j in idx]
        assert mine == sorted(mine), (c, mine)
    return launches


def test_partition_is_by_long_side(classes):
    order = sorted(range(19), key=lambda ts: LONG[ts])
    assert all(classes[a] <= classes[b] for a, b in zip(order, order[1:]))           # monotone in max(W, H) ...
    for a in range(19):
        for b in range(19):
            if LONG[a] == LONG[b]: assert classes[a] == classes[b]                     # ... and a function of it
    assert sorted(set(classes.values())) == list(range(len(set(classes.values()))))
    assert classes[0] == classes[1] == 0 and all(LONG[ts] <= 16 for ts in range(19) if classes[ts] == 0)   # the 4- and 8-point blocks drag no 32- or 64-point body along


def test_all_sizes(exe, classes):
    jobs = [(ts, 3 + 7 * ts) for ts in range(19)]
    launches = check(exe, classes, jobs)
    assert len(launches) == len(set(classes.values()))   # no class has more than 16 of the 19 sizes


def test_split_inside_a_class(exe, classes):
    jobs = [((0, 1, 5, 6)[k % 4], 65 + k) for k in range(18)]     # 18 jobs of 4- and 8-point sizes: 16 + 2
    launches = check(exe, classes, jobs)
    assert [(cls, idx) for cls, idx, _ in launches] == [(0, list(range(16))), (0, [16, 17])]
    assert launches[1][2] == [0, -(-81 // TEAMS[0]), -(-81 // TEAMS[0]) - (-82 // TEAMS[1])]   # the second launch counts its workgroups from 0 again


def test_absent_class(exe, classes):
    for absent in set(classes.values()):
        jobs = [(ts, 10) if classes[ts] != absent else (ts, 0) for ts in range(19)]
        launches = check(exe, classes, jobs)
        assert launches and all(cls != absent for cls, _, _ in launches)


def test_every_job_empty(exe, classes):
    assert check(exe, classes, [(ts, 0) for ts in range(19)]) == []
    assert check(exe, classes, [(0, 0), (4, -3)]) == []


def test_interleaved_classes(exe, classes):
    jobs = [(4, 3), (0, 65), (16, 9), (1, 33), (14, 17), (0, 1), (12, 5), (7, 0), (3, 9), (5, 40), (2, 16), (17, 4)]
    launches = check(exe, classes, jobs)
    for c in set(classes.values()):
        want = [j for j, (ts, n) in enumerate(jobs) if n > 0 and classes[ts] == c]
        got = [j for cls, idx, _ in launches if cls == c for j in idx]
        assert got == want
    # ragged last workgroups: 65 blocks of 4x4 are one full workgroup of 64 teams and one more; 3 blocks of 64x64 are two workgroups of two teams
    wg = {j: fw[k + 1] - fw[k] for _, idx, fw in launches for k, j in enumerate(idx)}
    assert wg[1] == 2 and wg[0] == 2 and wg[5] == 1
