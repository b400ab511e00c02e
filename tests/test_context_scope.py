"""Context.scope(), Context.call(), Context.timed() and default_bd() against a recording stand-in for the library: no device, no libsvtav1_hip.so.
What is pinned: a scope frees exactly what was allocated through it, once, however the block ends; planes, structure arrays and empty arrays are uploaded
by the rules the public methods rely on; the timing loop's arithmetic."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_package


class FakeLib:
    """Records every call as (name, args...); svt_hip_malloc hands out distinct fake addresses."""

    def __init__(self):
        self.calls, self.next, self.free_status, self.fn_calls, self.t0 = [], 0x10000, 0, 0, 0

    def named(self, name):
        return [c for c in self.calls if c[0] == name]

    def svt_hip_malloc(self, h, ref, nbytes):
        ref._obj.value = self.next
        self.calls.append(("malloc", self.next, nbytes))
        self.next += (nbytes + 0xFFF) & ~0xFFF
        return 0

    def svt_hip_free(self, h, p):
        self.calls.append(("free", p.value))
        return self.free_status

    def svt_hip_memcpy_h2d(self, h, d, src, nbytes):
        self.calls.append(("h2d", d.value, src.value, nbytes))
        return 0

    def svt_hip_memcpy_d2h(self, h, dst, d, nbytes):
        self.calls.append(("d2h", d.value, nbytes))
        return 0

    def svt_hip_sync(self, h):
        self.calls.append(("sync",))
        return 0

    def svt_hip_last_error(self, h):
        return b"bad thing"

    def svt_hip_timer_start(self, h):
        self.t0 = self.fn_calls
        return 0

    def svt_hip_timer_stop_ms(self, h, ref):
        ref._obj.value = 0.5 * (self.fn_calls - self.t0)   # half a millisecond per call of the timed function
        self.calls.append(("window", self.fn_calls - self.t0))
        return 0

    def svt_hip_boom_dev(self, h, a, b):
        self.calls.append(("boom", a, b))
        return 7


@pytest.fixture
def pkg():
    return load_package()


@pytest.fixture
def ctx(pkg):
    c = pkg.Context.__new__(pkg.Context)   # no __init__: no library, no device
    c.L, c.h = FakeLib(), C.c_void_p(0)    # h = NULL: __del__ -> close() destroys nothing
    return c


def allocated(L):
    return [c[1] for c in L.named("malloc")]


def freed(L):
    return [c[1] for c in L.named("free")]


def five_allocations(pkg, s, after_third=None):
    s.plane(np.zeros((4, 8), np.uint8))
    s.structs((pkg.GmJob * 3)())
    s.filled(5, -7, np.int32)
    if after_third is not None:
        raise after_third
    s.empty(100)
    s.upload(np.arange(6, dtype=np.int16))


def test_normal_exit_frees_each_allocation_once(pkg, ctx):
    with ctx.scope() as s:
        five_allocations(pkg, s)
        assert freed(ctx.L) == []
    assert len(allocated(ctx.L)) == 5 and len(set(allocated(ctx.L))) == 5
    assert sorted(freed(ctx.L)) == sorted(allocated(ctx.L))


@pytest.mark.parametrize("free_status", [0, 2])
def test_exception_exit_frees_and_propagates(pkg, ctx, free_status):
    ctx.L.free_status = free_status   # a failing svt_hip_free must not mask the block's exception
    boom = KeyError("the block's own exception")
    with pytest.raises(KeyError) as info:
        with ctx.scope() as s:
            five_allocations(pkg, s, after_third=boom)
    assert info.value is boom
    assert len(allocated(ctx.L)) == 3
    assert sorted(freed(ctx.L)) == sorted(allocated(ctx.L))


def test_caller_owned_and_offset_pointers_are_not_freed(ctx):
    mine = C.c_void_p(0xABC000)
    with ctx.scope() as s:
        d = s.empty(64)
        inner = C.c_void_p(d.value + 16)
        assert s.download(mine, (2,), np.int32).shape == (2,) and s.download(inner, (2,), np.int32).shape == (2,)
    assert freed(ctx.L) == [d.value]
    assert [c[1] for c in ctx.L.named("d2h")] == [mine.value, inner.value]


def test_plane_of_an_offset_strided_view(ctx):
    a = np.arange(16 * 32, dtype=np.uint16).reshape(16, 32).copy()   # owns its data: the root of every view below
    v = a[3:11, 5:21]
    with ctx.scope() as s:
        rec = s.plane(v)
        assert ctx.L.named("malloc") == [("malloc", rec.d_root.value, a.nbytes)]
        assert ctx.L.named("h2d") == [("h2d", rec.d_root.value, a.ctypes.data, a.nbytes)]   # the whole root, once
        assert rec.ptr.value == rec.d_root.value + (3 * 32 + 5) * 2
        assert rec.stride == 32 and rec.root is a and rec.view is v
        back = s.plane_back(rec)
        assert back.shape == v.shape and back.strides == v.strides and back.base.shape == a.shape
        assert ctx.L.named("d2h") == [("d2h", rec.d_root.value, a.nbytes)]
        with pytest.raises(AssertionError):
            s.plane(a[:, ::2])
    assert freed(ctx.L) == [rec.d_root.value]


def test_zero_length_structs_and_empty_upload(pkg, ctx):
    with ctx.scope() as s:
        s.structs((pkg.GmJob * 0)())
        s.upload(np.zeros(0, np.int32))
        out = s.structs_back(C.c_void_p(0x5000), pkg.GmResult * 0)
        assert len(out) == 0 and isinstance(out, pkg.GmResult * 0)
        full = s.structs_back(C.c_void_p(0x5000), pkg.GmResult * 2)
    assert [c[2] for c in ctx.L.named("malloc")] == [4, 4]
    assert ctx.L.named("h2d") == []
    assert ctx.L.named("d2h") == [("d2h", 0x5000, C.sizeof(full))]
    assert len(freed(ctx.L)) == 2


def test_call_reports_as_check_does(ctx):
    for kwargs, what in (({}, "boom"), ({"what": "the big one"}, "the big one")):
        with pytest.raises(RuntimeError) as info:
            ctx.call("boom_dev", 1, 2, **kwargs)
        with pytest.raises(RuntimeError) as want:
            ctx.check(7, what)
        assert str(info.value) == str(want.value) == f"{what} failed: status 7: bad thing"
    assert ctx.L.named("boom") == [("boom", 1, 2)] * 2
    ctx.sync()
    assert ctx.L.calls[-1] == ("sync",)


def test_timed_windows(ctx):
    window_ms, ms_per_call = 100.0, 0.5

    def fn():
        ctx.L.fn_calls += 1

    want, reps = [], 2   # the windows the growth rule asks for, from the rule itself
    while True:
        want.append(reps)
        ms = ms_per_call * reps
        if ms >= window_ms:
            break
        reps = int(reps * max(2.0, 1.2 * window_ms / max(ms, 1e-3)))
    assert len(want) > 1 and ms_per_call * want[-2] < window_ms <= ms_per_call * want[-1]
    t, window, got_reps = ctx.timed(fn, window_ms)
    assert [c[1] for c in ctx.L.named("window")] == want
    assert (t, window, got_reps) == (ms_per_call * want[-1] / want[-1], ms_per_call * want[-1], want[-1])
    assert ctx.L.fn_calls == 2 + sum(want)
    assert ctx.L.calls.index(("sync",)) < ctx.L.calls.index(("window", want[0]))   # warm calls are synchronised before the first window


def test_default_bd(pkg):
    assert pkg.default_bd(1) == 8 and pkg.default_bd(2) == 10
    assert pkg.default_bd(2, 8) == 8 and pkg.default_bd(1, 8) == 8 and pkg.default_bd(2, 12) == 12 and pkg.default_bd(2, None) == 10
