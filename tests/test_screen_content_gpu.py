"""GPU: svt_hip_screen_content_detect_dev against is_screen_content restated around the reference's own functions (tests/palette_common.py: ref_screen_content) on
the pictures tests/test_palette_ref_cpu.py proves to be what they are named after: counts one below, on and one above either threshold, blocks of exactly 4 and 5
colours, two-colour blocks of rounded variance 0 and 1, sizes that are no multiple of 16 from 16x16 (and one with no whole block) to 512x288, embedded views; at 8
and at 10 bits, the four outputs and the words behind them."""
import numpy as np
import pytest

import palette_common as P
import test_palette_abi as abi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,bd", [(np.uint8, 8), (np.uint16, 10)], ids=["u8", "u16_bd10"])
def test_pictures(hip, ref, dtype, bd):
    pics = P.sc_pictures(dtype, bd)
    assert any(p.strides[0] > p.shape[1] * p.itemsize for _, p, _ in pics) and any(p.shape[0] % 16 and p.shape[1] % 16 for _, p, _ in pics)
    for name, pic, known in pics:
        want = P.ref_screen_content(ref, pic, bd)
        assert known is None or want == known, name
        before = np.array([0x7EADBEEF, -5, 123456, 99, 0x1234567, -77, 31, 64], np.int32)   # the call owns the first four words alone
        got = hip.screen_content_detect(pic, bd=bd, out=before)
        assert got[:4].tolist() == want, (name, got[:4].tolist(), want)
        assert (got[4:] == before[4:]).all(), name


def test_refusals_with_a_live_context(hip, pkg):
    L = hip.L
    d = hip.to_device(np.zeros(1 << 16, np.uint8))
    try:
        assert abi.call_detect(L, hip.h, d.value) == 0
        hip.check(L.svt_hip_sync(hip.h), "sync")
        for c in abi.DETECT_BAD:
            assert abi.call_detect(L, hip.h, d.value, **c) == abi.BAD_ARG, c
            assert L.svt_hip_last_error(hip.h).decode().startswith("svt_hip_screen_content_detect_dev: bad argument"), c
        hip.check(L.svt_hip_sync(hip.h), "sync")
    finally:
        hip.free(d)
