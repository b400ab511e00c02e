"""The three sample formats of the library -- (uint8, bd 8), (uint16, bd 10) and (uint16, bd 8): 8-bit samples in 16-bit planes, what the encoder's
`-16bit-pipeline 1` hands every stage after mode decision -- as test parameters.

A test that took `bd` and derived the sample type from it takes `bd, fmt` from bd_fmts(): fmt is None for the two formats it always ran (ids "8", "10", ...
unchanged) and np.uint16 for the added one (id "u16-8").  The (u16, 8) case has two witnesses: the oracle at (2, 8), and the (1, 8) result on the same
samples widened -- first between the two oracle results on the CPU, then between the two device results."""
import numpy as np
import pytest

U16_8 = pytest.param(8, np.uint16, id="u16-8")


def bd_fmts(*bds):
    return [pytest.param(bd, None, id=str(bd)) for bd in (bds or (8, 10))] + [U16_8]


def dtype_of(bd, fmt=None):
    return fmt if fmt is not None else (np.uint8 if bd == 8 else np.uint16)


def check_8bit_range(*arrays):
    """the expected result of a (u16, 8) case: nothing above 255 -- a clip at 1023 would show -- and both ends of the range present, so the clamps were engaged"""
    mx = max(int(np.max(a)) for a in arrays); mn = min(int(np.min(a)) for a in arrays)
    assert mx == 255 and mn == 0, (mn, mx)


def same_results(wide, narrow, what=""):
    """results of a (u16, 8) run against those of the (u8, 8) run: sample planes (uint16 against uint8) widened, everything else -- sums, errors, taps, vectors -- unchanged"""
    assert len(wide) == len(narrow), what
    for i, (a, b) in enumerate(zip(wide, narrow)):
        a, b = np.asarray(a), np.asarray(b)
        if b.dtype == np.uint8 and a.dtype == np.uint16: b = b.astype(np.uint16)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, i, np.argwhere(a != b)[:4] if a.shape == b.shape else (a.shape, b.shape))


_inputs_seen = [False]


def note_inputs(*planes):
    """the sample planes a (u16, 8) case (or its uint8 companion) is fed: inside 0 .. 255 with both ends present.  Called by the content generators of the cases whose
    results are numbers -- sums, errors, taps, levels -- and not samples; two_witnesses() insists that one of the two range checks has been made."""
    check_8bit_range(*planes)
    _inputs_seen[0] = True


def _as_list(r):
    return [r] if isinstance(r, np.ndarray) else list(r)


def two_witnesses(case, fmt, bd, *args):
    """The one driver of the three formats.  case(*args, bd, dt, wide) -> (device results, oracle results), two arrays or two lists of arrays that `case` has already
    asserted equal: the first witness.  wide asks for the content and the sizes of the added format -- all-max, all-0 and 0 / max checkerboard or binary regions, the
    smallest ragged size.  For 8-bit samples in 16-bit planes the expected sample planes must stay inside 0 .. 255 and reach both ends (where the results hold no
    samples, the input planes, through note_inputs()), and the second witness is the (u8, 8) run of the same case: the two oracle results agree (the widening
    property, on the CPU), then the two device results."""
    _inputs_seen[0] = False
    got, exp = map(_as_list, case(*args, bd, dtype_of(bd, fmt), fmt is not None))
    if fmt is None: return
    planes = [e for e in exp if np.asarray(e).dtype == np.uint16 and np.asarray(e).ndim == 2]
    if planes: check_8bit_range(*planes)
    assert planes or _inputs_seen[0], "a (u16, 8) case must assert the 0 .. 255 range of its expected samples or of its inputs"
    got8, exp8 = map(_as_list, case(*args, 8, np.uint8, True))
    same_results(exp, exp8, "oracle (2, 8) vs (1, 8)")
    same_results(got, got8, "device (2, 8) vs (1, 8)")
