"""gfix (ff_schedule.hpp): the one quantiser of the generalized rare rows, floor(t 2^e) of a binary32 term, through
ff_debug_gfix -- the function the staging and pair_low_general_kernel both call."""
import ctypes

import numpy as np
import pytest

from frackyfrac_amd import _lib as L

# the plan's e puts the largest per-sample total into [2^60, 2^61): the smallest binary32 denormal alone, or 2^31 terms
# of the largest binary32 number
E_MAX, E_MIN = 60 + 149, 60 - 128 - 31


def gfix(t, e):
    t = np.ascontiguousarray(t, dtype=np.float32)
    out = np.zeros(len(t), dtype=np.uint64)
    fn = L.lib().ff_debug_gfix
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    fn.restype = None
    fn(t.ctypes.data, len(t), e, out.ctypes.data)
    return out


@pytest.mark.parametrize("e", [E_MIN, -3, 0, 37, E_MAX])
def test_gfix_is_monotone_and_exact_where_the_product_is_an_integer(e):
    rng = np.random.default_rng(e + 1000)
    top = 60 - e  # terms below 2^top stay below 2^60
    t = np.sort(np.ldexp(rng.uniform(0.5, 1.0, 4000), rng.integers(max(top - 70, -149), min(top, 127) + 1, 4000)).astype(np.float32))
    got = gfix(t, e)
    assert np.all(np.diff(got.astype(np.int64)) >= 0)
    want = [int(np.floor(np.ldexp(float(x), e))) if np.ldexp(float(x), e) < 2.0 ** 53 else None for x in t]
    assert all(w is None or int(g) == w for g, w in zip(got, want))
    assert gfix([0.0], e)[0] == 0
    for k in range(max(-e, -149), min(top, 127) + 1, 7):  # powers of two: exact
        assert int(gfix([np.ldexp(np.float32(1.0), k)], e)[0]) == 1 << (k + e)
    if e == E_MAX:
        assert int(gfix([np.float32(1e-45)], e)[0]) == 1 << 60  # the smallest denormal
