"""Generalized UniFrac d(alpha): the option's interface and its validation.  Everything here ends before the device
is touched (FF_ERR_ARG, never FF_ERR_DEVICE), so it runs without a GPU."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L
from frackyfrac_amd.api import _opts


def tiny(neg_length=False):  # two samples on a three-node tree
    return ff.FlatNodes([0, 2, 3], [1, 2, 1], [0.5, 0.5, 1.0], [0.0, -1.0 if neg_length else 1.0, 2.0])


@pytest.mark.parametrize("kwargs, neg_length, word", [
    (dict(weighted=True, alpha=-0.1), False, "bad alpha"),
    (dict(weighted=True, alpha=1.5), False, "bad alpha"),
    (dict(weighted=True, alpha=math.nan), False, "bad alpha"),
    (dict(weighted=False, alpha=0.5), False, "weighted"),
    (dict(weighted=True, alpha=0.5, unsorted_walk=True), False, "unsorted"),
    (dict(weighted=True, alpha=0.5), True, "branch length 1"),
])
def test_bad_alpha_requests_are_argument_errors(kwargs, neg_length, word):
    nodes = tiny(neg_length)
    for call in (lambda: ff.unifrac_dists(nodes, **kwargs), lambda: ff.Plan(nodes, **kwargs)):
        with pytest.raises(ff.FFError) as e:
            call()
        assert e.value.code == L.FF_ERR_ARG and word in str(e.value), str(e.value)


def test_alpha_helpers_round_trip_and_defaults_stay_clear():
    lib = L.lib()
    o = _opts(True)
    assert o.flags == 0 and list(o.reserved) == [0, 0] and math.isnan(lib.ff_options_alpha(ctypes.byref(o)))
    for alpha in (0.0, 0.5, 1.0):
        o = _opts(True, alpha=alpha)
        assert o.flags == L.FLAG_GENERALIZED and lib.ff_options_alpha(ctypes.byref(o)) == alpha
        bits = int(np.float64(alpha).view(np.uint64))  # low word first
        assert [r & 0xFFFFFFFF for r in o.reserved] == [bits & 0xFFFFFFFF, bits >> 32]


@pytest.mark.parametrize("args, message", [
    (["-g", "0.5"], "ERROR: -g can only be used with weighted unifrac\n"),
    (["-w", "-g", "abc"], 'invalid value "abc" for flag -g: parse error\n'),
    (["-w", "-g", "1.5"], "ERROR: bad alpha: 1.5\n"),
])
def test_cli_messages(args, message):
    r = subprocess.run([L.FRCFRC_PATH, "-t", "no-such.tree", *args], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith(message), r.stderr
