"""Variance-adjusted weighted UniFrac: what the option refuses.  Everything here ends before the device is touched
(FF_ERR_ARG, never FF_ERR_DEVICE), so it runs without a GPU."""
import math
import subprocess

import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L


def tiny(length=1.0, count=4.0):  # three samples on a three-node tree, undivided abundances
    return ff.FlatNodes([0, 2, 3, 5], [1, 2, 1, 1, 2], [count, 2.0, 7.0, 1.0, 1.0], [0.0, length, 2.0])


@pytest.mark.parametrize("kwargs, nodes, word", [
    (dict(weighted=False), tiny(), "weighted"),
    (dict(weighted=True, alpha=0.5), tiny(), "alpha"),
    (dict(weighted=True, unsorted_walk=True), tiny(), "unsorted"),
    (dict(weighted=True, precision="fixed32"), tiny(), "precision"),
    (dict(weighted=True, precision="exact64"), tiny(), "precision"),
    (dict(weighted=True), tiny(length=-1.0), "branch length 1"),
    (dict(weighted=True), tiny(length=math.inf), "branch length 1"),
    (dict(weighted=True), tiny(length=math.nan), "branch length 1"),
    (dict(weighted=True), tiny(count=-4.0), "abundance"),
    (dict(weighted=True), tiny(count=math.inf), "abundance"),
])
def test_bad_requests_are_argument_errors(kwargs, nodes, word):
    with pytest.raises(ff.FFError) as e:
        ff.unifrac_dists(nodes, variance_adjusted=True, **kwargs)
    assert e.value.code == L.FF_ERR_ARG and word in str(e.value), str(e.value)


def test_reference_l_is_refused_where_the_lists_are_flattened():
    tree = ff.parse_newick("((a:1,b:2):1,c:3);")
    with pytest.raises(ff.FFError) as e:
        ff.Plan.from_leaves(tree, [0, 1, 2, 3], [0, 1, 2], [4.0, 7.0, 1.0], True, leave_unnormalized="reference",
                            variance_adjusted=True)
    assert e.value.code == L.FF_ERR_ARG and "unsorted" in str(e.value), str(e.value)


def test_cli_messages():
    r = subprocess.run([L.FRCFRC_PATH, "-t", "no-such.tree", "-vaw"], capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("ERROR: -vaw can only be used with weighted unifrac\n"), r.stderr
