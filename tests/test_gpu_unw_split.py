"""Unweighted FIXED32 with the rows few samples reach reduced apart (pair_low_unw_kernel: k_r added to every pair of
samples that both have rare row r; U = W_i + W_j - 2 (common over the matrix rows + that)): the same integers as with
every row on the matrix cores.  FF_UNW_SPLIT=1 forces the split, 0 forbids it.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-6  # FIXED32's stated guarantee (include/frackyfrac_amd.h)


def rel_err(got, want):
    m = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    denom = np.where(want[m] == 0, 1.0, np.abs(want[m]))
    return float(np.max(np.abs(got[m] - want[m]) / denom)) if m.any() else 0.0


def problem(ns, nl, dens):
    tree, ptr, idx, val = synth.make(ns, nl, dens, 17 + ns)
    nodes = ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), ptr, idx, val)
    ft = O.FlatTree(tree.names, tree.branch_len, tree.size, tree.parent)
    ip, on = O.flatten_samples(ft, ptr, idx, val, 0)
    return nodes, ip, on, ft


def run(plan):
    import torch
    out = torch.empty(plan.n_slots, dtype=torch.float64, device="cuda")
    plan.run(out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# 333: the smallest sample count at which the split is considered (2 x LOW_TILE_MAX up) that no block side divides --
# diagonal and off-diagonal blocks, a ragged last one; the other two take the lists from long to nearly empty
@pytest.mark.parametrize("ns,nl,dens", [(333, 500, 0.05), (700, 9000, 0.003), (2100, 3000, 0.01)])
def test_unweighted_split_gives_the_same_integers(monkeypatch, ns, nl, dens):
    nodes, ip, on, ft = problem(ns, nl, dens)
    outs, rare = {}, {}
    monkeypatch.setenv("FF_REFINE", "0")  # compare the raw integers
    for flag in ("0", "1", "128", "112", "96", "80", "64"):  # (the last five: the split with that block side forced)
        monkeypatch.setenv("FF_UNW_SPLIT", "0" if flag == "0" else "1")
        if len(flag) > 1:
            monkeypatch.setenv("FF_LOW_TILE", flag)
        plan = ff.Plan(nodes, False, precision="fixed32")
        rare[flag] = int(plan.info.rare_rows)
        outs[flag] = run(plan)
        if flag == "1":  # re-targeted at shards: the rare rows' tiles and sums follow the shard
            parts = []
            for r in range(3):
                plan.set_shard(r, 3)
                parts.append(run(plan))
            assert np.array_equal(np.concatenate(parts), outs["1"])
        plan.close()
    monkeypatch.delenv("FF_LOW_TILE")
    assert rare["0"] == 0
    for flag in ("1", "128", "112", "96", "80", "64"):
        assert 0 < rare[flag] < nodes.n_branches, flag
        assert np.array_equal(outs[flag], outs["0"]), flag
    monkeypatch.delenv("FF_REFINE")
    monkeypatch.setenv("FF_UNW_SPLIT", "1")
    want = O.unifrac_dists(ip, on, ft.dist, False)
    assert np.array_equal(ff.unifrac_dists(nodes, False, precision="fixed32"), want)  # (dyadic lengths: bit-exact)


def test_unweighted_split_with_lengths_off_the_grid(monkeypatch):
    """Log-normal lengths (bench.with_lognormal_lengths): a rare branch's integer length passes two base-128 digits
    and rides whole in the LDS add, the matrix rows are graded."""
    nodes, ip, on, ft = problem(700, 9000, 0.003)
    bl = np.random.default_rng(7).lognormal(-3.0, 1.5, nodes.n_branches)
    bl[nodes.branch_len == 0.0] = 0.0
    nodes = ff.FlatNodes(nodes.indptr, nodes.branch_id, nodes.abnd, bl)
    outs = {}
    monkeypatch.setenv("FF_REFINE", "0")
    for flag in ("0", "1"):
        monkeypatch.setenv("FF_UNW_SPLIT", flag)
        plan = ff.Plan(nodes, False, precision="fixed32")
        assert (int(plan.info.rare_rows) > 0) == (flag == "1")
        assert not plan.info.lengths_exact
        outs[flag] = run(plan)
        plan.close()
    assert np.array_equal(outs["1"], outs["0"])
    monkeypatch.delenv("FF_REFINE")
    got = ff.unifrac_dists(nodes, False, precision="fixed32")
    err = rel_err(got, O.unifrac_dists(ip, on, bl, False))
    print("split, refined, against the oracle: worst relative error %.3e" % err)
    assert err <= RTOL
