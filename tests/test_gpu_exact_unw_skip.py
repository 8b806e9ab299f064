"""pair_exact_unw_skip_kernel: the row-skipping form of the exact unweighted reduction against the oracle,
bit for bit, and against the dense form of the same problem.  Forced by FF_XU_SKIP=1, with tiles of one and of two
column groups.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import synth
from oracle import oracle as O
from test_gpu_exact_unw import EXACT64, HOST_THREADS, K_EXACT_UNW, problem, same_bits

pytestmark = pytest.mark.gpu


def clustered(ns, lengths="lognormal", nl=2000, per_sample=12, seed=21):
    """Sample s draws its leaves from the (s // 40)-th of ceil(ns / 40) contiguous ranges of the leaf order: whole
    (tile, slab) cells are empty, others hold one branch, and 40 divides neither 8 nor 64 (groups straddle clusters)."""
    tree = synth.yule_tree(nl, seed)
    rng = np.random.default_rng(seed)
    nc = -(-ns // 40)
    rows = [np.sort(rng.choice(np.arange(c * nl // nc, (c + 1) * nl // nc), per_sample, replace=False)) for c in np.arange(ns) // 40]
    ptr, idx, val = np.arange(ns + 1, dtype=np.int64) * per_sample, tree.leaf_ids[np.concatenate(rows)], np.ones(ns * per_sample)
    bl = rng.lognormal(-3.0, 1.5, tree.n)
    bl[0] = 0.0
    # a branch inside cluster 1, and the root's child with the smaller subtree (some pairs have neither)
    inside, near_root = int(tree.parent[tree.leaf_ids[nl // nc + 7]]), 1 if tree.size[1] * 2 < tree.n else 1 + int(tree.size[1])
    special = {"inf": np.inf, "nan": np.nan, "negative": -0.37, "minus_zero": -0.0, "tiny": 5e-324}
    if lengths != "lognormal":
        bl[[inside, near_root]] = special[lengths]
    n0 = ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), ptr, idx, val)
    ft = O.FlatTree(tree.names, bl, tree.size, tree.parent)
    ip, on = O.flatten_samples(ft, ptr, idx, val, 0)
    return ff.FlatNodes(n0.indptr, n0.branch_id, n0.abnd, bl), O.unifrac_dists(ip, on, bl, False, nthreads=HOST_THREADS)


def check(monkeypatch, nodes, want, world=1, may_visit_nothing=False):
    """Both tile widths: the skipping form's plan says what it is, and its bits are the oracle's and the dense form's."""
    for jmax in ("1", "2"):
        monkeypatch.setenv("FF_XU_JMAX", jmax)
        monkeypatch.setenv("FF_XU_SKIP", "0")
        dense = ff.Plan(nodes, False, precision="auto")
        assert dense.info.active_fraction == 1.0
        want_dense = dense.run_host()
        dense.close()
        monkeypatch.setenv("FF_XU_SKIP", "1")
        plan = ff.Plan(nodes, False, precision="auto")
        parts = []
        for r in range(world):
            if world > 1:
                plan.set_shard(r, world)
            info = plan.info
            print("jmax %s shard %d/%d: active_fraction %.4f" % (jmax, r, world, info.active_fraction))
            assert (info.kernel, info.precision) == (K_EXACT_UNW, EXACT64)
            assert (0.0 <= info.active_fraction < 1.0) if may_visit_nothing else (0.0 < info.active_fraction < 1.0)
            parts.append(plan.run_host())
        plan.close()
        got = np.concatenate(parts)
        assert same_bits(got, want), jmax
        assert np.array_equal(got.view(np.uint64), want_dense.view(np.uint64)), jmax


@pytest.mark.parametrize("ns,lengths", [(333, "lognormal"), (130, "lognormal"), (130, "inf"), (130, "nan"), (130, "negative"),
                                        (130, "minus_zero"), (130, "tiny")])
def test_clustered_table_and_lengths_no_arithmetic_may_touch(monkeypatch, ns, lengths):
    """Empty (tile, slab) cells, cells of a single branch, ragged last groups (333); lengths that only masking leaves
    intact, one inside a cluster and one next to the root."""
    nodes, want = clustered(ns, lengths)
    if lengths in ("inf", "nan"):
        assert np.isnan(want).any() and not np.isnan(want).all()
    check(monkeypatch, nodes, want)


@pytest.mark.parametrize("world", [1, 3])
def test_uniform_sparse_table_one_shard_and_retargeted(monkeypatch, world):
    """Nearly every slab visited, most of its rows skipped; the plan re-targeted shard by shard gives the same."""
    nodes, ip, on, ft = problem(700, 9000, 0.003, 5)
    check(monkeypatch, nodes, O.unifrac_dists(ip, on, ft.dist, False, nthreads=HOST_THREADS), world=world)


def test_empty_samples(monkeypatch):
    """The shapes DESIGN 4.5 records a fault next to: no presence bit at all (every distance 0 / 0), then every other
    sample empty; a sample count the tile height does not divide."""
    n = 2055
    tree, ptr, idx, val = synth.make(n, 400, 0.1, 5)
    T = ff.parse_newick(tree.newick())
    ft = O.FlatTree(tree.names, tree.branch_len, tree.size, tree.parent)
    keep = np.arange(n) % 2 == 0
    for cnt in (np.zeros(n, dtype=np.int64), np.where(keep, np.diff(ptr), 0)):
        p2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        sel = np.flatnonzero(np.repeat(cnt > 0, np.diff(ptr)))
        ip, on = O.flatten_samples(ft, p2, idx[sel], val[sel], 0)
        want = O.unifrac_dists(ip, on, ft.dist, False, nthreads=HOST_THREADS)
        assert np.isnan(want).all() == (cnt.sum() == 0)
        check(monkeypatch, ff.flatten_leaf_csr(T, p2, idx[sel], val[sel]), want, may_visit_nothing=cnt.sum() == 0)


def test_the_estimate_declines_on_a_dense_table(monkeypatch):
    """Switch unset, one sample in ten has a leaf: nearly every (tile, row) cell is touched and the dense form stays."""
    monkeypatch.delenv("FF_XU_SKIP", raising=False)
    nodes, ip, on, ft = problem(513, 1000, 0.1, 613)
    plan = ff.Plan(nodes, False, precision="auto")
    assert plan.info.kernel == K_EXACT_UNW and plan.info.active_fraction == 1.0
    assert same_bits(plan.run_host(), O.unifrac_dists(ip, on, ft.dist, False, nthreads=HOST_THREADS))
    plan.close()
