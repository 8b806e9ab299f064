"""pair_vaw_kernel: variance-adjusted weighted UniFrac against a dense binary64 restatement of its definition
(include/frackyfrac_amd.h, FF_FLAG_VARIANCE_ADJUSTED).  Needs an MI355X: `pytest -m gpu`."""
import functools
import os
import subprocess
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L
from frackyfrac_amd import api, synth
from test_gpu_general import HOST_THREADS, slot

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_VAW, FLOAT32 = 9, 3
TWIN, EMPTY, SAME_LEAF, OTHER_LEAF = (5, 4), (7, 9), (11, 13), 15
TOL = 1e-6  # absolute


@functools.lru_cache(maxsize=None)  # (by table object: computed once per table, shared, never written to)
def reference(nodes):
    """d_VAW from dense binary64 X[sample, branch] and T - X, row by row of the triangle, in iter_pairs order."""
    X = np.zeros((nodes.n_samples, nodes.n_branches))
    for s in range(nodes.n_samples):
        e = slice(nodes.indptr[s], nodes.indptr[s + 1])
        X[s, nodes.branch_id[e]] = nodes.abnd[e]
    T = X.max(1, initial=0.0)
    C = T[:, None] - X
    P = np.divide(X, T[:, None], out=np.zeros_like(X), where=T[:, None] > 0)

    def row(i):
        mr = (X[i] + X[:i]) * (C[i] + C[:i])
        w = np.divide(nodes.branch_len, np.sqrt(mr), out=np.zeros_like(mr), where=mr > 0)
        with np.errstate(invalid="ignore"):
            return (w * np.abs(P[i] - P[:i])).sum(1) / (w * (P[i] + P[:i])).sum(1)

    with ThreadPool(HOST_THREADS) as pool:  # (the rows are independent; numpy releases the interpreter lock)
        return np.concatenate(pool.map(row, range(1, nodes.n_samples)))


@functools.lru_cache(maxsize=None)
def table(ns):
    """synth.make(ns, 2000, 0.1) as INTEGER leaf counts on log-normal lengths, flattened undivided; sample 5 a copy of
    sample 4, samples 7 and 9 empty, 11 and 13 wholly under one leaf (3 and 8 counts), 15 wholly under another."""
    tree, ptr, idx, val = synth.make(ns, 2000, 0.1, 11)
    bl = np.random.default_rng(12).lognormal(-3.0, 1.5, len(tree.branch_len))
    bl[0] = 0.0
    tree.branch_len = bl
    cut = lambda a, s: a[ptr[s]:ptr[s + 1]]  # noqa: E731
    leaves, counts = [cut(idx, s) for s in range(ns)], [np.ceil(1e4 * cut(val, s)) for s in range(ns)]
    leaves[TWIN[0]], counts[TWIN[0]] = leaves[TWIN[1]], counts[TWIN[1]]
    for s in EMPTY:
        leaves[s], counts[s] = leaves[s][:0], counts[s][:0]
    for s, leaf, n in ((SAME_LEAF[0], idx[0], 3.0), (SAME_LEAF[1], idx[0], 8.0), (OTHER_LEAF, idx[ptr[1] - 1], 5.0)):
        leaves[s], counts[s] = np.array([leaf]), np.array([n])
    assert idx[0] != idx[ptr[1] - 1]
    return ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), np.cumsum([0] + [len(x) for x in leaves]),
                               np.concatenate(leaves), np.concatenate(counts), leave_unnormalized=True)


def planted_nan(ns):
    """No term survives: empty / empty, both under the same single leaf, empty against a sample under a single leaf."""
    nan = np.zeros(ff.num_pairs(ns), dtype=bool)
    single = SAME_LEAF + (OTHER_LEAF,)
    for i, j in [EMPTY, SAME_LEAF] + [(e, s) for e in EMPTY for s in single]:
        nan[slot(max(i, j), min(i, j))] = True
    return nan


def run_with_height(nodes, h):
    L.lib().ff_tune(b"FF_X_TILE_H", str(h).encode())
    try:
        plan = ff.Plan(nodes, True, variance_adjusted=True)
    finally:
        L.lib().ff_tune(b"FF_X_TILE_H", None)
    assert plan.info.kernel == K_VAW and plan.info.precision == FLOAT32
    got = plan.run_host()
    assert plan.refined_pairs()[0] == 0 and plan.audit()[:2] == (0, 0)
    plan.close()
    return got


@pytest.mark.parametrize("ns", [130, 333])
def test_against_the_definition_at_both_tile_heights(ns):
    nodes = table(ns)
    ref = reference(nodes)
    got8, got16 = (run_with_height(nodes, h) for h in (8, 16))
    assert np.array_equal(got8, got16, equal_nan=True)
    nan = planted_nan(ns)
    assert np.array_equal(np.isnan(ref), nan) and np.array_equal(np.isnan(got8), nan)
    worst = np.max(np.abs(got8 - ref)[~nan])
    print("ns %d: worst |got - ref| = %.3g" % (ns, worst))
    assert worst <= TOL
    assert got8[slot(*TWIN)] == 0.0
    for e in EMPTY:
        for o in set(range(ns)) - set(EMPTY) - set(SAME_LEAF) - {OTHER_LEAF}:
            assert got8[slot(max(e, o), min(e, o))] == 1.0


def test_shards_of_one_plan_give_the_whole_plans_bits():
    nodes = table(333)
    whole = ff.Plan(nodes, True, variance_adjusted=True).run_host()
    plan, parts = ff.Plan(nodes, True, variance_adjusted=True, rank=0, world=3), []
    for rank in range(3):
        plan.set_shard(rank, 3)
        parts.append(plan.run_host())
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)


def test_cli_and_streams_on_the_golden_table():
    sparse, tree = os.path.join(GOLDEN, "wtd.sparse"), os.path.join(GOLDEN, "wtd.tree")
    nodes = ff.flatten(ff.parse_sparse_abundance(open(sparse).read()), ff.Tree.read_file(tree), leave_unnormalized=True)
    ref = reference(nodes)
    r = subprocess.run([L.FRCFRC_PATH, "-w", "-s", "-vaw", "-i", sparse, "-t", tree], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert np.max(np.abs(np.array([float(x) for x in r.stdout.split()]) - ref)) <= TOL
    text = []
    api.unifrac_text_stream(nodes, True, text.append, variance_adjusted=True)
    assert b"".join(text) == r.stdout
    whole = ff.unifrac_dists(nodes, True, variance_adjusted=True)
    pieces = [d for _, d in api.unifrac_dists_stream(nodes, True, variance_adjusted=True, max_pairs_per_chunk=7)]
    assert np.array_equal(np.concatenate(pieces), whole)
