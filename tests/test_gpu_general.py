"""pair_general_kernel: generalized UniFrac d(alpha) against a dense binary64 restatement of its definition.
Needs an MI355X: `pytest -m gpu`."""
import functools
import os
import subprocess
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L
from frackyfrac_amd import api
from test_gpu_exact_unw import HOST_THREADS, problem as lognormal_problem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_GENERAL, FLOAT32 = 8, 3
TWIN, EMPTY = (5, 4), (7, 9)
TOL = 1e-6  # absolute


slot = lambda i, j: i * (i - 1) // 2 + j  # noqa: E731


@functools.lru_cache(maxsize=None)  # (by table object: computed once per table and alpha, shared, never written to)
def reference(nodes, alpha):
    """d(alpha) from a dense binary64 X[sample, branch], row by row of the triangle, in iter_pairs order."""
    X = np.zeros((nodes.n_samples, nodes.n_branches))
    for s in range(nodes.n_samples):
        e = slice(nodes.indptr[s], nodes.indptr[s + 1])
        X[s, nodes.branch_id[e]] = nodes.abnd[e]

    def row(i):
        s, d = X[i] + X[:i], np.abs(X[i] - X[:i])
        has = s > 0
        w = np.where(has, nodes.branch_len * s ** alpha, 0.0)
        q = np.divide(d, s, out=np.zeros_like(s), where=has)
        with np.errstate(invalid="ignore"):
            return np.einsum("pb,pb->p", w, q) / w.sum(1)

    with ThreadPool(HOST_THREADS) as pool:  # (the rows are independent; numpy releases the interpreter lock)
        return np.concatenate(pool.map(row, range(1, nodes.n_samples)))


@functools.lru_cache(maxsize=None)
def table(ns):
    """synth.make(ns, 2000, 0.1) on log-normal lengths; sample 5 a copy of sample 4, samples 7 and 9 empty."""
    nodes = lognormal_problem(ns, 2000, 0.1, 11)[0]
    cut = lambda a, s: a[nodes.indptr[s]:nodes.indptr[s + 1]]
    src = [TWIN[1] if s == TWIN[0] else s for s in range(ns)]
    ids = [cut(nodes.branch_id, s)[:0 if t in EMPTY else None] for t, s in enumerate(src)]
    ab = [cut(nodes.abnd, s)[:0 if t in EMPTY else None] for t, s in enumerate(src)]
    return ff.FlatNodes(np.cumsum([0] + [len(x) for x in ids]), np.concatenate(ids), np.concatenate(ab), nodes.branch_len)


def run_with_height(nodes, h, **kwargs):
    L.lib().ff_tune(b"FF_X_TILE_H", str(h).encode())
    try:
        plan = ff.Plan(nodes, True, **kwargs)
    finally:
        L.lib().ff_tune(b"FF_X_TILE_H", None)
    assert plan.info.kernel == K_GENERAL and plan.info.precision == FLOAT32
    got = plan.run_host()
    assert plan.refined_pairs()[0] == 0 and plan.audit()[:2] == (0, 0)
    plan.check_precision()
    plan.close()
    return got


@pytest.mark.parametrize("alpha", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("ns", [130, 333])
def test_against_the_definition_at_both_tile_heights(ns, alpha):
    nodes = table(ns)
    ref = reference(nodes, alpha)
    got8, got16 = (run_with_height(nodes, h, alpha=alpha) for h in (8, 16))
    assert np.array_equal(got8, got16, equal_nan=True)
    nan = np.zeros(len(ref), dtype=bool)
    nan[slot(max(EMPTY), min(EMPTY))] = True
    assert np.array_equal(np.isnan(ref), nan) and np.array_equal(np.isnan(got8), nan)
    worst = np.max(np.abs(got8 - ref)[~nan])
    print("ns %d alpha %g: worst |got - ref| = %.3g" % (ns, alpha, worst))
    assert worst <= TOL
    assert got8[slot(*TWIN)] == 0.0
    for e in EMPTY:
        for o in set(range(ns)) - set(EMPTY):
            assert got8[slot(max(e, o), min(e, o))] == 1.0


@pytest.mark.parametrize("precision", ["auto", "fixed32"])
def test_alpha_one_is_the_weighted_plan(precision):
    nodes = table(333)
    a, b = ff.Plan(nodes, True, precision=precision, alpha=1.0), ff.Plan(nodes, True, precision=precision)
    assert (a.info.kernel, a.info.precision) == (b.info.kernel, b.info.precision) and a.info.kernel != K_GENERAL
    assert np.array_equal(a.run_host(), b.run_host(), equal_nan=True)


def test_shards_of_one_plan_give_the_whole_plans_bits():
    nodes = table(333)
    whole = ff.Plan(nodes, True, alpha=0.5).run_host()
    plan, parts = ff.Plan(nodes, True, alpha=0.5, rank=0, world=3), []
    for rank in range(3):
        plan.set_shard(rank, 3)
        parts.append(plan.run_host())
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)


def test_cli_and_streams_on_the_golden_table():
    sparse, tree = os.path.join(GOLDEN, "wtd.sparse"), os.path.join(GOLDEN, "wtd.tree")
    nodes = ff.flatten(ff.parse_sparse_abundance(open(sparse).read()), ff.Tree.read_file(tree))
    ref = reference(nodes, 0.5)
    r = subprocess.run([L.FRCFRC_PATH, "-w", "-s", "-g", "0.5", "-i", sparse, "-t", tree], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert np.max(np.abs(np.array([float(x) for x in r.stdout.split()]) - ref)) <= TOL
    text = []
    api.unifrac_text_stream(nodes, True, text.append, alpha=0.5)
    assert b"".join(text) == r.stdout
    whole = ff.unifrac_dists(nodes, True, alpha=0.5)
    pieces = [d for _, d in api.unifrac_dists_stream(nodes, True, alpha=0.5, max_pairs_per_chunk=7)]
    assert np.array_equal(np.concatenate(pieces), whole)
