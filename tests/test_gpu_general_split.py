"""pair_low_general_kernel: the rare rows of a generalized plan (FF_SPARSE_SPLIT=1) against the dense binary64
restatement of d(alpha).  Needs an MI355X: `pytest -m gpu`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L
from test_gpu_general import EMPTY, GOLDEN, K_GENERAL, TOL, TWIN, reference, slot
from test_gpu_general import lognormal_problem

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def table(ns, density, shrunk=None):
    """2,000 leaves on log-normal lengths; sample 5 a copy of sample 4, samples 7 and 9 empty (test_gpu_general.table);
    shrunk: that sample's abundances times 2^-40."""
    nodes = lognormal_problem(ns, 2000, density, 11)[0]
    cut = lambda a, s: a[nodes.indptr[s]:nodes.indptr[s + 1]]  # noqa: E731
    src = [TWIN[1] if s == TWIN[0] else s for s in range(ns)]
    ids = [cut(nodes.branch_id, s)[:0 if t in EMPTY else None] for t, s in enumerate(src)]
    ab = [cut(nodes.abnd, s)[:0 if t in EMPTY else None] * (2.0 ** -40 if t == shrunk else 1.0) for t, s in enumerate(src)]
    return ff.FlatNodes(np.cumsum([0] + [len(x) for x in ids]), np.concatenate(ids), np.concatenate(ab), nodes.branch_len)


def forced_plan(nodes, h=None, **kwargs):
    L.lib().ff_tune(b"FF_SPARSE_SPLIT", b"1")
    L.lib().ff_tune(b"FF_X_TILE_H", None if h is None else str(h).encode())
    try:
        return ff.Plan(nodes, True, **kwargs)
    finally:
        L.lib().ff_tune(b"FF_SPARSE_SPLIT", None)
        L.lib().ff_tune(b"FF_X_TILE_H", None)


def check_values(got, ref, ns):
    nan = np.zeros(len(ref), dtype=bool)
    nan[slot(max(EMPTY), min(EMPTY))] = True
    assert np.array_equal(np.isnan(ref), nan) and np.array_equal(np.isnan(got), nan)
    worst = np.max(np.abs(got - ref)[~nan])
    print("worst |got - ref| = %.3g" % worst)
    assert worst <= TOL
    assert got[slot(*TWIN)] == 0.0
    for e in EMPTY:
        for o in set(range(ns)) - set(EMPTY):
            assert got[slot(max(e, o), min(e, o))] == 1.0


@pytest.mark.parametrize("alpha", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("ns,density", [(130, 0.1), (333, 0.01)])
def test_against_the_definition_at_both_tile_heights(ns, density, alpha):
    nodes, got = table(ns, density), []
    for h in (8, 16):
        plan = forced_plan(nodes, h, alpha=alpha)
        info = plan.info
        assert 0 < info.rare_rows < info.n_rows and info.rare_updates > 0 and info.kernel == K_GENERAL
        got.append(plan.run_host())
        plan.close()
    assert np.array_equal(got[0], got[1], equal_nan=True)
    check_values(got[0], reference(nodes, alpha), ns)


def test_shards_of_one_forced_plan_give_the_whole_plans_bits():
    nodes = table(333, 0.01)
    whole = forced_plan(nodes, alpha=0.5).run_host()
    plan, parts = forced_plan(nodes, alpha=0.5, rank=0, world=3), []
    assert plan.info.rare_rows > 0
    for rank in range(3):
        plan.set_shard(rank, 3)
        parts.append(plan.run_host())
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)


def test_a_sample_2_to_the_40_below_the_others_declines_the_split():
    """alpha = 0.75: the shrunk sample's total of terms is 2^-30 of the others', under the 2 (rare rows) 2^-e the
    truncation may cost (at alpha = 0.5 it is 2^-20 of them, which the bound still accepts at these 4,000 rows)."""
    nodes = table(130, 0.1, shrunk=20)
    plan = forced_plan(nodes, alpha=0.75)
    assert plan.info.rare_rows == 0 and plan.info.kernel == K_GENERAL
    check_values(plan.run_host(), reference(nodes, 0.75), 130)
    assert forced_plan(table(130, 0.1), alpha=0.75).info.rare_rows > 0


def test_cli_with_the_split_forced_through_the_environment():
    sparse, tree = os.path.join(GOLDEN, "wtd.sparse"), os.path.join(GOLDEN, "wtd.tree")
    nodes = ff.flatten(ff.parse_sparse_abundance(open(sparse).read()), ff.Tree.read_file(tree))
    r = subprocess.run([L.FRCFRC_PATH, "-w", "-s", "-g", "0.5", "-i", sparse, "-t", tree], capture_output=True,
                       env=dict(os.environ, FF_SPARSE_SPLIT="1"))
    assert r.returncode == 0, r.stderr
    assert np.max(np.abs(np.array([float(x) for x in r.stdout.split()]) - reference(nodes, 0.5))) <= TOL
