"""pair_vaw_skip_kernel: the row-skipping form of variance-adjusted weighted UniFrac against the dense form
of the same plan, bit for bit, and against the dense binary64 restatement of the definition.  Forced by FF_VAW_SKIP=1;
built at 8-row tiles only, so a plan forced to 16 rows must stay on the dense kernel.  Needs an MI355X: `pytest -m gpu`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L
from frackyfrac_amd import synth
from test_gpu_vaw import EMPTY, FLOAT32, GOLDEN, K_VAW, SAME_LEAF, TOL, TWIN, reference, slot

pytestmark = pytest.mark.gpu

# test_gpu_vaw.table's planted samples, each pair of them in different clusters of 40: twins, empty, under one leaf, under another
TWIN_FAR, EMPTY_FAR, SAME_LEAF_FAR, OTHER_LEAF_FAR = (45, TWIN[1]), (EMPTY[0], 49), (SAME_LEAF[0], 53), 95
SKIP_H = 8  # ff_schedule.hpp VW_SKIP_TILE_H


@functools.lru_cache(maxsize=None)
def clustered(ns, empty=False, nl=2000, per_sample=12, seed=21):
    """test_gpu_exact_unw_skip.clustered with integer counts, flattened undivided: empty (tile, slab) cells, cells only
    the tile's rows or only its columns have, cells both have (counts: DESIGN 4.15); 40 divides neither 8 nor 64."""
    tree = synth.yule_tree(nl, seed)
    rng = np.random.default_rng(seed)
    nc = -(-ns // 40)
    leaves = [tree.leaf_ids[np.sort(rng.choice(np.arange(c * nl // nc, (c + 1) * nl // nc), per_sample, replace=False))]
              for c in np.arange(ns) // 40]
    counts = [rng.integers(1, 200, per_sample).astype(np.float64) for _ in range(ns)]
    bl = rng.lognormal(-3.0, 1.5, tree.n)
    bl[0] = 0.0
    tree.branch_len = bl
    leaves[TWIN_FAR[0]], counts[TWIN_FAR[0]] = leaves[TWIN_FAR[1]], counts[TWIN_FAR[1]]
    for s in range(ns) if empty else EMPTY_FAR:
        leaves[s], counts[s] = leaves[s][:0], counts[s][:0]
    if not empty:
        one, other = leaves[0][0], leaves[90][0]
        for s, leaf, n in ((SAME_LEAF_FAR[0], one, 3.0), (SAME_LEAF_FAR[1], one, 8.0), (OTHER_LEAF_FAR, other, 5.0)):
            leaves[s], counts[s] = np.array([leaf]), np.array([n])
    return ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), np.cumsum([0] + [len(x) for x in leaves]),
                               np.concatenate(leaves), np.concatenate(counts), leave_unnormalized=True)


def plan_with(monkeypatch, nodes, skip, h=SKIP_H, **kw):
    monkeypatch.setenv("FF_VAW_SKIP", skip)
    monkeypatch.setenv("FF_X_TILE_H", str(h))
    plan = ff.Plan(nodes, True, variance_adjusted=True, **kw)
    assert (plan.info.kernel, plan.info.precision) == (K_VAW, FLOAT32)
    return plan


same_bits = lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))  # noqa: E731


@pytest.mark.parametrize("h", [8, 16])
@pytest.mark.parametrize("ns", [130, 333])
def test_skipping_form_gives_the_dense_forms_bits_and_the_definition(monkeypatch, ns, h):
    nodes = clustered(ns)
    dense = plan_with(monkeypatch, nodes, "0", h)
    assert dense.info.active_fraction == 1.0
    want = dense.run_host()
    dense.close()
    plan = plan_with(monkeypatch, nodes, "1", h)
    print("ns %d H %d: active_fraction %.4f" % (ns, h, plan.info.active_fraction))
    # (no skipping kernel at 16 rows: the dense one, and the plan says so)
    assert 0.0 < plan.info.active_fraction < 1.0 if h == SKIP_H else plan.info.active_fraction == 1.0
    got = plan.run_host()
    plan.close()
    assert same_bits(got, want)
    ref = reference(nodes)
    single = SAME_LEAF_FAR + (OTHER_LEAF_FAR,)
    nan = np.zeros(ff.num_pairs(ns), dtype=bool)
    for i, j in [EMPTY_FAR, SAME_LEAF_FAR] + [(e, s) for e in EMPTY_FAR for s in single]:
        nan[slot(max(i, j), min(i, j))] = True
    assert np.array_equal(np.isnan(ref), nan) and np.array_equal(np.isnan(got), nan)
    worst = np.max(np.abs(got - ref)[~nan])
    print("ns %d H %d: worst |got - ref| = %.3g" % (ns, h, worst))
    assert worst <= TOL
    assert got[slot(*TWIN_FAR)] == 0.0
    for e in EMPTY_FAR:
        for o in set(range(ns)) - set(EMPTY_FAR) - set(single):
            assert got[slot(max(e, o), min(e, o))] == 1.0


def test_retargeted_shards_give_the_whole_plans_bits(monkeypatch):
    nodes = clustered(333)
    whole = plan_with(monkeypatch, nodes, "1").run_host()
    plan, parts = plan_with(monkeypatch, nodes, "1", rank=0, world=3), []
    for rank in range(3):
        plan.set_shard(rank, 3)
        assert 0.0 < plan.info.active_fraction < 1.0
        parts.append(plan.run_host())
    plan.close()
    assert same_bits(np.concatenate(parts), whole)


def test_every_sample_empty(monkeypatch):
    """Next to the shape of DESIGN 4.5's fault: no occupancy bit, only the streams' zero chunks are read, all 0 / 0."""
    plan = plan_with(monkeypatch, clustered(130, empty=True), "1")
    assert 0.0 <= plan.info.active_fraction < 1.0
    assert np.isnan(plan.run_host()).all()
    plan.close()


def test_cli_prints_the_same_bytes():
    sparse, tree = os.path.join(GOLDEN, "wtd.sparse"), os.path.join(GOLDEN, "wtd.tree")
    out = [subprocess.run([L.FRCFRC_PATH, "-w", "-s", "-vaw", "-i", sparse, "-t", tree], capture_output=True,
                          env=dict(os.environ, FF_VAW_SKIP=v)) for v in ("0", "1")]
    assert out[0].returncode == 0 and out[1].returncode == 0, (out[0].stderr, out[1].stderr)
    assert out[0].stdout and out[0].stdout == out[1].stdout
