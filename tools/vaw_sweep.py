"""pair_vaw_kernel beside pair_general_kernel at alpha = 0.5 on the same table of counts: kernel ms per pass, medians of
three alternating rounds in one session, and the share of (row, branch) cells on each chain of the kernel.
python tools/vaw_sweep.py [SAMPLESxLEAVES@DENSITY ...]   (default: C3's shape)
python tools/vaw_sweep.py --skip [SAMPLESxLEAVES@DENSITY ...]: pair_vaw_kernel (FF_VAW_SKIP=0) beside pair_vaw_skip_kernel
(FF_VAW_SKIP=1) and the switch unset, the same method; the (tile, row) cells by kind, counted here from the table; and
whether the three variants' distances are the same bits."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import frackyfrac_amd as ff
from frackyfrac_amd import synth

ROUNDS, PASSES = 3, 3


def cell_kinds(nodes, n, rows, h):
    """(tile, row) cells of the whole triangle's h x 64 tiles by kind -- both groups have the branch, only the rows, only
    the columns -- as fractions of all cells, from the table alone (staged rows = branches some sample has)."""
    sample = np.repeat(np.arange(n), np.diff(nodes.indptr))[nodes.abnd > 0]
    row = np.unique(nodes.branch_id[nodes.abnd > 0], return_inverse=True)[1]
    dev = torch.device("cuda")
    occ = lambda g: torch.zeros(((n + g - 1) // g, rows), device=dev).index_put_(  # noqa: E731
        (torch.as_tensor(sample // g, device=dev), torch.as_tensor(row, device=dev)), torch.ones((), device=dev))
    R, C = occ(h), occ(64)
    gi = torch.arange(R.shape[0], device=dev)
    # tile (row group gi, column group gj) exists where it holds a pair j < i: 64 gj < min(h gi + h, n) - 1
    live = (64 * torch.arange(C.shape[0], device=dev)[None, :] < (torch.clamp(h * gi + h, max=n) - 1)[:, None]).double()
    both = ((R.double() @ C.double().T) * live).sum().item()
    rows_have = (R.double().sum(1)[:, None] * live).sum().item()
    cols_have = (C.double().sum(1)[None, :] * live).sum().item()
    cells = live.sum().item() * rows
    return both / cells, (rows_have - both) / cells, (cols_have - both) / cells


def skip_sweep(specs):
    for spec in specs:
        shape, dens = spec.split("@")
        n, nl = (int(x) for x in shape.split("x"))
        tree, ptr, idx, val = synth.make(n, nl, float(dens), synth.CONFIGS["C3"]["seed"])
        nodes = ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), ptr, idx, np.ceil(1e4 * val), leave_unnormalized=True)
        plans = {}
        for name, v in (("dense", "0"), ("skip forced", "1"), ("unset", None)):
            os.environ.pop("FF_VAW_SKIP", None)
            if v is not None:
                os.environ["FF_VAW_SKIP"] = v
            plans[name] = ff.Plan(nodes, True, variance_adjusted=True)
        os.environ.pop("FF_VAW_SKIP", None)
        outs = {k: torch.empty(ff.num_pairs(n), dtype=torch.float64, device="cuda") for k in plans}
        ms = {k: [] for k in plans}
        for k, p in plans.items():  # warm-up, and the distances to compare
            p.run(outs[k].data_ptr())
        torch.cuda.synchronize()
        same = all(torch.equal(outs["dense"].view(torch.int64), o.view(torch.int64)) for o in outs.values())
        for _ in range(ROUNDS):
            for k, p in plans.items():
                for _ in range(PASSES):
                    p.run(outs[k].data_ptr(), timed=True)
                torch.cuda.synchronize()
                t, c = p.timing_collect()
                ms[k].append(t / c)
        for k, p in plans.items():
            i = p.info
            print("%-18s %-12s H %2d  rows %6d  tiles %7d  active_fraction %.4f  non-empty slabs %10d  terms %.4g  ms/pass median %9.3f  (rounds %s)" % (
                spec, k, 8 if i.active_fraction < 1 else round(i.elements / i.n_tiles / 64 / max(i.n_rows, 1)), i.n_rows, i.n_tiles,
                i.active_fraction, i.n_items, i.elements, float(np.median(ms[k])), " ".join("%.3f" % x for x in ms[k])), flush=True)
        rows = plans["dense"].info.n_rows
        print("%-18s cells of 8 x 64 tiles: both %.4f, rows only %.4f, columns only %.4f, neither %.4f; same bits: %s" % (
            (spec,) + (lambda b, r, c: (b, r, c, 1 - b - r - c))(*cell_kinds(nodes, n, rows, 8)) + (same,)), flush=True)
        for p in plans.values():
            p.close()


if sys.argv[1:2] == ["--skip"]:
    skip_sweep(sys.argv[2:] or ["4096x10000@0.1"])
    sys.exit(0)
for spec in sys.argv[1:] or ["4096x10000@0.1"]:
    shape, dens = spec.split("@")
    n, nl = (int(x) for x in shape.split("x"))
    tree, ptr, idx, val = synth.make(n, nl, float(dens), synth.CONFIGS["C3"]["seed"])
    nodes = ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), ptr, idx, np.ceil(1e4 * val), leave_unnormalized=True)
    plans = {"alpha 0.5": ff.Plan(nodes, True, alpha=0.5), "variance adjusted": ff.Plan(nodes, True, variance_adjusted=True)}
    out = torch.empty(ff.num_pairs(n), dtype=torch.float64, device="cuda")
    ms = {k: [] for k in plans}
    for k, p in plans.items():  # warm-up
        p.run(out.data_ptr())
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, p in plans.items():
            for _ in range(PASSES):
                p.run(out.data_ptr(), timed=True)
            torch.cuda.synchronize()
            t, c = p.timing_collect()
            ms[k].append(t / c)
    for k, p in plans.items():
        print("%-18s %-18s kernel %d  H %2d  rows %6d  tiles %7d  staged %.2f GB  ms/pass median %8.3f  (rounds %s)" % (
            spec, k, p.info.kernel, p.info.n_tiles and round(p.info.elements / p.info.n_tiles / 64 / max(p.info.n_rows, 1)),
            p.info.n_rows, p.info.n_tiles, p.info.staged_bytes / 1e9, float(np.median(ms[k])), " ".join("%.3f" % x for x in ms[k])), flush=True)
    rows = plans["variance adjusted"].info.n_rows
    f = np.bincount(nodes.branch_id, minlength=nodes.n_branches) / n  # per branch: the share of samples that have it
    f = f[f > 0]
    print("%-18s cells on chain Y (row has the branch) %.4f, chain X %.4f; terms with a transcendental: variance adjusted %.4f "
          "(a side present), alpha 0.5 %.4f (both present); ms ratio %.3f" % (
              spec, f.sum() / rows, 1 - f.sum() / rows, (1 - (1 - f) ** 2).sum() / rows, (f * f).sum() / rows,
              float(np.median(ms["variance adjusted"]) / np.median(ms["alpha 0.5"]))), flush=True)
    for p in plans.values():
        p.close()
