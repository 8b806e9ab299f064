"""pair_vaw_kernel beside pair_general_kernel at alpha = 0.5 on the same table of counts: kernel ms per pass, medians of
three alternating rounds in one session, and the share of (row, branch) cells on each chain of the kernel.
python tools/vaw_sweep.py [SAMPLESxLEAVES@DENSITY ...]   (default: C3's shape)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import frackyfrac_amd as ff
from frackyfrac_amd import synth

ROUNDS, PASSES = 3, 3
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
