"""pair_general_kernel beside the EXACT64 weighted pass on the same table: kernel ms per pass for alpha = 0.5, 0 and
0.25 -- every row in the matrix (FF_SPARSE_SPLIT=0) and the rare rows on pair_low_general_kernel (=1), with the rare
rows' share of the pass -- and for pair_exact64_skip_kernel, medians of three alternating rounds in one session.
python tools/general_sweep.py [SAMPLESxLEAVES@DENSITY ...]   (default: C3's shape and the 0.2 % density table)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import frackyfrac_amd as ff
from frackyfrac_amd import _lib as L, synth

ROUNDS, PASSES = 3, 3
for spec in sys.argv[1:] or ["4096x10000@0.1", "8192x50000@0.002"]:
    shape, dens = spec.split("@")
    n, nl = (int(x) for x in shape.split("x"))
    tree, ptr, idx, val = synth.make(n, nl, float(dens), synth.CONFIGS["C3"]["seed"])
    nodes = ff.flatten_leaf_csr(ff.parse_newick(tree.newick()), ptr, idx, val)
    plans = {"exact64 weighted": ff.Plan(nodes, True, precision="exact64")}
    for alpha in (0.5, 0.0, 0.25):
        for split in ("0", "1"):
            L.lib().ff_tune(b"FF_SPARSE_SPLIT", split.encode())
            plans["alpha %g split %s" % (alpha, split)] = ff.Plan(nodes, True, alpha=alpha)
    L.lib().ff_tune(b"FF_SPARSE_SPLIT", None)
    out = torch.empty(ff.num_pairs(n), dtype=torch.float64, device="cuda")
    ms, rare = {k: [] for k in plans}, {k: [] for k in plans}
    for k, p in plans.items():  # warm-up
        p.run(out.data_ptr())
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, p in plans.items():
            for _ in range(PASSES):
                p.run(out.data_ptr(), timed=True)
            torch.cuda.synchronize()
            t, r, c = p.timing_collect_parts()
            ms[k].append(t / c)
            rare[k].append(r / c)
    for k, p in plans.items():
        print("%-18s %-18s kernel %d  H %2d  rows %6d  rare %6d  updates %.3g  tiles %7d  ms/pass median %8.3f  of which rare %8.3f  (rounds %s)" % (
            spec, k, p.info.kernel, p.info.n_tiles and round(p.info.elements / p.info.n_tiles / 64 / max(p.info.n_rows, 1)),
            p.info.n_rows, p.info.rare_rows, p.info.rare_updates, p.info.n_tiles, float(np.median(ms[k])), float(np.median(rare[k])),
            " ".join("%.3f" % x for x in ms[k])), flush=True)
        p.close()
