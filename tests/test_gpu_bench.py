"""bench.py end to end on the GPU box: the N = 1 line with its `secondary` entries, and the
N > 1 path through the SELF-LAUNCH (`python bench.py --gpus 2`, no torch.distributed.run around
it) rehearsed with two ranks on the one GPU (gloo as control plane)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=900):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def test_self_launch_runs_two_ranks_and_prints_one_line():
    out, err = run_bench("--gpus", "2", "--rehearse-on-one-gpu", "--steps", "3", "--warmup", "1", "--workload",
                         "768x1500", "--no-cpu-baseline", "--no-secondary", "--scaling", "strong")
    assert "launching 2 ranks" in err
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "strong"
    assert out["config"]["pairs"] == 768 * 767 // 2
    assert out["gather"]["transport"] in ("ipc", "nccl")
    assert "REHEARSAL" in out["data"]
    assert out["roofline"]["launches"] == 3 and out["roofline"]["kernel_ms"] > 0
    # what the first real multi-GPU run will need for a post-mortem: every rank's own figures, the transport
    # that ran and why the other did not, the process group as the backend saw it
    g = out["gather"]
    assert g["backend"] == "gloo" and g["world_size"] == 2 and g["chunks"] == 1
    assert (g["fallback_reason"] is None) == (g["transport"] == "ipc")
    assert g["exposed_ms_last_step_max"] >= 0
    ranks = out["ranks"]
    assert [r["rank"] for r in ranks] == [0, 1] and sum(r["pairs"] for r in ranks) == 768 * 767 // 2
    for r in ranks:
        assert r["kernel_ms"] > 0 and r["launches"] == 3 and r["elapsed_ms_per_step"] >= r["kernel_ms"] * 0.5
        assert r["transport"] == g["transport"] and r["device"] and r["local_rank"] == 0
    assert ranks[0]["exposed_gather_ms_last_step"] == 0 or g["transport"] == "nccl"
    assert out["roofline"]["floor_ms"] > 0 and out["roofline"]["floor_ms"] < out["roofline"]["kernel_ms"]
    # value = all ranks' pairs over the MAX-over-ranks time of the timed steps
    assert abs(out["value"] - sum(r["pairs"] for r in ranks) / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["ms_per_step"] >= max(r["elapsed_ms_per_step"] for r in ranks) * (1 - 1e-9)
    assert "nccl" in g["untested_transport"] and "gloo" in g["untested_transport"]
    # weak scaling: the sample count grows as sqrt(N), rounded to 32
    out, _ = run_bench("--gpus", "2", "--rehearse-on-one-gpu", "--steps", "2", "--warmup", "1", "--workload",
                       "768x1500", "--no-cpu-baseline", "--no-secondary")
    assert out["scaling"] == "weak" and out["config"]["pairs"] == 1088 * 1087 // 2


def test_plain_run_is_the_primary_record_alone_and_dumps_the_last_steps_distances(tmp_path):
    """Without --full the line is the primary record: nothing that takes runs of its own (secondary entries, CPU baseline,
    end to end, live counter passes).  --dump-outputs leaves the last timed step's distances, one float64 per pair in
    IterPairs order, and they are the oracle's on the same seeded inputs within FIXED32's bar."""
    import numpy as np

    import bench
    from frackyfrac_amd import synth
    from oracle import oracle as O

    d = tmp_path / "dump"
    out, _ = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "768x1500", "--dump-outputs", str(d))
    assert out["metric"] and out["unit"] == "pairs/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["roofline"]["launches"] == 3
    pairs = 768 * 767 // 2
    assert out["config"]["pairs"] == pairs and abs(out["value"] - pairs / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    for k in ("secondary", "reference_width", "sparse_regime", "cpu_baseline", "end_to_end"):
        assert k not in out, k
    assert "traffic_note" not in out["roofline"] and "fetch_size_kib" not in out["roofline"]
    assert sorted(p.name for p in d.iterdir()) == ["distances.npy"]
    got = np.load(d / "distances.npy")
    assert got.dtype == np.float64 and got.shape == (pairs,)
    ctx = bench.Ctx()
    ctx.rank, ctx.world = 0, 1
    cfg, _ = bench.make_problem(ctx, "768x1500")
    tree, ptr, idx, val = synth.make(cfg["n_samples"], cfg["n_leaves"], cfg["density"], cfg["seed"])
    ft = O.FlatTree(tree.names, tree.branch_len, tree.size, tree.parent)
    ip, on = O.flatten_samples(ft, ptr, idx, val, 0)
    want = O.unifrac_dists(ip, on, ft.dist, True)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want))


def test_single_gpu_line_carries_the_secondary_entries():
    out, _ = run_bench("--full", "--steps", "3", "--warmup", "1", "--secondary-steps", "2", "--cpu-budget", "3")
    assert out["n_gpus"] == 1 and out["dtype"] == "u32" and out["config"]["workload"].startswith("C3:")
    # (three quarters of C3's staged rows are reduced by pair_low_kernel: the fraction of the full 2*B count passes 1; each
    # kernel on its own rows is in `parts`, from the event the plan records between the two launches -- the matrix rows'
    # kernel cannot pass the vector ALU's peak on the lane-ops it does issue)
    r = out["roofline"]
    assert r["kernel"] == "pair_sad_kernel" and 0.5 < r["frac"] < 5 and "frac_note" in r   # (8 waves: fewer than 8,000 matrix rows)
    matrix, rare = r["parts"]
    assert matrix["kernel"] == "pair_sad_kernel" and rare["kernel"] == "pair_low_kernel"
    assert matrix["rows"] + rare["rows"] == r["rows_staged"] and rare["rows"] == r["rare_rows"]
    assert 0.5 < matrix["frac"] < 1.0 and 0 < rare["ms"] < r["kernel_ms_between_events"]
    assert abs(matrix["ms"] + rare["ms"] - r["kernel_ms"]) <= 1e-6 * r["kernel_ms"]
    # (the rare rows' kernel on its own work: updates of an LDS accumulator against the rate the LDS takes ds_add_u32 at)
    assert rare["bound"] == "lds" and 1e9 < rare["updates"] < 1e10 and 0.05 < rare["frac"] < 1.0
    assert abs(rare["achieved"] * 1e12 * rare["ms"] * 1e-3 - rare["updates"]) <= 1e-6 * rare["updates"]
    a = out["audit"]
    assert a["uniform_sample"] == 4096 and a["pairs"] == 4096 + a["risk_pairs_checked"] and a["failed"] == 0
    assert a["min_headroom"] is None or a["min_headroom"] >= 1.0   # (everything under 1 is re-computed exactly)
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["single_thread"]["cores"] == 1
    sec = out["secondary"]
    assert [e["config"]["workload"].split(":")[0] for e in sec] == ["C3", "C3", "C2", "C4", "C5", "C3", "C3"]
    assert [e["dtype"] for e in sec] == ["f64", "i8", "i8", "u32", "u32", "i8", "f64"]
    # the last one: C3 unweighted with log-normal branch lengths -- graded digit planes on the matrix cores, the
    # run-time audit against binary64 in play (lengths off the binary grid), every audited pair inside the bar
    assert "log-normal" in sec[5]["config"]["workload"] and sec[5]["roofline"]["kernel"] == "pair_common_mfma_kernel"
    assert sec[5]["audit"]["failed"] == 0 and sec[5]["audit"]["worst_rel_err"] <= 5e-7
    # ... and what the engine does with such lengths when nobody asks for fixed32: the reference's bits, on
    # pair_exact_unw_kernel, priced at two binary64 additions per branch and pair
    assert "log-normal" in sec[6]["config"]["workload"] and sec[6]["config"]["precision"] == "exact64"
    assert sec[6]["roofline"]["kernel"] == "pair_exact_unw_kernel" and "audit" not in sec[6]
    # the reference-width figure sits in the primary record too, with both operation counts
    rw = out["reference_width"]
    assert rw["dtype"] == "f64" and rw["value"] == sec[0]["value"] and rw["roofline"]["kernel"] == "pair_exact64_skip_kernel"
    assert abs(rw["roofline"]["frac_unfused6"] - 3.0 * rw["roofline"]["frac"]) < 1e-9
    # the rocprof-reported rate: the primary kernel's counter bytes per launch over this run's kernel time.  Either
    # measured on THIS box (two child runs under rocprofv3 --pmc, bench.py live_traffic) or -- a box whose profiler is
    # absent, refuses a counter or runs out of time -- the committed figure of profiles/traffic.json with a
    # `traffic_note` saying so: both are valid outcomes of the line.  (That the live figure agrees with the committed
    # one is asserted under `-m perf`, tests/test_gpu_perf.py: no profiler can fail the parity gate.)
    rl, hbm = out["roofline"], out["roofline"]["hbm"]
    assert rl["traffic"] > 0 and rl["traffic_source"]
    if "traffic_note" in rl:
        assert "committed" in rl["traffic_note"] or "profiler" in rl["traffic_note"]
        assert "fetch_size_kib" not in rl
    else:
        assert rl["traffic_source"].startswith("live on this box")
        assert abs(rl["traffic"] - (2 * rl["fetch_size_kib"] + rl["write_size_kib"]) * 1024) < 1.0
        assert rl["traffic_committed"] > 0
    assert hbm["measured_GBps"] > hbm["achieved"] and 0 < hbm["measured_frac_of_8000"] < hbm["measured_frac_of_6290"] < 1
    assert hbm["traffic_ratio"] > 1.0 and abs(hbm["traffic_ratio"] - rl["traffic"] / hbm["algorithmic_bytes"]) < 1e-9
    # end to end: host buffers, and the frcfrc executable on C3 and C4 as files -- default flags, -p 1,
    # -p <cores>: every run ends well, writes one line per pair, and the three outputs are the same bytes
    e2e = out["end_to_end"]
    assert e2e["host_buffers_ms"] > 0 and e2e["text_stream_ms"] > 0
    assert 15 * out["config"]["pairs"] < e2e["text_stream_bytes"] < 25 * out["config"]["pairs"]
    assert [e["workload"] for e in e2e["frcfrc"]] == ["C3", "C4"]
    for e in e2e["frcfrc"]:
        assert "error" not in e, e
        assert e["outputs_identical"] and e["lines_ok"], e
        assert [r["flags"] for r in e["runs"]] == ["(default)", "-p 1", "-p %d" % cb["cores"]]
        assert e["cold_start"]["rc"] == 0 and e["cold_start"]["wall_s"] > 0   # (the command's first run on the box, apart)
        for r in e["runs"]:
            assert r["rc"] == 0 and r["lines"] == e["pairs"] and r["precision"] == "fixed32"
            assert set(r["seconds"]) == {"tree", "load", "validate", "open", "convert", "distances", "write", "close"}
            assert r["detail"]["kernels"] > 0 and r["detail"]["text_bytes"] == int(round(r["output_MB"] * 1e6))
        assert e["runs"][0]["threads"] == cb["cores"] and e["runs"][1]["threads"] == 1
    assert sec[0]["config"]["precision"] == "exact64" and sec[0]["roofline"]["kernel"] == "pair_exact64_skip_kernel"
    assert sec[1]["roofline"]["bound"] == "mfma" and "unweighted" in sec[1]["config"]["workload"]
    assert sec[1]["roofline"]["kernel"] == "pair_common_mfma_kernel" and sec[2]["roofline"]["kernel"] == "pair_common_small_kernel"
    assert sec[3]["config"]["pairs"] == 16384 * 16383 // 2 and sec[4]["config"]["pairs"] == 8192 * 8191 // 2
    for e in sec:
        # (where the rare rows are reduced by pair_low_kernel, work is skipped: the fraction of the full 2*B count may pass 1)
        assert e["ms_per_step"] > 0 and 0 < e["roofline"]["frac"] < (40.0 if e["roofline"].get("rare_rows") else 1.0)
    assert out["roofline"]["kernels"] == ["pair_sad_kernel", "pair_low_kernel"] and out["roofline"]["rare_rows"] > 0
    assert sec[3]["roofline"]["kernels"][0] == "pair_sad_kernel12"   # (C4: 16 ms of matrix rows, the 12-wave variant)
    assert sec[3]["roofline"]["rare_rows"] > 0 and sec[4]["roofline"]["rare_rows"] > 0   # C4, C5
    sp = out["sparse_regime"]
    assert [e["roofline"]["kernels"][1] for e in sp] == ["pair_low_kernel"] * 2 and all(e["roofline"]["frac"] > 2 for e in sp)
    assert all(e["cpu_baseline"]["value"] > 0 and e["gpu_over_cpu_all_cores"] > 100 for e in sp)


def test_c2_pass_is_one_launch():
    """BASELINE configs[1] (512 samples x 2k-leaf tree, unweighted): the small-shard matrix-core kernel does the pair
    reduction, the sum over branch ranges and the division in ONE launch (two in round 2).  Steps this short are timed
    with an event pair around every 8th launch.  How many microseconds a pass takes is asserted in test_gpu_perf.py
    (`-m perf`), not here: a slower-clocked box must not be able to fail the parity gate."""
    out, _ = run_bench("--workload", "C2", "--steps", "400", "--warmup", "20", "--no-cpu-baseline", "--no-secondary",
                       "--no-live-traffic")
    assert out["config"]["workload"].startswith("C2:") and out["dtype"] == "i8" and out["config"]["pairs"] == 130816
    assert out["roofline"]["kernel"] == "pair_common_small_kernel" and out["roofline"]["bound"] == "mfma"
    assert out["roofline"]["timed_every"] == 8 and out["roofline"]["launches"] == 50
    assert 0 < out["roofline"]["kernel_ms"] <= out["ms_per_step"]


def test_default_multi_gpu_line_leads_with_c4_strong_and_carries_the_weak_one():
    """`python bench.py --gpus N` as the driver starts it (no --scaling, no --workload): the line leads with BASELINE
    configs[3] -- C4 at its stated size, pair tiles over the N ranks, "scaling": "strong" -- and carries the
    weak-scaled C3 beside it; C5 is the secondary entry.  Rehearsed with two ranks on the one GPU."""
    out, _ = run_bench("--full", "--gpus", "2", "--rehearse-on-one-gpu", "--steps", "2", "--warmup", "1", "--secondary-steps", "1",
                       "--no-cpu-baseline")
    assert out["n_gpus"] == 2 and out["scaling"] == "strong"
    assert out["config"]["workload"].startswith("C4:") and out["config"]["pairs"] == 16384 * 16383 // 2
    assert sum(r["pairs"] for r in out["ranks"]) == 16384 * 16383 // 2
    assert abs(out["value"] - 16384 * 16383 // 2 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    # (floor_ms prices ALL 2*B lane-ops per pair; with the rare rows reduced by pair_low_kernel fewer are issued and the
    # kernels may finish under it: roofline.frac_note)
    assert 0 < out["roofline"]["floor_ms"] and 0 < out["roofline"]["kernel_ms"]
    assert out["roofline"]["floor_ms"] < out["roofline"]["kernel_ms"] or out["roofline"].get("rare_rows", 0) > 0
    # the base of the strong curve: the same problem on one GPU, same build, same run
    sb = out["strong_base"]
    assert sb["n_gpus"] == 1 and sb["workload"].startswith("C4:") and sb["value"] > 0 and sb["kernel"].startswith("pair_sad_kernel")
    assert abs(sb["value"] - 16384 * 16383 // 2 / (sb["ms_per_step"] * 1e-3)) <= 1e-6 * sb["value"]
    weak = out["weak_scaling"]
    assert weak["scaling"] == "weak" and weak["config"]["workload"].startswith("C3:") and weak["config"]["pairs"] == 5792 * 5791 // 2
    assert [r["rank"] for r in weak["ranks"]] == [0, 1] and "C3" in out["scaling_note"]
    assert [e["config"]["workload"].split(":")[0] for e in out["secondary"]] == ["C5"]
