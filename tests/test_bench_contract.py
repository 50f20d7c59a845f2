"""bench.py prints ONE compact JSON line (< 4 KB, the LAST stdout line).  A plain run carries the headline alone and can dump what its
last timed step computed (--dump-outputs); with --full the line carries `roofline` and `cpu_baseline` and the full record goes to
--full-out (GPU); its CPU leg and the compact-record builder work on their own (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return str(sock.getsockname()[1])


def _strict(line):
    """json.loads that refuses NaN / Infinity (a strict parser, like the driver's, rejects them)"""
    def bad(c):
        raise ValueError(f"non-finite constant {c} in the bench line")
    return json.loads(line, parse_constant=bad)


def _bench(cmd, tmp_path, env=None, timeout=900):
    """run bench.py (or a launcher around it) -> (compact record = the LAST stdout line, full record from --full-out)"""
    full = os.path.join(str(tmp_path), "bench_full.json")
    out = subprocess.run([*cmd, "--full-out", full], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len([l for l in lines if l.startswith("{")]) == 1 and lines[-1].startswith("{")       # ONE JSON line and it is the final line
    assert len(lines[-1]) < 4096, len(lines[-1])                                                  # round 5: 23.5 KB came back unparsed
    d = _strict(lines[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline"):
        assert k in d, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "launch_us", "algorithmic_bytes_per_launch", "served_by",
              "frac_timed_region", "frac_wall_clock", "frac_hbm_only"):
        assert k in d["roofline"], k

    def strings(v):
        if isinstance(v, str):
            yield v
        elif isinstance(v, dict):
            for x in v.values():
                yield from strings(x)
        elif isinstance(v, list):
            for x in v:
                yield from strings(x)
    assert all(len(x) <= 200 for x in strings(d)) and all(len(x) <= 120 for x in strings(d["roofline"]))
    assert "configs" not in d and "per_config" not in d["roofline"] and not any("note" in k for k in d["roofline"])
    f = _strict(open(full).read())
    for k in ("value", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert d[k] == f[k], k
    assert abs(d["roofline"]["frac"] - f["roofline"]["frac"]) < 1e-6 and d["roofline"]["kernel"] == f["roofline"]["kernel"]
    return d, f


def test_compact_record_of_a_full_record():
    """compact_record() on the builder's committed round-5 full record (23.5 KB): < 4 KB, strict JSON, roofline + cpu_baseline + ten
    scalar extras inside; on an 8-rank record: still < 4 KB with the per-rank short forms."""
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_20steps.json")))
    full["config"]["distinct_devices"] = 1
    line = json.dumps(bench.compact_record(full, "bench_full.json"), allow_nan=False, separators=(",", ":"))
    assert len(line) < 3000 < bench.COMPACT_LIMIT == 4096
    d = _strict(line)
    assert d["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-6) and d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert d["value"] == full["value"] and len(d["extras"]) == 10 and all(isinstance(v, (int, float)) for v in d["extras"].values())
    assert d["full_record"] == "bench_full.json" and "configs" not in d and "per_gpu" not in d
    full["n_gpus"], full["config"]["process_group"] = 8, "nccl"
    full["per_gpu"] = [{"rank": r, "device_index": r, "pci_bus_id": f"0000:{0x15 + r:02x}:00", "stream_id": r, "launch_us": 64.7284001, "steps_per_s": 6.1e10,
                        "initial_state_sha256_first_cubes": "ab" * 32} for r in range(8)]
    line8 = json.dumps(bench.compact_record(full, "bench_full.json"), allow_nan=False, separators=(",", ":"))
    assert len(line8) < bench.COMPACT_LIMIT and len(_strict(line8)["per_gpu"]) == 8


def test_cpu_baseline_leg_shape():
    sys.path.insert(0, ROOT)
    import bench
    cb = bench.cpu_baseline(budget_s=0.5)
    assert cb["kind"] == "port" and cb["unit"] == "steps/s" and cb["cores"] >= 1 and cb["value"] > 1e6
    assert cb["single_core_steps_per_s"] > 1e6 and cb["numpy_env_1core_steps_per_s"] > 1e3 and "sample" in cb


@pytest.mark.gpu
def test_bench_json_line(tmp_path):
    c, d = _bench([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "3"], tmp_path, timeout=600)
    # the compact line (what the driver parses): contract keys, roofline and cpu_baseline IN THAT LINE, ten scalar extras
    assert c["n_gpus"] == 1 and c["steps"] == 20 and c["unit"] == "steps/s" and c["dtype"] == "u8" and c["vs_baseline"] is None
    assert c["scaling"] == "weak" and c["higher_is_better"] is True and "workload" in c["config"] and "model" not in c["config"]
    assert c["value"] > 1e9 and c["config"]["cubes_per_gpu"] == 1 << 22 and c["config"]["distinct_devices"] == 1 and c["config"]["pci_bus_id"]
    cr = c["roofline"]
    assert cr["bound"] == "hbm" and cr["unit"] == "GB/s" and cr["peak"] == 8000.0 and abs(cr["frac"] - cr["achieved"] / cr["peak"]) < 1e-6
    assert abs(cr["achieved"] - cr["algorithmic_bytes_per_launch"] / (cr["launch_us"] * 1e-6) / 1e9) < 1e-3 * cr["achieved"] and 0.5 < cr["frac"] < 1.0
    assert cr["kernel"].startswith("k_step<Cube3,V=") and cr["served_by"] == "hbm + infinity cache" and 0.5 < cr["frac_hbm_only"] < 0.95
    cb = c["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "steps/s" and cb["cores"] >= 1 and cb["value"] > 1e6 and len(cb["sample"]) <= 120
    assert cb["single_core_steps_per_s"] > 1e6 and cb["numpy_env_1core_steps_per_s"] > 1e3
    assert len(c["extras"]) == 10 and all(isinstance(v, (int, float)) and v > 0 for v in c["extras"].values()), c["extras"]
    assert c["full_record"].endswith("bench_full.json")
    # the full record (--full-out): everything the compact line leaves out
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["value"] > 1e9                     # the round's floor target: >= 1e9 cube-move steps/s
    assert r["traffic_source"] and r["device_copy_GBps"] > 1000 and d["cpu_baseline"]["value"] == pytest.approx(cb["value"], rel=1e-5)
    # the other BASELINE configs ride in the full record, each with its own roofline sub-record
    recs = d["configs"]["records"]
    names = " | ".join(x["config"] for x in recs)
    for needle in ("config 2", "config 3", "fused compact one-hot code", "fused dense f32", "fused dense bf16", "expansion of 1M", "2x2x2",
                   "compact code -> dense bf16"):
        assert needle in names, needle
    for x in recs:
        assert x["kernel"].startswith("k_") and x["launch_us"] > 0 and x["value"] > 0
        rr = x["roofline"]
        assert rr["peak"] == 8000.0 and 0.05 < rr["frac"] < 1.0 and abs(rr["frac"] - rr["achieved"] / rr["peak"]) < 1e-9
        assert rr["algorithmic_bytes_per_launch"] > 0
    adi = [x for x in recs if x["config"].startswith("config 3")][0]
    assert adi["roofline"]["bytes_per_unit"] == 715 and adi["roofline"]["frac"] > 0.6
    c5 = d["configs"]["config5_mcts_4096_leaves"]
    for k in ("hipgraph_serial_step_us", "serial_step_us", "batched_mcts_device_step_hipgraph_us", "batched_mcts_leaves_step_with_d2h_hipgraph_us",
              "batched_mcts_transfers_us", "batched_mcts_simulate_native_tree_ms", "batched_mcts_simulate_split_us"):
        assert k in c5, (k, c5)
    assert set(c5["batched_mcts_simulate_split_us"]) == {"select", "device_and_transfers", "update"}
    # host wall-clock figures on a shared pool gate only gross regressions (2x the measured value): round 5 measured 203-215 us
    assert c5["batched_mcts_leaves_step_with_d2h_hipgraph_us"] < 430 and "two_stream_step_us" not in c5
    # round 5: the loops the reference actually runs ride in the driver line
    ap = d["configs"]["adi_pipeline"]
    for size in ("200x30", "20000x30", "100000x30", "200x30_hipgraph", "2x2x2_20000x14"):
        assert ap[size]["seconds"] > 0 and ap[size]["samples_per_s"] > 0, ap
    assert ap["CubeEnv.get_random_samples_200x30"]["seconds"] < 12e-3 and ap["CubeEnv.get_random_samples_200x30_hipgraph"]["seconds"] < 12e-3, ap
    # measured 1.55 ms / 4.8-4.9 M samples/s; the bars are half of that (the reference: 15 s / 393 samples/s)
    assert ap["200x30"]["seconds"] < 4e-3 and ap["20000x30"]["samples_per_s"] > 2.4e6 and ap["100000x30"]["samples_per_s"] > 2.4e6, ap
    ro = d["configs"]["rollout"]
    assert all(ro[k]["us_per_timestep"] > 0 for k in ("n300_eager", "n300_hipgraph", "n65536_eager", "n65536_hipgraph")), ro
    rs = d["configs"]["reset_seeds_1M_k30"]
    assert rs["envs"] == 1 << 20 and rs["scramble_count"] == 30 and rs["legacy_actions_us"] < 1500 and rs["reset_ms"] < 3.0, rs   # device-event time (measured 150 us) / host clock measured 0.32 ms; round 4: 3.0 ms of draws
    for k in ("frac_basis", "frac_timed_region", "frac_wall_clock"):
        assert k in r, k
    assert abs(r["frac_timed_region"] - r["algorithmic_bytes_per_launch"] / (r["launch_us_timed_region"] * 1e-6) / 8e12) < 1e-6
    assert abs(r["frac_wall_clock"] - r["algorithmic_bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 8e12) < 1e-6 and r["frac_basis"].startswith("launch_us")
    # the facade must stay FASTER than the reference's own batch-1 step (24.6 us on one core; 11-12 us measured
    # here on an idle box).  Wall-clock on a shared host: the best of five 1100-step batches gates, the median only a gross regression
    fb = d["configs"]["facade_batch1"]
    assert fb["CubeEnv.step_us_best_batch"] < 24.6 and fb["CubeEnv.step_us"] < 50 and fb["config1_2x2x2"]["step_us"] < 50, fb
    # kernel names come from the library's dispatch (rc_describe_dispatch), never from literals
    assert r["kernel"].startswith("k_step<Cube3,V=") and "POL=" in r["kernel"] and "grid=" in r["kernel"]
    assert all("grid=" in x["kernel"] for x in recs)
    # the HBM-only point (2^24 cubes, 1.8 GB ping-pong: nothing cached) rides beside the 4M headline
    hbm = [x for x in recs if "nothing cached" in x["config"]][0]
    assert "POL=2" in hbm["kernel"] and abs(r["frac_hbm_only"] - hbm["roofline"]["frac"]) < 1e-12 and 0.5 < r["frac_hbm_only"] < 0.95
    assert r["served_by"] == "hbm + infinity cache" and d["config"]["cubes_per_gpu"] == 1 << 22
    assert any("IN PLACE" in x["config"] for x in recs)
    assert [x for x in recs if "compact code -> dense bf16" in x["config"]][0]["kernel"].startswith("k_code_to_dense_front<Cube3,bf16,F=1,lds>")
    f32 = [x for x in recs if "fused dense f32" in x["config"]][0]
    assert f32["kernel"].startswith("k_step<Cube3,V=2,move,store,code,POL=0>") and "+ k_code_to_dense_front<Cube3,f32,F=1,gather>" in f32["kernel"]
    # round 4: the dense one-hot writers no longer depend on where the output buffer lives (front writer / 64-cube tiles)
    for name in ("fused dense f32", "fused dense bf16", "compact code -> dense f32", "compact code -> dense bf16"):
        assert [x for x in recs if name in x["config"]][0]["roofline"]["frac"] > 0.75, name
    # the `roofline` object alone lets a reader recompute every fraction (the driver's parsed record keeps that key)
    assert r["achievable_GBps"] == 6300.0 and abs(r["frac_of_achievable"] - r["achieved"] / 6300.0) < 1e-9
    assert r["launch_batches"] >= 7 and r["launches_per_batch"] == 20
    assert r["launch_us_min"] <= r["launch_us"] <= r["launch_us_max"] and r["launch_us_timed_region"] > 0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["launch_us"] * 1e-6) / 1e9) < 1e-3 * r["achieved"]
    pc = {x["name"]: x for x in r["per_config"]}
    for name in ("cfg2 1M step+reward", "4M step in place", "4M step+reward", "4M step+reward+code", "16M step (HBM only)",
                 "1M step+dense f32", "1M step+dense bf16", "1M code->dense f32", "1M code->dense bf16", "1M expansion",
                 "cfg3 ADI 100k x 30", "ADI 100k x 30 codes", "ADI 100k x 30 family", "1M code->dense f16", "1M code->dense u8", "1M step+dense u8",
                 "2x2x2 1M expansion", "2x2x2 1M code->dense f32", "2x2x2 ADI blocks f32 20000x12", "ADI dense blocks f32 43008x1", "ADI dense blocks f32 20000x2", "ADI dense blocks bf16 43008x2"):
        x = pc[name]
        assert x["kernel"].startswith("k_") and abs(x["frac"] - x["bytes"] / (x["launch_us"] * 1e-6) / 8e12) < 2e-3, name
    assert len(r["per_config"]) == len(recs)
    assert pc["ADI dense blocks f32 43008x1"]["frac"] > 0.65 and pc["ADI dense blocks f32 43008x1"]["kernel"].startswith("k_code_to_dense_front<Cube3,f32,F=1,gather,family>")
    assert [x for x in recs if x["short"] == "ADI 100k x 30 family"][0]["roofline"]["bytes_per_unit"] == 64
    # the family record halves the code-emitting ADI launch (64 B per (walk, depth) instead of 327 B; round-3 review: <= 110 us)
    assert pc["ADI 100k x 30 family"]["launch_us"] < 110 and pc["ADI 100k x 30 family"]["launch_us"] < 0.7 * pc["ADI 100k x 30 codes"]["launch_us"]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["force_dist", "torchrun_1"])
def test_bench_distributed_branch_world1_rccl(how, tmp_path):
    """The branch the 2/4/8-GPU runs execute -- RCCL process group created with device_id, barrier, all_gather of device tensors,
    all_gather_object, all_reduce(MAX), destroy_process_group -- executed once on the one MI355X a builder has, at world size 1:
    once through --force-dist and once under the launcher the driver uses.  (The reference's workers never exchange anything
    either: train.py:85-92,141-147.)"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    tail = ["--full", "--steps", "20", "--warmup", "3", "--no-cpu", "--no-configs", "--backend", "nccl", "--cubes-per-gpu", str(1 << 20)]
    if how == "force_dist":
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist", *tail]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
               "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "1", *tail]
    c, d = _bench(cmd, tmp_path, env=env, timeout=600)
    assert d["n_gpus"] == 1 and d["config"]["process_group"] == "nccl" and d["value"] > 1e9
    assert len(d["per_gpu"]) == 1 and d["per_gpu"][0]["rank"] == 0 and d["per_gpu"][0]["stream_id"] == 0
    assert abs(d["roofline"]["aggregate_frac_of_n_x_peak"] - d["roofline"]["frac"]) < 1e-9
    assert "configs" not in d and "per_config" not in d["roofline"]


def test_bench_refuses_legacy_ipc_for_rccl():
    """RCCL needs dmabuf IPC on this driver stack: an explicitly exported HSA_ENABLE_IPC_MODE_LEGACY other than 0 is an error
    before anything touches the GPU, not a hipIpcGetMemHandle failure later (runs without a GPU)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist", "--backend", "nccl"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "HSA_ENABLE_IPC_MODE_LEGACY must be 0" in out.stderr, out.stderr[-1000:]


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal(oracle, tmp_path):
    """The N>1 path (one process per rank, barrier, MAX over ranks, rank 0 prints) rehearsed with two ranks sharing
    this box's single GPU over gloo, at BASELINE config 4's shape (1M cubes per rank, rank-distinct RNG streams, no collective
    on the env path; the reference's pattern is one env per worker process, train.py:85-92,141-147).  The driver runs the real
    thing with RCCL on 2/4/8 GPUs: `--cubes-per-gpu 1048576` is the only difference from the headline command."""
    import hashlib
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "20", "--warmup", "3", "--backend", "gloo",
           "--cubes-per-gpu", str(1 << 20)]
    # two ranks, one visible GPU: refused without --share-gpu (the line must never report N GPUs from fewer cards without saying so)
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert bad.returncode != 0 and "--share-gpu" in bad.stderr and not [l for l in bad.stdout.splitlines() if l.startswith("{")], bad.stderr[-2000:]
    cmd[cmd.index("--master-port") + 1] = _free_port()
    c, d = _bench(cmd + ["--share-gpu"], tmp_path, env=env, timeout=900)
    assert c["config"]["distinct_devices"] == 1 and c["config"]["shared_gpu_rehearsal"] is True and c["n_gpus"] == 2
    assert [x["dev"] for x in c["per_gpu"]] == [0, 0] and c["per_gpu"][0]["pci"] == c["per_gpu"][1]["pci"] and c["per_gpu"][0]["pci"]
    assert [x["requested_device_index"] for x in d["per_gpu"]] == [0, 1] and [x["device_index"] for x in d["per_gpu"]] == [0, 0]
    assert all(x["sha12"] == y["initial_state_sha256_first_cubes"][:12] for x, y in zip(c["per_gpu"], d["per_gpu"]))
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d and d["value"] > 1e9
    assert d["config"]["cubes_per_gpu"] == 1 << 20 and d["config"]["total_cubes"] == 2 << 20 and "configs[3]" in d["config"]["workload"]
    assert [r["rank"] for r in d["per_gpu"]] == [0, 1] and all(r["steps_per_s"] > 1e9 for r in d["per_gpu"])
    assert [r["stream_id"] for r in d["per_gpu"]] == [0, 1]                    # rank-distinct RNG streams
    assert d["roofline"]["aggregate_GBps"] > 0
    # every rank's first 65536 scrambled cubes are the oracle's (seed, stream_id = rank) stream
    import bench
    for r in d["per_gpu"]:
        exp = oracle.adi(3, r["sha_cubes"], bench.SCRAMBLE_DEPTH, seed=bench.SCRAMBLE_SEED, stream=r["stream_id"], want_children=False)["parents"][:, -1]
        assert hashlib.sha256(np.ascontiguousarray(exp, dtype=np.uint8).tobytes()).hexdigest() == r["initial_state_sha256_first_cubes"], r["rank"]
    assert d["per_gpu"][0]["initial_state_sha256_first_cubes"] != d["per_gpu"][1]["initial_state_sha256_first_cubes"]
    # N > 1 skips the other configs by default (--configs asks for them): rank 0 leaves with its peer, seven GPUs do not idle behind it
    assert "configs" not in d and "per_config" not in d["roofline"] and d["config"]["process_group"] == "gloo"


GPU_PROCESS_LIMIT = 6     # this pool's process guard: at most 6 processes of one job may use the GPU at once


@pytest.mark.gpu
def test_bench_many_ranks_rehearsal(oracle, tmp_path):
    """BASELINE config 4 is 8 ranks x 1M cubes.  With one GPU and a guard of 6 GPU processes per job -- of which this pytest process
    is one once any in-process GPU test has run, and the launcher another (round 5: 5 ranks + launcher + a pytest process that already
    held the GPU = 7 = a killed run) -- the rehearsal is FOUR ranks x 1M cubes sharing the GPU over gloo, --no-configs: distinct stream_ids,
    oracle-matching shas, the aggregate keys of the N > 1 line.  `bench.py --gpus 8 --cubes-per-gpu 1048576` under the driver's
    launcher is this same code path with backend nccl (exercised at world size 1 above).  Eight streams against the oracle without
    a GPU: tests/test_host_logic.py::test_eight_rank_streams_and_shards."""
    import hashlib
    ranks = GPU_PROCESS_LIMIT - 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--full", "--steps", "20", "--warmup", "3",
           "--backend", "gloo", "--share-gpu", "--cubes-per-gpu", str(1 << 20)]
    c, d = _bench(cmd, tmp_path, env=env, timeout=900)
    assert c["config"]["distinct_devices"] == 1 and c["config"]["shared_gpu_rehearsal"] is True and len(c["per_gpu"]) == ranks
    assert d["n_gpus"] == ranks and d["config"]["total_cubes"] == ranks << 20 and "configs" not in d
    assert [r["rank"] for r in d["per_gpu"]] == list(range(ranks)) and [r["stream_id"] for r in d["per_gpu"]] == list(range(ranks))
    assert 0 < d["roofline"]["aggregate_frac_of_n_x_peak"] < 1 and d["roofline"]["aggregate_GBps"] > 0
    import bench
    shas = set()
    for r in d["per_gpu"]:
        exp = oracle.adi(3, r["sha_cubes"], bench.SCRAMBLE_DEPTH, seed=bench.SCRAMBLE_SEED, stream=r["stream_id"], want_children=False)["parents"][:, -1]
        assert hashlib.sha256(np.ascontiguousarray(exp, dtype=np.uint8).tobytes()).hexdigest() == r["initial_state_sha256_first_cubes"], r["rank"]
        shas.add(r["initial_state_sha256_first_cubes"])
    assert len(shas) == ranks


@pytest.mark.parametrize("ranks", [2, 4, 8])
def test_bench_eight_ranks_dry_run(ranks, tmp_path):
    """The N = 8 line's plumbing without a GPU (RC_BENCH_DRY=1: no kernel, numbers mean nothing): the driver's launcher shape
    (`torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8`), a process group, eight contiguous stream ids, barrier,
    all_gather, MAX over ranks, ONE JSON line from rank 0 with eight `per_gpu` entries and total_cubes = 8 x 2^20 -- so that the first
    real 8-GPU run cannot fail on anything but the kernels (which the one-GPU tests cover).  Pattern: train.py:85-92."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", RC_BENCH_DRY="1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--full", "--steps", "5", "--warmup", "1", "--backend", "gloo",
           "--cubes-per-gpu", str(1 << 20)]
    c, d = _bench(cmd, tmp_path, env=env, timeout=600)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "per_gpu"):
        assert k in d, k
    assert d["dry_run"] is True and "NO kernel ran" in d["data"] and "cpu_baseline" not in d and "configs" not in d
    assert d["n_gpus"] == ranks and d["steps"] == 5 and d["scaling"] == "weak" and d["unit"] == "steps/s" and d["dtype"] == "u8"
    assert d["config"]["cubes_per_gpu"] == 1 << 20 and d["config"]["total_cubes"] == ranks << 20 and "configs[3]" in d["config"]["workload"]
    assert d["config"]["process_group"] == "gloo" and d["config"]["parallelism"].startswith(f"{ranks} independent ranks")
    assert [r["rank"] for r in d["per_gpu"]] == list(range(ranks)) and [r["stream_id"] for r in d["per_gpu"]] == list(range(ranks))
    assert d["roofline"]["kernel"].startswith("k_step<Cube3,V=2,move,store,POL=0>")         # 1M cubes per GPU: the resident policy
    assert d["roofline"]["aggregate_GBps"] > 0 and "aggregate_frac_of_n_x_peak" in d["roofline"]
    # every rank REQUESTS its own device (LOCAL_RANK), never local_rank % device_count: eight ranks ask for eight distinct indices
    assert [r["requested_device_index"] for r in d["per_gpu"]] == list(range(ranks)) == [r["device_index"] for r in d["per_gpu"]]
    assert c["config"]["distinct_devices"] == ranks and [x["dev"] for x in c["per_gpu"]] == list(range(ranks)) and c["dry_run"] is True
    assert c["config"]["shared_gpu_rehearsal"] is False and "cpu_baseline" not in c and "extras" not in c
    if ranks != 8:
        return
    # a dry run refuses the RCCL backend (it would touch the GPUs)
    env1 = {k: v for k, v in env.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist", "--backend", "nccl"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env1)
    assert bad.returncode != 0 and "RC_BENCH_DRY" in bad.stderr


HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _plain(cmd, env=None, timeout=600):
    """run a plain bench.py (no --full) -> its one JSON line, which carries the headline and nothing measured beyond it"""
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len([l for l in lines if l.startswith("{")]) == 1 and lines[-1].startswith("{")
    c = _strict(lines[-1])
    for k in HEADLINE_KEYS:
        assert k in c, k
    assert not {"roofline", "cpu_baseline", "extras", "full_record", "configs"} & set(c), sorted(c)
    assert abs(c["value"] - c["config"]["total_cubes"] / (c["ms_per_step"] * 1e-3)) < 1e-6 * c["value"]      # ms_per_step = one timed step
    return c


def test_bench_plain_dry_run_is_lean():
    """A plain N = 2 dry run: the headline keys and the short per-rank list, no roofline / cpu_baseline / extras / full record.  The dump
    sample is fixed: the same 2^17 ascending distinct indices every time."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", RC_BENCH_DRY="1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1", "--backend", "gloo",
           "--cubes-per-gpu", str(1 << 20)]
    c = _plain(cmd, env=env)
    assert c["dry_run"] is True and c["n_gpus"] == 2 and c["steps"] == 5 and c["unit"] == "steps/s" and c["dtype"] == "u8"
    assert [x["stream"] for x in c["per_gpu"]] == [0, 1] and not any("sha12" in x or "launch_us" in x for x in c["per_gpu"])
    assert c["config"]["distinct_devices"] == 2
    sys.path.insert(0, ROOT)
    import bench
    idx = bench.dump_sample(bench.N_CUBES)
    assert len(idx) == bench.DUMP_CUBES == 1 << 17 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < bench.N_CUBES
    assert (bench.dump_sample(bench.N_CUBES) == idx).all() and (bench.dump_sample(1000) == np.arange(1000)).all()


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step_outputs(oracle, tmp_path):
    """bench.py without --full: the headline line alone, and --dump-outputs writes what the last of the warmup + timed steps computed for
    the fixed sample of cubes -- replayed here through the oracle from the same seeded scramble and actions."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, steps, warmup = bench.DUMP_CUBES + 4097, 20, 3
    out_dir = tmp_path / "outputs"
    c = _plain([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--cubes-per-gpu", str(n),
                "--dump-outputs", str(out_dir)])
    assert c["n_gpus"] == 1 and c["steps"] == steps and c["warmup"] == warmup and c["config"]["cubes_per_gpu"] == n and c["value"] > 0
    assert sorted(os.listdir(out_dir)) == ["done.npy", "states.npy"]
    states, done = np.load(out_dir / "states.npy"), np.load(out_dir / "done.npy")
    idx = bench.dump_sample(n)
    assert states.dtype == np.float32 and states.shape == (len(idx), 54) and done.dtype == np.float32 and done.shape == (len(idx),)
    assert states.nbytes + done.nbytes <= 64 << 20
    st = oracle.adi(3, n, bench.SCRAMBLE_DEPTH, seed=bench.SCRAMBLE_SEED, stream=0, threads=4, want_children=False)["parents"][:, -1]
    acts = torch.randint(0, 12, (n,), generator=torch.Generator(device="cuda:0").manual_seed(1), device="cuda:0", dtype=torch.uint8).cpu().numpy()
    for _ in range(warmup + steps):
        st, _, d, _ = oracle.step(3, st, acts, threads=4)
    assert (states == st[idx]).all() and (done == d[idx]).all()
