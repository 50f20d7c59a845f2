#!/usr/bin/env python3
"""What the subgroup chain costs on one GPU (development tool; DESIGN.md "Subgroup chain").  Writes profiles/chain.json (or --out);
every number is measured on the device, nothing is estimated.  It has no --prove mode: tests/test_gpu_chain.py proves every index of
every table on each run of the suite.

    python tools/bench_chain.py [--out profiles/chain.json] [--log2n 20]

  build     ChainTables.build's loop per stage (rct_build_begin, one rct_build_level per distance, the count read back per level): a
            device event pair per stage, median of --builds builds after one warm-up build;
  descend   rct_descend of each stage alone at 2^log2n cubes scrambled by 100 device moves: the cubie rows, lengths and actions are put
            back to the stage's entry state before every timed call (copies outside the event pair); median of --runs calls;
  solve     the whole search.chain_solve, eager and as one hipGraph (its own capture: the launches chain_solve(graph=True) makes), a
            host clock around work that ends in a synchronise for the eager call and device events around the replay; median of --runs;
  lengths   the histogram of the solutions' quarter turns and of the generators per stage."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rubiks_cube_solver_amd import VecCubeEnv, _chain_lib, _lib, ops, search  # noqa: E402
from rubiks_cube_solver_amd.pattern import MAX_LEVELS, ChainTables  # noqa: E402

ML = _chain_lib.MAX_LENGTH


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": len(v)}


def build_times(dev, builds):
    """-> per stage the total ms samples of the build loop, and the level counts"""
    L, P, sp = _chain_lib.chain_lib(), _lib.ptr, _lib.stream_ptr(dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    out = []
    for stage in range(_chain_lib.STAGES):
        n = _chain_lib.table_bytes(stage)
        table = torch.empty(n, dtype=torch.uint8, device=dev)
        totals, levels = [], None
        for b in range(builds + 1):                              # the first build is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert L.rct_build_begin(P(table), n, stage, sp) == 0
            lv = []
            for depth in range(MAX_LEVELS + 1):
                assert L.rct_build_level(P(table), n, stage, depth, P(count), sp) == 0
                c = int(count[0])                                # the synchronisation of the real loop
                if c == 0:
                    break
                lv.append(c)
            e1.record()
            torch.cuda.synchronize()
            if b:
                totals.append(e0.elapsed_time(e1))
            levels = lv
        out.append({"stage": stage, "table_bytes": n, "levels_after_the_goals": levels, "depth": len(levels), "launches": 2 * (len(levels) + 1) + 1,
                    "total_ms": stats(totals)})
        print(json.dumps(out[-1]), flush=True)
    return out


def descend_legs(chain, env, runs):
    """Each stage alone on the cubes the earlier stages left."""
    n, dev = env.num_envs, chain.device
    L, P, sp = _chain_lib.chain_lib(), _lib.ptr, _lib.stream_ptr(dev)
    cub = ops.cubies(env.stickers, n, 3, status=False)["cubies"]
    pitch = int(cub.shape[-1])
    ap = _lib.pitch_for(n, 16)
    actions = torch.full((ML, ap), 12, dtype=torch.uint8, device=dev)
    length = torch.zeros(ap, dtype=torch.int32, device=dev)
    moves, status = torch.empty(ap, dtype=torch.uint8, device=dev), torch.empty(ap, dtype=torch.uint8, device=dev)
    out = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for stage in range(_chain_lib.STAGES):
        t = chain.tables[stage]
        entry = (cub.clone(), actions.clone(), length.clone())
        call = lambda: L.rct_descend(P(cub), n, pitch, stage, P(t), t.numel(), P(actions), ML, ap, P(length), P(moves), P(status), sp)
        us = []
        for r in range(runs + 2):                                # two warm-up calls
            for dst, src in zip((cub, actions, length), entry):
                dst.copy_(src)
            torch.cuda.synchronize()
            e0.record()
            assert call() == 0
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                us.append(e0.elapsed_time(e1) * 1e3)
        assert not bool(status[:n].any())
        gens = moves[:n].float()
        taken = (length[:n] - entry[2][:n]).float()
        med = statistics.median(us)
        out.append({"stage": stage, "n_cubes": n, "us": stats(us), "generators_mean": round(float(gens.mean()), 3), "generators_max": int(gens.max()),
                    "quarter_turns_mean": round(float(taken.mean()), 3),
                    "table_reads": int((gens.sum() * len(_chain_lib.generators(stage))).item()) + n,
                    "ns_per_cube": round(med * 1e3 / n, 4), "ns_per_cube_step": round(med * 1e3 / max(float(gens.sum()), 1.0), 4),
                    # what the rule needs: 20 rows in, 20 out for a walked cube, length in and out, moves, status, the actions written
                    "byte_model": int(n * (20 + 20 + 8 + 2) + taken.sum().item())})
        print(json.dumps(out[-1]), flush=True)
    return out


def solve_legs(chain, env, runs):
    dev = chain.device
    eager, replay = [], []
    res = None
    for r in range(runs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = search.chain_solve(chain, env)
        torch.cuda.synchronize()
        if r >= 2:
            eager.append((time.perf_counter() - t0) * 1e3)
    g = []
    for r in range(runs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = search.chain_solve(chain, env, graph=True)
        torch.cuda.synchronize()
        if r >= 2:
            g.append((time.perf_counter() - t0) * 1e3)
    assert all(torch.equal(out[k], res[k]) for k in res)
    # the device time of the launches alone, as a graph of this tool's own: what a caller who keeps the graph pays per batch
    n = env.num_envs
    cub = ops.alloc_code(n, 3, dev, env.stickers.shape[-1])
    ap = _lib.pitch_for(n, 16)
    legal, length = torch.empty(ap, dtype=torch.uint8, device=dev), torch.empty(ap, dtype=torch.int32, device=dev)
    actions, moves, status = (torch.empty((rows, ap), dtype=torch.uint8, device=dev) for rows in (ML, 4, 4))
    L, P, sp = _chain_lib.chain_lib(), _lib.ptr, lambda: _lib.stream_ptr(dev)

    def launches():
        ops.cubies(env.stickers, n, 3, cubies=cub, status=legal[:n])
        actions.fill_(12)
        length.copy_(legal.ne(0).to(torch.int32).neg())
        for s in range(4):
            t = chain.tables[s]
            assert L.rct_descend(P(cub), n, int(cub.shape[-1]), s, P(t), t.numel(), P(actions), ML, ap, P(length), P(moves[s]), P(status[s]), sp()) == 0

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launches()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(runs + 2):
        torch.cuda.synchronize()
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            replay.append(e0.elapsed_time(e1))
    assert torch.equal(length[:n], res["length"]) and not bool(status[:, :n].any())
    ln = res["length"].cpu().numpy()
    mv = res["stage_moves"].cpu().numpy().astype(np.int64)
    return ({"n_cubes": n, "solved": int(res["solved"].sum()), "chain_solve_eager_ms_host_clock": stats(eager),
             "chain_solve_graph_ms_host_clock_capture_included": stats(g), "kept_graph_replay_ms_device_events": stats(replay),
             "cubes_per_second_kept_graph": round(n / (statistics.median(replay) * 1e-3))},
            {"quarter_turns": {"mean": round(float(ln.mean()), 3), "min": int(ln.min()), "max": int(ln.max()), "histogram": np.bincount(ln).tolist()},
             "generators": {"mean": round(float(mv.sum(0).mean()), 3), "max": int(mv.sum(0).max()),
                            "per_stage_histogram": [np.bincount(mv[s]).tolist() for s in range(4)]}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain.json"))
    ap.add_argument("--builds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--log2n", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_chain needs a GPU: nothing is estimated"
    assert a.builds >= 7 and a.runs >= 7, "medians of at least 7 runs"
    dev = torch.device("cuda", 0)
    _lib.init(dev)
    rec = {"command": "python tools/bench_chain.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around single calls after two warm-up calls, medians; the eager chain_solve by a host clock around work that "
                     "ends in a synchronise (it allocates, launches and reads the longest length back)"}
    rec["build"] = build_times(dev, a.builds)
    chain = ChainTables.build(dev)
    with torch.no_grad():
        env = VecCubeEnv(1 << a.log2n, dev, 3, obs=None)
        env.reset(scramble_count=100)
        rec["descend"] = descend_legs(chain, env, a.runs)
        rec["solve"], rec["lengths"] = solve_legs(chain, env, a.runs)
    print(json.dumps(rec["solve"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
