#!/usr/bin/env python3
"""What IDA* costs on one GPU (development tool; DESIGN.md "IDA*").  Writes profiles/ida.json (or --out); every number is measured on
the device, nothing is estimated.  It has no --prove mode: tests/test_gpu_ida.py compares the search with its restatement on each run
of the suite.

    python tools/bench_ida.py [--out profiles/ida.json] [--log2n 20] [--cubes 1000]

  passes    ida_search alone at 2^log2n cubes scrambled by 100 device moves (none is solved inside the budget: every lane runs every
            pass), under no table, the corner table and MaxTable(corner, e{0..5}, e{6..11}): a device event pair around one launch of
            --steps passes, median of --runs launches; passes per second over all lanes, ns per pass of one lane, and the time one
            launch at ida_max_steps() would take by that rate -- the measurement the cap was chosen from;
  walks     --cubes walks each of 8..14 moves under the MaxTable: search.ida_search (limit 20, --budget passes per cube) and
            astar_search(front="table", batch 1, --iterations iterations) ALTERNATING in this process on the same cubes, a host clock
            around each call (it ends in a synchronise): solved share, median / largest node count, the time, A*'s overflow share, and
            whether the lengths are equal wherever both answered;
  split     split = 0 against split = 2 on the same --cubes cubes, twice each, at --split-lengths.
  The arguments of the run are kept in the file."""
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

from rubiks_cube_solver_amd import VecCubeEnv, _ida_lib, _lib, ops, search  # noqa: E402
from rubiks_cube_solver_amd.pattern import CornerTable, EdgeTable, MaxTable  # noqa: E402


def say(*a):
    print(*a, flush=True)


def walks(n, moves, seed, dev):
    rng = np.random.default_rng(seed)
    env = VecCubeEnv(n, dev, 3, obs=None)
    env.reset(actions=rng.integers(0, 12, (n, moves)).astype(np.uint8))
    return env


def passes(table, log2n, steps, runs, dev):
    n = 1 << log2n
    env = VecCubeEnv(n, dev, 3, obs=None)
    env.reset(scramble_count=100)
    cub = ops.cubies(env.stickers, n, 3, status=False)["cubies"]
    fr = search.IdaFrame(table, cub, n, ops._state_arg(cub, 20, n, None, "cubies"), 20, 20)
    fr.init()
    fr.search(steps)                                                       # warm-up
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fr.search(steps)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert int(fr.running[0]) == n, "a cube ended inside the timed launches"
    med = statistics.median(ms)
    return {"cubes": n, "steps_per_launch": steps, "ms": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "runs": runs},
            "passes_per_second": round(n * steps / (med * 1e-3)), "ns_per_pass_of_one_lane": round(med * 1e6 / steps, 1),
            "ns_per_pass_over_all_lanes": round(med * 1e6 / steps / n, 5),
            "seconds_per_launch_at_ida_max_steps": round(med * 1e-3 / steps * _ida_lib.max_steps(), 3)}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ida.json"))
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cubes", type=int, default=1000)
    ap.add_argument("--budget", type=int, default=1 << 22)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--lengths", default="8,9,10,11,12,13,14")
    ap.add_argument("--split-lengths", default="10,12,13")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.init(dev)
    corner = CornerTable.build(3, dev)
    best = MaxTable(corner, EdgeTable.build(range(6), dev), EdgeTable.build(range(6, 12), dev))
    out = {"device": torch.cuda.get_device_name(dev), "arguments": {k: v for k, v in vars(a).items() if k != "out"}, "ida_max_steps": _ida_lib.max_steps(), "passes": {}, "walks": {}, "split": {}}
    for name, table in (("none", None), ("corner", corner), ("max(corner, e0-5, e6-11)", best)):
        out["passes"][name] = passes(table, a.log2n, a.steps, a.runs, dev)
        say("passes", name, json.dumps(out["passes"][name]))
    for moves in [int(x) for x in a.lengths.split(",")]:
        env = walks(a.cubes, moves, 100 + moves, dev)
        row = {}
        for rep in range(2):                                               # alternating: ida, a*, ida, a*
            ida, t_ida = timed(lambda: search.ida_search(best, env, limit=20, max_steps=a.budget))
            star, t_star = timed(lambda: search.astar_search(best, env, 1, a.iterations, front="table"))
            both = ida["solved"] & star["solved"] & ~star["overflow"]
            nodes = ida["nodes"][ida["solved"]]
            row[f"rep{rep}"] = {
                "ida": {"seconds": round(t_ida, 4), "solved_share": round(float(ida["solved"].float().mean()), 4),
                        "nodes_median_of_solved": int(nodes.median()) if nodes.numel() else None,
                        "nodes_max_of_solved": int(nodes.max()) if nodes.numel() else None,
                        "length_mean_of_solved": round(float(ida["length"][ida["solved"]].float().mean()), 3) if nodes.numel() else None,
                        "least_bound_of_unsolved": int(ida["bound"][~ida["solved"]].min()) if bool((~ida["solved"]).any()) else None},
                "astar": {"seconds": round(t_star, 4), "solved_share": round(float(star["solved"].float().mean()), 4),
                          "overflow_share": round(float(star["overflow"].float().mean()), 4), "capacity": star["capacity"]},
                "both_answered": int(both.sum()), "equal_lengths_where_both_answered": bool((ida["length"][both] == star["length"][both]).all()),
                "solved_by_ida_alone": int((ida["solved"] & ~star["solved"]).sum()), "solved_by_astar_alone": int((star["solved"] & ~ida["solved"]).sum())}
        out["walks"][str(moves)] = row
        say("walks", moves, json.dumps(row["rep1"]))
        json.dump(out, open(a.out, "w"), indent=1)
    for moves in [int(x) for x in a.split_lengths.split(",")]:
        env = walks(a.cubes, moves, 100 + moves, dev)
        row = {}
        for split in (0, 2, 0, 2):
            res, t = timed(lambda: search.ida_search(best, env, limit=20, max_steps=a.budget, split=split))
            row.setdefault(f"split{split}", []).append({"seconds": round(t, 4), "solved_share": round(float(res["solved"].float().mean()), 4)})
            row[f"lengths{split}"] = res["length"]
        same = bool((row.pop("lengths0") == row.pop("lengths2")).all())
        row["equal_lengths"] = same
        out["split"][str(moves)] = row
        say("split", moves, json.dumps(row))
        json.dump(out, open(a.out, "w"), indent=1)
    json.dump(out, open(a.out, "w"), indent=1)
    say("wrote", a.out)


if __name__ == "__main__":
    main()
