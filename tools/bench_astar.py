#!/usr/bin/env python3
"""Batch-weighted A* benchmark (rubiks-cube-solver_amd/search.py astar_search, DESIGN.md "A* search").  Writes
profiles/astar_search.json (or --out), two parts:

  timing   3x3x3, P = 1000 cubes, B = 1024, random-init DeepCube [1024, 256, 128] fp32, dense front: time per iteration split into pop /
           expand / score / merge with a device-event pair around each stage, after warm-up iterations that fill the batch (iteration t
           pops min(B, 11^(t-1)-ish) nodes: the fourth is the first full one).  In the same process, alternating iteration by depth,
           beam_search's step at W = 1024 split into expand / score / select / advance.
  rates    2x2x2, the shipped checkpoint on tests/golden/crosscheck_222.npz's scrambles: solve rate and mean solution length per
           scramble depth for A* at B = 16, weight 1.0 and 0.6, beside the beam at W = 16; the net rows that belong to live nodes
           (rows_live) and the rows the net was run on (rows_scored: every slot of the batch is scored, live or not).

The statement to check: pop + merge stay a small share of an iteration beside the net, as the beam's expand + select + advance do."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_beam import DeepCubeStandIn, stats
from rubiks_cube_solver_amd import VecCubeEnv, search
from rubiks_cube_solver_amd.adi import _module_dtype

A_PHASES = ("pop", "expand", "score", "merge")
B_PHASES = ("expand", "score", "select", "advance")


def timed(e, key, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    e[key] = (a, b)


@torch.no_grad()
def timing(P, B, warmup, steps, dtype=torch.float32):
    torch.manual_seed(0)
    model = DeepCubeStandIn().cuda().to(dtype).eval()
    env = VecCubeEnv(P, "cuda", 3, obs=None)
    env.reset(scramble_count=100)
    n = warmup + steps
    cap = 1 + B * 11 * n
    ap = search.AStarPlan(P, 3, B, cap, env.device, _module_dtype(model), weight=1.0)
    bp = search.BeamPlan(P, 3, B, n, env.device, _module_dtype(model))
    ap.init(env.stickers, env.stickers.shape[-1])
    bp.init(env.stickers, env.stickers.shape[-1])
    am, bm, popped = [], [], []
    for t in range(1, n + 1):
        e = {}
        timed(e, "pop", ap.pop)
        popped.append(ap.beam.live.sum())
        timed(e, "expand", ap.expand)
        timed(e, "score", lambda: ap.score(model))
        timed(e, "merge", lambda: (ap.merge(), ap.iteration.add_(1)))
        am.append(e)
        e, parity = {}, (t - 1) & 1
        timed(e, "expand", lambda: bp.expand(parity))
        timed(e, "score", lambda: bp.score(model))
        timed(e, "select", bp.select)
        timed(e, "advance", lambda: (bp.advance(parity), bp.depth.add_(1)))
        bm.append(e)
    torch.cuda.synchronize()
    ms = lambda marks, phases: {k: [m[k][0].elapsed_time(m[k][1]) for m in marks[warmup:]] for k in phases}
    a, b = ms(am, A_PHASES), ms(bm, B_PHASES)
    med = lambda d: {k: float(np.median(v)) for k, v in d.items()}
    a_med, b_med = med(a), med(b)
    a_total, b_total = sum(a_med.values()), sum(b_med.values())      # sums of the stage medians: what the shares below divide by
    # the whole iteration / depth, measured: first event of its first stage to last event of its last stage
    whole = lambda marks, first, last: [m[first][0].elapsed_time(m[last][1]) for m in marks[warmup:]]
    a_whole, b_whole = whole(am, "pop", "merge"), whole(bm, "expand", "advance")
    count = ap.count.cpu().numpy()
    S, KW = ap.S, ap.keys.shape[0]
    node_bytes = S + 8 * KW + 4 + 1 + 4 + 4 + 4 + 1
    nodes = float(count.mean())
    # bytes per iteration and problem (DESIGN.md "A* search"): pop scans state + prio of every node per pass (open count, up to 8 radix
    # passes, compaction) and gathers B nodes; merge reads flags + keys + one scratch slot + one table slot per candidate, the score of
    # the new ones, and writes a node and a table slot for each
    cands = B * ap.A
    model_bytes = {"pop_scan_per_pass": nodes * 5, "pop_gather": B * (2 * S + 4 + 2),
                   "merge_read": cands * (1 + 8 * KW + 8 + 8) + B * 8, "merge_write_max": B * (ap.A - 1) * (node_bytes + 8 + 1)}
    return {
        "problems": P, "batch": B, "width": B, "capacity": cap, "dtype": str(dtype).replace("torch.", ""), "warmup_iterations": warmup,
        "popped_per_problem": [round(float(x) / P, 2) for x in popped], "nodes_per_problem_at_end": nodes,
        "pool_bytes_per_node": node_bytes, "table_bytes_per_node": ap.table.numel() / (P * cap),
        "astar_ms": {k: stats(v) for k, v in a.items()}, "beam_ms": {k: stats(v) for k, v in b.items()},
        "astar_iteration_ms_sum_of_stage_medians": round(a_total, 3), "beam_depth_ms_sum_of_stage_medians": round(b_total, 3),
        "astar_iteration_ms_measured": stats(a_whole), "beam_depth_ms_measured": stats(b_whole),
        "astar_pop_plus_merge_ms": round(a_med["pop"] + a_med["merge"], 3),
        "astar_pop_plus_merge_share": round((a_med["pop"] + a_med["merge"]) / a_total, 5),
        "astar_bookkeeping_share_with_expand": round((a_med["pop"] + a_med["merge"] + a_med["expand"]) / a_total, 5),
        "beam_expand_select_advance_ms": round(b_med["expand"] + b_med["select"] + b_med["advance"], 3),
        "beam_search_kernels_share": round((b_med["expand"] + b_med["select"] + b_med["advance"]) / b_total, 5),
        "byte_model_per_problem": {k: round(v) for k, v in model_bytes.items()},
        "overflowed_problems": int(ap.overflow.sum()),
    }


@torch.no_grad()
def run_astar(model, env, B, max_iterations, weight):
    """search.astar_search's loop, counting net rows on the device."""
    P, cs = env.num_envs, env.cube_size
    cap = search.astar_capacity(P, cs, B, max_iterations)
    plan = search.AStarPlan(P, cs, B, cap, env.device, _module_dtype(model), weight=weight)
    plan.init(env.stickers, env.stickers.shape[-1])
    live = torch.zeros((), dtype=torch.int64, device=env.device)
    scored = 0
    for t in range(1, max_iterations + 1):
        plan.pop()
        live += (plan.beam.live * plan.beam.active).sum()
        plan.expand(); plan.score(model); plan.merge(); plan.iteration.add_(1)
        scored += plan.A * plan.beam.nbp
        if t % 4 == 0 and not bool(plan.beam.active.any()):
            break
    return plan.beam.length.cpu().numpy(), int(live) * plan.A, scored, plan.overflow.cpu().numpy()


@torch.no_grad()
def run_beam(model, env, W, max_depth):
    plan = search.BeamPlan(env.num_envs, env.cube_size, W, max_depth, env.device, _module_dtype(model))
    plan.init(env.stickers, env.stickers.shape[-1])
    live = torch.zeros((), dtype=torch.int64, device=env.device)
    scored = 0
    for t in range(1, max_depth + 1):
        live += (plan.live * plan.active).sum()
        plan.step(model, (t - 1) & 1)
        scored += plan.A * plan.nbp
        if t % 4 == 0 and not bool(plan.active.any()):
            break
    return plan.length.cpu().numpy(), int(live) * plan.A, scored


def rates(max_iterations):
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        sd = {k: z[k] for k in z.files}
    model = DeepCubeStandIn((7, 21), sd=sd).cuda().eval()
    env = VecCubeEnv(len(g["ks"]), "cuda", 2, obs=None)
    env.reset(actions=g["scramble"].astype(np.uint8))
    runs = {}
    for w in (1.0, 0.6):
        length, live, scored, over = run_astar(model, env, 16, max_iterations, w)
        runs[f"astar_b16_w{w}"] = dict(length=length, rows_live=live, rows_scored=scored, overflowed=int(over.sum()))
    length, live, scored = run_beam(model, env, 16, 30)
    runs["beam_w16"] = dict(length=length, rows_live=live, rows_scored=scored)
    out = {"max_iterations": max_iterations, "per_depth": [], "totals": {}}
    for name, r in runs.items():
        solved = r["length"] >= 0
        out["totals"][name] = {k: v for k, v in r.items() if k != "length"} | {
            "solved_fraction": round(float(solved.mean()), 4), "mean_length": round(float(r["length"][solved].mean()), 3)}
    for di, k in enumerate(g["depths"]):
        m = g["ks"] == k
        row = {"k": int(k), "greedy": float(g["greedy_rate"][0, di])}
        for name, r in runs.items():
            s = r["length"][m] >= 0
            row[name] = float(s.mean())
            row[name + "_mean_length"] = round(float(r["length"][m][s].mean()), 3) if s.any() else None
        out["per_depth"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "astar_search.json"))
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    args = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0),
           "method": "device events, one pair per stage per iteration; A* iterations and beam depths alternate in one process; medians of --steps "
                     "samples after --warmup iterations"}
    rec["timing_333"] = timing(args.problems, args.batch, args.warmup, args.steps)
    print(json.dumps({"timing_333": rec["timing_333"]}), flush=True)
    rec["rates_222"] = rates(args.max_iterations)
    print(json.dumps({"rates_222": rec["rates_222"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
