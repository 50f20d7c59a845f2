#!/usr/bin/env python3
"""What the edge pattern databases cost and buy on one GPU (development tool; DESIGN.md "Edge pattern databases").  Writes
profiles/edge.json (or --out); every number is measured on the device, nothing is estimated.

    python tools/bench_edge.py [--out profiles/edge.json] [--prove] [--log2n 20 22]

  build     EdgeTable's loop (rce_build_begin, one rce_build_level per distance, the count read back per level) for the pieces {0..5},
            {6..11} and the 7-piece set --mask7: a device event pair per level, median of --builds builds after one warm-up build;
  kernels   rce_lookup and rce_score_codes (both combine modes) beside rcp_score_keys at 2^20 and 2^22 20-move device walks, batches
            that ALTERNATE between the legs in one process, median of the batches with the range, beside their byte models.  The code
            buffer holds the A children of those walks (rc_search_expand), so the score legs cover A * n slots;
  astar     one A* iteration at 1000 cubes x B = 1024 with MaxTable(corner, e{0..5}, e{6..11}) against the CornerTable alone: two
            plans on the same roots, iterations alternating, stage by stage as tools/bench_pattern.py does;
  walks     the 500 walks each of 3, 5 and 7 moves of tests/test_gpu_pattern.py, batch 1, weight 1, under both heuristics:
            iterations and nodes (reported, never asserted: a dominating bound does not guarantee fewer expansions per instance);
  prove     (--prove) the distance proof of tests/test_gpu_edge.py over ALL indices of the three tables: |h(child) - h(parent)| <= 1,
            h > 0 => some child has h - 1, h == 0 <=> home; outcome and wall time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_beam import stats  # noqa: E402
from bench_pattern import timed  # noqa: E402
from rubiks_cube_solver_amd import VecCubeEnv, _edge_lib, _lib, _pattern_lib, ops, search  # noqa: E402
from rubiks_cube_solver_amd.pattern import MAX_LEVELS, CornerTable, EdgeTable, MaxTable  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, the figure bench.py's roofline uses
LOW6, HIGH6 = 0x03F, 0xFC0
A = 12


def build_times(mask, dev, builds):
    """-> (per-level ms samples [builds][levels], total ms samples, levels)"""
    L, P, sp = _edge_lib.edge_lib(), _lib.ptr, _lib.stream_ptr(dev)
    n = _edge_lib.table_bytes(mask)
    table = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    per_level, totals, levels = [], [], None
    for b in range(builds + 1):                                  # the first build is the warm-up
        marks, lv = [], [1]
        first = torch.cuda.Event(enable_timing=True)
        first.record()
        assert L.rce_build_begin(P(table), n, mask, sp) == 0
        for depth in range(MAX_LEVELS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert L.rce_build_level(P(table), n, mask, depth, P(count), sp) == 0
            e1.record()
            c = int(count[0])                                    # the synchronisation of the real loop
            marks.append((e0, e1))
            if c == 0:
                break
            lv.append(c)
        torch.cuda.synchronize()
        if b:
            per_level.append([x.elapsed_time(y) for x, y in marks])
            totals.append(first.elapsed_time(marks[-1][1]))
        levels = lv
    return per_level, totals, levels


def kernel_legs(log2n, corner, edge, dev, batch, batches):
    n = 1 << log2n
    E, R, sp, P = _edge_lib.edge_lib(), _pattern_lib.pattern_lib(), _lib.stream_ptr(dev), _lib.ptr
    W = 1024
    plan = search.BeamPlan(n // W, 3, W, 1, dev, front="table")
    st = plan.beams[0]                                           # n slots, tiled as a beam
    ops.fill_solved(st, n, 3)
    ops.scramble(st, n, 3, 20, seed=5)
    plan.active.fill_(1)
    plan.live.fill_(W)
    plan.last_action.fill_(A)
    plan.expand(0)                                               # the codes and keys of all A * n children
    pitch = int(st.shape[-1])
    code = ops.alloc_code(n, 3, dev, pitch)
    ops.encode(st, n, 3, code, _lib.FMT_CODE)
    dist = torch.empty(n, dtype=torch.uint8, device=dev)
    NE, NC = edge.table.numel(), corner.table.numel()
    a_code, a_tab, a_dist, a_cc, a_sc, a_keys, a_ct = P(code), P(edge.table), P(dist), P(plan.code), P(plan.scores), P(plan.keys), P(corner.table)
    legs = {"lookup": lambda: E.rce_lookup(a_code, n, pitch, edge.mask, a_tab, NE, a_dist, sp),
            "score_codes_write": lambda: E.rce_score_codes(a_cc, n // W, W, plan.pitch, edge.mask, a_tab, NE, a_sc, 0, sp),
            "score_codes_min": lambda: E.rce_score_codes(a_cc, n // W, W, plan.pitch, edge.mask, a_tab, NE, a_sc, 1, sp),
            "corner_score_keys": lambda: R.rcp_score_keys(a_keys, n // W, W, plan.pitch, 3, a_ct, NC, a_sc, sp)}
    assert all(fn() == 0 for fn in legs.values())
    for fn in legs.values():
        for _ in range(10):
            fn()
    legs["score_codes_write"]()
    torch.cuda.synchronize()
    assert int(dist.max()) <= edge.depth                          # the legs agree before they are timed:
    assert bool(((-plan.scores[:, :n] - dist.float()[None, :]).abs() <= 1).all())   # every child is at most one step from its parent
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in legs}
    for _ in range(batches):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / batch)   # us per call
    med = {k: statistics.median(v) for k, v in times.items()}
    slots = A * plan.nbp
    # bytes per call: what the rule needs, a table byte counted as ONE byte (the gather fetches a whole sector or line for it)
    model = {"lookup": n * (12 + 1 + 1), "score_codes_write": slots * (12 + 1 + 4), "score_codes_min": slots * (12 + 1 + 8),
             "corner_score_keys": slots * (24 + 1 + 4)}
    return {"mask": edge.mask, "n_states": n, "pitch": pitch, "slots": slots,
            "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "byte_model": model,
            "byte_model_us_at_8TBps": {k: round(model[k] / HBM_PEAK * 1e6, 2) for k in legs},
            "fraction_of_hbm_peak_8TBps": {k: round(model[k] / (med[k] * 1e-6) / HBM_PEAK, 3) for k in legs},
            "ns_per_slot": {k: round(med[k] * 1e3 / slots, 4) for k in legs if k != "lookup"}}


@torch.no_grad()
def astar_iteration(corner, maxtable, P, B, warmup, steps):
    env = VecCubeEnv(P, "cuda", 3, obs=None)
    env.reset(scramble_count=100)
    n = warmup + steps
    cap = 1 + B * 11 * n
    plans = {"max": (search.AStarPlan(P, 3, B, cap, env.device, front="table", weight=1.0), maxtable),
             "corner": (search.AStarPlan(P, 3, B, cap, env.device, front="table", weight=1.0), corner)}
    for plan, _ in plans.values():
        plan.init(env.stickers, env.stickers.shape[-1])
    marks = {k: [] for k in plans}
    for _ in range(n):
        for k, (plan, m) in plans.items():
            e = {}
            timed(e, "pop", plan.pop)
            timed(e, "expand", plan.expand)
            timed(e, "score", lambda: plan.score(m))
            timed(e, "merge", lambda: (plan.merge(), plan.relax(), plan.iteration.add_(1)))
            marks[k].append(e)
    torch.cuda.synchronize()
    out = {"problems": P, "batch": B, "capacity": cap, "warmup_iterations": warmup}
    for k, (plan, _) in plans.items():
        ms = {ph: [m[ph][0].elapsed_time(m[ph][1]) for m in marks[k][warmup:]] for ph in ("pop", "expand", "score", "merge")}
        whole = [m["pop"][0].elapsed_time(m["merge"][1]) for m in marks[k][warmup:]]
        out[k] = {"stage_ms": {ph: stats(v) for ph, v in ms.items()}, "iteration_ms_measured": stats(whole),
                  "nodes_per_problem_at_end": float(plan.count.float().mean())}
    out["max_over_corner_iteration"] = round(out["max"]["iteration_ms_measured"]["median"] / out["corner"]["iteration_ms_measured"]["median"], 4)
    return out


@torch.no_grad()
def walks(corner, maxtable):
    from tests.test_gpu_pattern import LIMITS_333, walks333
    out = []
    for k in sorted(LIMITS_333):
        iters, cap = LIMITS_333[k]
        env = VecCubeEnv(500, "cuda", 3, obs=None)
        env.reset(actions=walks333(k))
        rec = {"moves": k, "cubes": 500, "max_iterations": iters, "capacity": cap}
        per_cube = {}
        for name, model in (("corner", corner), ("max", maxtable)):
            torch.cuda.synchronize()
            t0 = time.time()
            res = search.astar_search(model, env, 1, iters, weight=1.0, capacity=cap, front="table", graph=k == 7, sync_every=4 if k < 7 else 128)
            torch.cuda.synchronize()
            it, nodes, length = (res[x].cpu().numpy() for x in ("iterations", "nodes", "length"))
            per_cube[name] = (it, nodes, length)
            rec[name] = {"solved": int(res["solved"].sum()), "lengths": np.bincount(length[length >= 0]).tolist(), "iterations_max": int(it.max()),
                         "iterations_sum": int(it.sum()), "nodes_max": int(nodes.max()), "nodes_sum": int(nodes.sum()), "seconds": round(time.time() - t0, 3)}
        rec["lengths_equal"] = bool((per_cube["max"][2] == per_cube["corner"][2]).all())
        rec["cubes_with_more_iterations_under_max"] = int((per_cube["max"][0] > per_cube["corner"][0]).sum())
        rec["cubes_with_more_nodes_under_max"] = int((per_cube["max"][1] > per_cube["corner"][1]).sum())
        out.append(rec)
    return out


def prove(table, chunk=1 << 22):
    """The distance proof over every index; -> dict(mask, indices, holds, seconds)."""
    N, home, dev = table.table.numel(), table.home, table.device
    torch.cuda.synchronize()
    t0, ok = time.time(), True
    for at in range(0, N, chunk):
        n = min(chunk, N - at)
        part = torch.arange(at, at + n, dtype=torch.int64, device=dev)
        st = table.states(part)
        ok = ok and not bool(ops.cubies(st, n, 3, cubies=False, status=True)["status"].any())
        code = ops.alloc_code(n, 3, dev, st.shape[-1])
        ops.encode(st, n, 3, code, _lib.FMT_CODE)
        h = table.distance(code, n).int()
        ok = ok and torch.equal(h, table.table[at:at + n].int())
        out = ops.expand_buffers(n, 3, dev, st.shape[-1], children=False, codes=True)
        ops.expand_children(st, n, 3, None, out["child_solved"], out["child_code"], pitch=st.shape[-1])
        down = torch.zeros(n, dtype=torch.bool, device=dev)
        for a in range(A):
            hc = table.distance(out["child_code"][a], n).int()
            ok = ok and bool(((hc - h).abs() <= 1).all())
            down |= hc == h - 1
        ok = ok and bool((down == (h > 0)).all()) and bool(((h == 0) == (part == home)).all())
    torch.cuda.synchronize()
    return {"mask": table.mask, "indices": N, "holds": bool(ok), "seconds": round(time.time() - t0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge.json"))
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--mask7", type=lambda s: int(s, 0), default=0xAB5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--astar-batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--prove", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edge needs a GPU: nothing is estimated"
    dev = torch.device("cuda", 0)
    _lib.init(dev)
    rec = {"command": "python tools/bench_edge.py" + (" --prove" if a.prove else ""), "device": torch.cuda.get_device_name(0),
           "timing": "device events; build: one pair per level, median over the builds after a warm-up build; kernels: batches of calls, "
                     "legs alternating batch by batch, us per call; astar: one pair per stage per iteration, plans alternating; walks: wall "
                     "time of whole searches",
           "build": [], "kernels": []}
    tables = {}
    for mask in (LOW6, HIGH6, a.mask7):
        per_level, totals, levels = build_times(mask, dev, a.builds)
        tables[mask] = EdgeTable.build(mask, dev)
        assert tables[mask].levels == tuple(levels) and sum(levels) == tables[mask].table.numel()
        rec["build"].append({"mask": mask, "pieces": list(tables[mask].edges), "table_bytes": tables[mask].table.numel(), "levels": levels,
                             "depth": tables[mask].depth, "builds": a.builds,
                             "level_ms_median": [round(statistics.median(b[d] for b in per_level), 4) for d in range(len(per_level[0]))],
                             "total_ms": stats(totals)})
        print(json.dumps(rec["build"][-1]), flush=True)
    corner = CornerTable.build(3, dev)
    maxtable = MaxTable(corner, tables[LOW6], tables[HIGH6])
    if a.prove:
        rec["prove"] = [prove(tables[m]) for m in (LOW6, HIGH6, a.mask7)]
        print(json.dumps(rec["prove"]), flush=True)
    del tables[a.mask7]
    torch.cuda.empty_cache()
    for log2n in a.log2n:
        rec["kernels"].append(kernel_legs(log2n, corner, tables[LOW6], dev, a.batch, a.batches))
        print(json.dumps(rec["kernels"][-1]), flush=True)
        torch.cuda.empty_cache()
    rec["astar_333"] = astar_iteration(corner, maxtable, a.problems, a.astar_batch, a.warmup, a.steps)
    print(json.dumps(rec["astar_333"]), flush=True)
    torch.cuda.empty_cache()
    rec["walks_333"] = walks(corner, maxtable)
    print(json.dumps(rec["walks_333"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
