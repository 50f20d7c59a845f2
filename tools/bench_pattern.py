#!/usr/bin/env python3
"""What the corner pattern database costs on one GPU (development tool; DESIGN.md "Corner pattern database").  Writes
profiles/pattern.json (or --out); every number is measured on the device, nothing is estimated.

    python tools/bench_pattern.py [--out profiles/pattern.json] [--prove] [--log2n 20 22]

  build     CornerTable's loop (rcp_build_begin, one rcp_build_level per distance, the count read back per level), both sizes: a device
            event pair per level, median of --builds builds after one warm-up build; the total is begin-to-last-level of one build;
  kernels   rcp_lookup and rcp_score_keys against rcc_cubies(corner_index alone) at 2^20 and 2^22 20-move device walks, batches that
            ALTERNATE between the legs in one process (tools/bench_cubies.py's method), median of the batches, beside their byte models.
            The key array holds the A children of those walks (rc_search_expand), so rcp_score_keys scores A * n slots;
  astar     one A* iteration at 1000 cubes x B = 1024 on the 3x3x3 with front="table" against the dense net front (random-init DeepCube
            [1024, 256, 128] fp32): two plans on the same roots, iterations alternating, stage by stage as tools/bench_astar.py does
            (the table plan's merge stage includes rcp_relax, as AStarPlan.step runs it);
  optimal   the exact distances of tests/golden/crosscheck_222.npz's scrambles: mean optimal length per scramble depth (README);
  prove     (--prove) the distance proof of tests/test_gpu_pattern.py over ALL indices of both tables: |h(child) - h(parent)| = 1,
            h > 0 => some child has h - 1, h == 0 <=> index 0; outcome and wall time."""
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

from bench_beam import DeepCubeStandIn, stats  # noqa: E402
from rubiks_cube_solver_amd import VecCubeEnv, _cubie_lib, _lib, _pattern_lib, ops, search  # noqa: E402
from rubiks_cube_solver_amd.pattern import MAX_LEVELS, CornerTable  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, the figure bench.py's roofline uses
S_OF, A_OF, KW_OF = {2: 24, 3: 54}, {2: 6, 3: 12}, {2: 2, 3: 3}
CORNER_ROWS = {2: 24, 3: 24}            # sticker rows rcp_lookup reads: 7 x 3 + the 3 fixed ones | 8 x 3


def build_times(cs, dev, builds):
    """-> (per-level ms samples [builds][levels], total ms samples, levels)"""
    L, P, sp = _pattern_lib.pattern_lib(), _lib.ptr, _lib.stream_ptr(dev)
    n = _pattern_lib.table_bytes(cs)
    table = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    per_level, totals, levels = [], [], None
    for b in range(builds + 1):                                  # the first build is the warm-up
        marks, lv = [], [1]
        first = torch.cuda.Event(enable_timing=True)
        first.record()
        assert L.rcp_build_begin(P(table), n, cs, sp) == 0
        for depth in range(MAX_LEVELS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert L.rcp_build_level(P(table), n, cs, depth, P(count), sp) == 0
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


def kernel_legs(cs, log2n, table, dev, batch, batches):
    n, S, A, KW = 1 << log2n, S_OF[cs], A_OF[cs], KW_OF[cs]
    L, C, sp, P = _pattern_lib.pattern_lib(), _cubie_lib.cubie_lib(), _lib.stream_ptr(dev), _lib.ptr
    W = 1024
    plan = search.BeamPlan(n // W, cs, W, 1, dev, front="table")
    st = plan.beams[0]                                           # n slots, tiled as a beam
    ops.fill_solved(st, n, cs)
    ops.scramble(st, n, cs, 20, seed=5)
    plan.active.fill_(1)
    plan.live.fill_(W)
    plan.last_action.fill_(A)
    plan.expand(0)                                               # the keys of all A * n children
    pitch = int(st.shape[-1])
    dist = torch.empty(n, dtype=torch.uint8, device=dev)
    ci = torch.empty(n, dtype=torch.int32, device=dev)
    N = table.table.numel()
    a_st, a_tab, a_dist, a_ci, a_keys, a_sc = P(st), P(table.table), P(dist), P(ci), P(plan.keys), P(plan.scores)
    legs = {"cubies_index": lambda: C.rcc_cubies(a_st, n, pitch, cs, None, 0, None, a_ci, None, sp),
            "lookup": lambda: L.rcp_lookup(a_st, n, pitch, cs, a_tab, N, a_dist, sp),
            "score_keys": lambda: L.rcp_score_keys(a_keys, n // W, W, plan.pitch, cs, a_tab, N, a_sc, sp)}
    assert all(fn() == 0 for fn in legs.values())
    for fn in legs.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(dist, table.table[ci.long()]) and int(dist.max()) <= 14            # the legs agree before they are timed
    assert bool(((-plan.scores[:, :n] - dist.float()[None, :]).abs() == 1).all())           # every child is one step from its parent
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
    model = {"cubies_index": n * (S + 4), "lookup": n * (CORNER_ROWS[cs] + 1 + 1), "score_keys": slots * (8 * KW + 1 + 4)}
    return {"cube_size": cs, "n_states": n, "pitch": pitch, "key_slots": slots,
            "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "byte_model": model,
            "byte_model_us_at_8TBps": {k: round(model[k] / HBM_PEAK * 1e6, 2) for k in legs},
            "fraction_of_hbm_peak_8TBps": {k: round(model[k] / (med[k] * 1e-6) / HBM_PEAK, 3) for k in legs},
            "lookup_over_cubies_index": round(med["lookup"] / med["cubies_index"], 3),
            "ns_per_key_slot": round(med["score_keys"] * 1e3 / slots, 4)}


def timed(e, key, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    e[key] = (a, b)


@torch.no_grad()
def astar_iteration(table, P, B, warmup, steps):
    torch.manual_seed(0)
    model = DeepCubeStandIn().cuda().eval()
    env = VecCubeEnv(P, "cuda", 3, obs=None)
    env.reset(scramble_count=100)
    n = warmup + steps
    cap = 1 + B * 11 * n
    plans = {"table": (search.AStarPlan(P, 3, B, cap, env.device, front="table", weight=1.0), table),
             "dense": (search.AStarPlan(P, 3, B, cap, env.device, torch.float32, weight=1.0), model)}
    for plan, _ in plans.values():
        plan.init(env.stickers, env.stickers.shape[-1])
    marks = {k: [] for k in plans}
    for _ in range(n):
        for k, (plan, m) in plans.items():
            e = {}
            timed(e, "pop", plan.pop)
            timed(e, "expand", plan.expand)
            timed(e, "score", lambda: plan.score(m))
            timed(e, "merge", lambda: (plan.merge(), plan.relax() if k == "table" else None, plan.iteration.add_(1)))   # table: + rcp_relax
            marks[k].append(e)
    torch.cuda.synchronize()
    out = {"problems": P, "batch": B, "capacity": cap, "warmup_iterations": warmup}
    for k, (plan, _) in plans.items():
        ms = {ph: [m[ph][0].elapsed_time(m[ph][1]) for m in marks[k][warmup:]] for ph in ("pop", "expand", "score", "merge")}
        whole = [m["pop"][0].elapsed_time(m["merge"][1]) for m in marks[k][warmup:]]
        out[k] = {"stage_ms": {ph: stats(v) for ph, v in ms.items()}, "iteration_ms_measured": stats(whole),
                  "nodes_per_problem_at_end": float(plan.count.float().mean()), "popped_per_problem_last": float(plan.beam.live.float().mean())}
    out["table_over_dense_iteration"] = round(out["table"]["iteration_ms_measured"]["median"] / out["dense"]["iteration_ms_measured"]["median"], 5)
    return out


def optimal_222(table):
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    env = VecCubeEnv(len(g["ks"]), "cuda", 2, obs=None)
    env.reset(actions=g["scramble"].astype(np.uint8))
    d = env.corner_distance(table).cpu().numpy()
    res = search.astar_search(table, env, 1, 16, weight=1.0, front="table")
    assert (res["length"].cpu().numpy() == d).all()
    return [{"k": int(k), "mean_optimal_length": round(float(d[g["ks"] == k].mean()), 3), "max": int(d[g["ks"] == k].max()),
             "cubes": int((g["ks"] == k).sum())} for k in g["depths"]]


def prove(table, chunk=1 << 22):
    """The distance proof over every index; -> dict(ok, seconds)."""
    cs, A, N = table.cube_size, A_OF[table.cube_size], table.table.numel()
    torch.cuda.synchronize()
    t0, ok = time.time(), True
    for at in range(0, N, chunk):
        n = min(chunk, N - at)
        part = torch.arange(at, at + n, dtype=torch.int64, device=table.device)
        st = table.states(part)
        h = table.distance(st, n).int()
        ok = ok and torch.equal(h, table.table[at:at + n].int())
        out = ops.expand_buffers(n, cs, table.device, st.shape[-1], children=True, codes=False)
        ops.expand_children(st, n, cs, out["children"], out["child_solved"], None, pitch=st.shape[-1])
        down = torch.zeros(n, dtype=torch.bool, device=table.device)
        for a in range(A):
            hc = table.distance(out["children"][a], n).int()
            ok = ok and bool(((hc - h).abs() == 1).all())
            down |= hc == h - 1
        ok = ok and bool((down == (h > 0)).all()) and bool(((h == 0) == (part == 0)).all())
    torch.cuda.synchronize()
    return {"cube_size": cs, "indices": N, "holds": bool(ok), "seconds": round(time.time() - t0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern.json"))
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--astar-batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--prove", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pattern needs a GPU: nothing is estimated"
    dev = torch.device("cuda", 0)
    _lib.init(dev)
    rec = {"command": "python tools/bench_pattern.py" + (" --prove" if a.prove else ""), "device": torch.cuda.get_device_name(0),
           "timing": "device events; build: one pair per level, median over the builds after a warm-up build; kernels: batches of calls, "
                     "legs alternating batch by batch, us per call; astar: one pair per stage per iteration, plans alternating",
           "build": [], "kernels": []}
    tables = {}
    for cs in (2, 3):
        per_level, totals, levels = build_times(cs, dev, a.builds)
        tables[cs] = CornerTable.build(cs, dev)
        assert tables[cs].levels == tuple(levels)
        rec["build"].append({"cube_size": cs, "table_bytes": tables[cs].table.numel(), "levels": levels, "builds": a.builds,
                             "level_ms_median": [round(statistics.median(b[d] for b in per_level), 4) for d in range(len(per_level[0]))],
                             "total_ms": stats(totals)})
        print(json.dumps(rec["build"][-1]), flush=True)
    for cs in (3, 2):
        for log2n in a.log2n:
            rec["kernels"].append(kernel_legs(cs, log2n, tables[cs], dev, a.batch, a.batches))
            print(json.dumps(rec["kernels"][-1]), flush=True)
            torch.cuda.empty_cache()
    rec["astar_333"] = astar_iteration(tables[3], a.problems, a.astar_batch, a.warmup, a.steps)
    print(json.dumps(rec["astar_333"]), flush=True)
    torch.cuda.empty_cache()
    rec["optimal_222"] = optimal_222(tables[2])
    print(json.dumps(rec["optimal_222"]), flush=True)
    if a.prove:
        rec["prove"] = [prove(tables[cs]) for cs in (2, 3)]
        print(json.dumps(rec["prove"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
