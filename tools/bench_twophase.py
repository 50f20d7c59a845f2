#!/usr/bin/env python3
"""What the two-phase solver costs and gives on one GPU (development tool; DESIGN.md "Two-phase").  Writes profiles/twophase.json (or
--out); every number is measured on the device, nothing is estimated.

    python tools/bench_twophase.py [--out profiles/twophase.json] [--log2n 20] [--sections build,passes,solve,curve,ida]

  build     TwoPhaseTables.build's loop per table (tp_build_begin, one tp_build_level per distance, the count read back per level): a
            device event pair per table, median of --builds builds after one warm-up build;
  passes    tp_phase1_search on 2^log2n cubes scrambled by 100 device moves and tp_phase2_search on 2^log2n G1 cubes after 40 phase-2
            generators: --steps passes per launch between device events, median of --runs, then ONE launch at tp_max_steps();
  solve     search.two_phase_solve at the defaults, and with candidates in --candidates, on 1000 and 2^16 cubes scrambled by 100 device
            moves, alternating with search.chain_solve in one process: a host clock around work that ends in a synchronise;
  curve     1000 cubes: candidates x max_steps x phase2_limit, what the defaults were chosen from;
  ida       the 1000 walks of 12 moves of tools/bench_ida.py: two_phase_solve's length minus ida_search's optimal length."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rubiks_cube_solver_amd import VecCubeEnv, _lib, _twophase_lib as T, ops, search  # noqa: E402
from rubiks_cube_solver_amd.pattern import MAX_LEVELS, ChainTables, CornerTable, EdgeTable, MaxTable, TwoPhaseTables  # noqa: E402


def say(*a):
    print(*a, flush=True)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": len(v)}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def build_times(dev, builds):
    L, P, sp = T.twophase_lib(), _lib.ptr, _lib.stream_ptr(dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    out = []
    for which in range(T.TABLES):
        n = T.table_bytes(which)
        table = torch.empty(n, dtype=torch.uint8, device=dev)
        totals, levels = [], None
        for b in range(builds + 1):                              # the first build is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert L.tp_build_begin(P(table), n, which, sp) == 0
            lv, empty = [1], 0
            for depth in range(MAX_LEVELS + 2):
                assert L.tp_build_level(P(table), n, which, depth, P(count), sp) == 0
                lv.append(int(count[0]))                         # the synchronisation of the real loop
                empty = empty + 1 if lv[-1] == 0 else 0
                if empty == (2 if which >= 2 else 1):
                    break
            e1.record()
            torch.cuda.synchronize()
            if b:
                totals.append(e0.elapsed_time(e1))
            levels = lv[:len(lv) - empty]
        out.append({"table": which, "bytes": n, "levels": levels, "launches": len(levels) + (2 if which >= 2 else 1), "ms": stats(totals)})
    return out


def scrambled(n, dev, seed=0):
    env = VecCubeEnv(n, dev, 3, obs=None)
    env.reset(scramble_count=100)
    return env


def g1_cubes(n, dev, generators=40, seed=7):
    """n cubes of G1: `generators` random phase-2 generators each, as quarter turns padded with the no-op."""
    gens, _ = T.generators(2)
    rng = np.random.default_rng(seed)
    pick = gens[rng.integers(0, len(gens), (n, generators))]               # [n, g, 2], 0xFF: no second action
    acts = np.where(pick == 0xFF, 12, pick).reshape(n, 2 * generators).astype(np.uint8)
    env = VecCubeEnv(n, dev, 3, obs=None)
    env.reset(actions=acts)
    return env


def passes(tp, phase, log2n, steps, runs, dev):
    n = 1 << log2n
    env = scrambled(n, dev) if phase == 1 else g1_cubes(n, dev)
    cub = ops.cubies(env.stickers, n, 3, status=False)["cubies"]
    p_c = ops._state_arg(cub, 20, n, None, "cubies")
    if phase == 1:
        fr = search.TwoPhase1Frame(tp, cub, n, p_c, 1, 32)
    else:
        pitch = _lib.pitch_for(n, 16)
        flat = torch.empty((20, pitch), dtype=torch.uint8, device=dev)
        flat[:, :n] = ops.to_aos(cub, n).T
        path = torch.full((T.MAX_DEPTH, pitch), T.NOOP, dtype=torch.uint8, device=dev)
        fr = search.TwoPhase2Frame(tp, flat, n, pitch, path, None, torch.full((pitch,), 32, dtype=torch.int32, device=dev))
    fr.init()
    started = int((fr.status[:n] == 0).sum())
    fr.search(steps)                                                       # warm-up
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fr.search(steps)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    running = int(fr.running[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fr.search(T.max_steps())
    e1.record()
    torch.cuda.synchronize()
    med = statistics.median(ms)
    return {"lanes": n, "running_at_start": started, "running_after_the_timed_launches": running, "steps_per_launch": steps,
            "ms": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "runs": runs},
            "passes_per_second": round(running * steps / (med * 1e-3)), "ns_per_pass_of_one_lane": round(med * 1e6 / steps, 1),
            "tp_max_steps": T.max_steps(), "seconds_of_one_launch_at_tp_max_steps": round(e0.elapsed_time(e1) * 1e-3, 3),
            "running_after_it": int(fr.running[0])}


def lengths(res):
    ok = res["solved"]
    ln = res["length"][ok].float()
    row = {"solved_share": round(float(ok.float().mean()), 4), "length_mean": round(float(ln.mean()), 3), "length_min": int(ln.min()),
           "length_max": int(ln.max())}
    if "source" in res:
        share = torch.bincount(res["source"][ok].long(), minlength=3).float() / max(1, int(ok.sum()))
        row["source_share"] = {"chain": round(float(share[0]), 4), "descent": round(float(share[1]), 4), "phase2": round(float(share[2]), 4)}
        row["nodes_mean"] = {"phase1": round(float(res["nodes"][0].float().mean())), "phase2": round(float(res["nodes"][1].float().mean()))}
        row["phase1_status_share"] = {str(k): round(float((res["status"] == k).float().mean()), 4) for k in (0, 1, 2, 4)}
    return row


def solve_rows(tp, chain, env, reps, **kw):
    row = {"arguments": kw or "defaults"}
    for rep in range(reps):                                                # alternating: two-phase, chain, two-phase, chain
        res, t2 = timed(lambda: search.two_phase_solve(tp, chain, env, **kw))
        ch, t1 = timed(lambda: search.chain_solve(chain, env))
        assert bool((res["length"] <= ch["length"]).all())
        row[f"rep{rep}"] = {"two_phase": dict(seconds=round(t2, 4), **lengths(res)), "chain": dict(seconds=round(t1, 5), **lengths(ch))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twophase.json"))
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--candidates", default="8,64,256")
    ap.add_argument("--sections", default="build,passes,solve,curve,ida")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.init(dev)
    sections = a.sections.split(",")
    defaults = {k: v.default for k, v in inspect.signature(search.two_phase_solve).parameters.items() if v.kind == v.KEYWORD_ONLY}
    out = {"device": torch.cuda.get_device_name(dev), "arguments": {k: v for k, v in vars(a).items() if k != "out"}, "defaults": defaults,
           "tp_max_steps": T.max_steps()}
    dump = lambda: json.dump(out, open(a.out, "w"), indent=1)
    if "build" in sections:
        out["build"] = build_times(dev, a.builds)
        say("build", json.dumps([(r["table"], r["ms"]["median"]) for r in out["build"]]))
        dump()
    tp, chain = TwoPhaseTables.build(dev), ChainTables.build(dev)
    if "passes" in sections:
        out["passes"] = {}
        for phase in (1, 2):
            out["passes"][f"phase{phase}"] = passes(tp, phase, a.log2n, a.steps, a.runs, dev)
            say("passes", phase, json.dumps(out["passes"][f"phase{phase}"]))
        dump()
    if "solve" in sections:
        out["solve"] = {}
        for n in (1000, 1 << 16):
            env = scrambled(n, dev)
            rows = {"defaults": solve_rows(tp, chain, env, 2)}
            say("solve", n, "defaults", json.dumps(rows["defaults"]["rep1"]))
            for K in [int(x) for x in a.candidates.split(",")]:
                if K != defaults["candidates"] and n * K <= 1 << 22:
                    rows[f"candidates={K}"] = solve_rows(tp, chain, env, 2, candidates=K)
                    say("solve", n, K, json.dumps(rows[f"candidates={K}"]["rep1"]["two_phase"]))
            out["solve"][str(n)] = rows
            dump()
    if "curve" in sections:
        env = scrambled(1000, dev)
        out["curve"] = []
        for K in [int(x) for x in a.candidates.split(",")]:
            for steps in (10000, 100000, 1000000):
                for p2 in (16, 20, 24):
                    if (steps == 1000000 and K > 64) or (p2 != 20 and K != 64):
                        continue
                    kw = dict(candidates=K, max_steps=steps, phase2_limit=p2)
                    res, t = timed(lambda: search.two_phase_solve(tp, chain, env, **kw))
                    out["curve"].append(dict(kw, seconds=round(t, 4), **lengths(res)))
                    say("curve", json.dumps(out["curve"][-1]))
                    dump()
    if "ida" in sections:
        rng = np.random.default_rng(112)                                    # tools/bench_ida.py walks(1000, 12, 100 + 12)
        env = VecCubeEnv(1000, dev, 3, obs=None)
        env.reset(actions=rng.integers(0, 12, (1000, 12)).astype(np.uint8))
        best = MaxTable(CornerTable.build(3, dev), EdgeTable.build(range(6), dev), EdgeTable.build(range(6, 12), dev))
        ida, t_ida = timed(lambda: search.ida_search(best, env, limit=20, max_steps=1 << 22))
        res, t_tp = timed(lambda: search.two_phase_solve(tp, chain, env))
        both = ida["solved"] & res["solved"]
        gap = (res["length"] - ida["length"])[both].float()
        out["ida"] = {"walks": 1000, "moves": 12, "ida_seconds": round(t_ida, 4), "two_phase_seconds": round(t_tp, 4), "both_answered": int(both.sum()),
                      "ida_length_mean": round(float(ida["length"][both].float().mean()), 3), "two_phase": lengths(res),
                      "length_minus_optimal": {"mean": round(float(gap.mean()), 3), "max": int(gap.max()), "min": int(gap.min()),
                                               "optimal_share": round(float((gap == 0).float().mean()), 4)}}
        say("ida", json.dumps(out["ida"]))
    dump()
    say("wrote", a.out)


if __name__ == "__main__":
    main()
