#!/usr/bin/env python3
"""Beam search benchmark (rubiks-cube-solver_amd/search.py): per-depth time split into expand / one-hot / net / select / advance,
and the 2x2x2 solve rates of the shipped checkpoint at W = 16 next to the greedy and MCTS rates recorded in
tests/golden/crosscheck_222.npz.  Writes profiles/beam_search.json (or --out).

  3x3x3  P = 1000, W = 1024, D = 30, random-init DeepCube [1024, 256, 128], fp32 and bf16 (nothing gets solved: all 30 depths run)
  2x2x2  the shipped checkpoint, P = 10000 scrambles of depth 14, W = 16, D = 30

--front {dense,codes,both} (default dense: the record above, unchanged) measures the net front (DESIGN.md "Net front") instead and
writes profiles/beam_search_front.json: per depth, the median of whole plan.step() calls for front="dense" and front="codes" in ONE
process, alternating; the split first layer / rest of the net / one-hot / search kernels; and rc_net_first_layer alone on every
candidate of a depth against its two bounds (LDS reads, HBM writes).

Phases are timed with device events around each launch group of every depth (the net and the one-hot writer alternate per chunk:
their events are summed).  Kernel names for `rocprofv3 --kernel-trace --stats` (run it separately, --quick): k_expand, k_insert,
k_select, k_advance (librubiksearch.so), k_code_to_dense* (librubikhip.so), the GEMMs of the net."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from rubiks_cube_solver_amd import VecCubeEnv, search
from rubiks_cube_solver_amd.adi import _module_dtype

HBM_PEAK = 8.0e12          # bytes/s (spec)
FP32_PEAK, BF16_PEAK = 157.3e12, 2.5e15   # dense FLOP/s (spec)
PHASES = ("expand", "onehot", "net", "select", "advance")


class DeepCubeStandIn(torch.nn.Module):
    """model.py:7-45's architecture (config.yaml hidden_dim [1024, 256, 128]), random init; or the shapes of a state dict."""

    def __init__(self, state_dim=(20, 24), action_dim=12, hidden=(1024, 256, 128), sd=None):
        super().__init__()
        nn = torch.nn
        if sd is not None:
            hidden = (sd["encoder_net.1.weight"].shape[0], sd["encoder_net.3.weight"].shape[0], sd["value_net.0.weight"].shape[0])
            action_dim = sd["policy_net.2.weight"].shape[0]
        d = state_dim[0] * state_dim[1]
        self.encoder_net = nn.Sequential(nn.Flatten(), nn.Linear(d, hidden[0]), nn.ELU(), nn.Linear(hidden[0], hidden[1]), nn.ELU())
        self.policy_net = nn.Sequential(nn.Linear(hidden[1], hidden[2]), nn.ELU(), nn.Linear(hidden[2], action_dim))
        self.value_net = nn.Sequential(nn.Linear(hidden[1], hidden[2]), nn.ELU(), nn.Linear(hidden[2], 1))
        if sd is not None:
            self.load_state_dict({k: torch.tensor(v) for k, v in sd.items() if k.split(".")[0] in ("encoder_net", "policy_net", "value_net")})

    def forward(self, x):
        h = self.encoder_net(x)
        return self.value_net(h), self.policy_net(h)


def net_flops(model, rows):
    return 2 * rows * sum(m.in_features * m.out_features for m in model.modules() if isinstance(m, torch.nn.Linear))


@torch.no_grad()
def timed_search(model, env, width, max_depth, sync_every=4):
    """search.beam_search's loop with device events around each phase of each depth -> (result dict, per-depth ms per phase)."""
    plan = search.BeamPlan(env.num_envs, env.cube_size, width, max_depth, env.device, _module_dtype(model))
    plan.init(env.stickers, env.stickers.shape[-1])
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = []
    t0 = time.perf_counter()
    for t in range(1, plan.D + 1):
        parity = (t - 1) & 1
        e = {k: [] for k in PHASES}
        a, b = ev(), ev(); a.record(); plan.expand(parity); b.record(); e["expand"].append((a, b))
        total, flat = plan.A * plan.nbp, plan.scores.view(-1)
        for j0 in range(0, total, plan.chunk):
            m = min(plan.chunk, total - j0)
            t0c = j0 // plan.pitch
            a, b = ev(), ev(); a.record()
            search.ops.onehot_from_code(plan.code[t0c:t0c + m // plan.pitch], m, plan.cs, plan.dense[:m])
            b.record(); e["onehot"].append((a, b))
            a, b = ev(), ev(); a.record()
            flat[j0:j0 + m].copy_(model(plan.dense[:m])[0][:, 0])
            b.record(); e["net"].append((a, b))
        a, b = ev(), ev(); a.record(); plan.select(); b.record(); e["select"].append((a, b))
        a, b = ev(), ev(); a.record(); plan.advance(parity); plan.depth.add_(1); b.record(); e["advance"].append((a, b))
        marks.append(e)
        if t % sync_every == 0 and not bool(plan.active.any()):
            break
    plan.backtrack()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    per_depth = [{k: sum(x.elapsed_time(y) for x, y in e[k]) for k in PHASES} for e in marks]
    return plan, per_depth, wall


def summarize(plan, model, per_depth, wall, dtype):
    A, nbp, P = plan.A, plan.nbp, plan.P
    cands = A * nbp
    mean = {k: float(np.mean([d[k] for d in per_depth])) for k in PHASES}
    depth_ms = sum(mean.values())
    kw = plan.keys.shape[0]
    search_ms = mean["expand"] + mean["select"] + mean["advance"]
    flops = net_flops(model, cands)
    peak = FP32_PEAK if dtype == torch.float32 else BF16_PEAK
    # bytes each search kernel must move at least, per candidate / per slot (DESIGN.md "Beam search")
    select_b = 1 + 8 * kw + 8 + 4                   # flags, key, one table slot, score: each read once
    expand_b = (plan.S + A * (plan.SL + 1 + 8 * kw)) / A   # parent stickers read, code + flags + key written, per candidate
    advance_b = 2 * plan.S + 4                      # parent gathered, child written, parent / action / history per slot (per slot)
    rec = {
        "problems": P, "width": plan.W, "max_depth": plan.D, "depths_run": len(per_depth), "candidates_per_depth": cands,
        "dtype": str(dtype).replace("torch.", ""), "dense_chunk_rows": plan.chunk,
        "per_depth_ms_mean": {k: round(v, 3) for k, v in mean.items()}, "per_depth_ms_total": round(depth_ms, 3),
        "per_depth_ms": [{k: round(v, 3) for k, v in d.items()} for d in per_depth],
        "wall_s": round(wall, 3),
        "search_kernels_share": round(search_ms / depth_ms, 4),
        "net_tflop_per_depth": round(flops / 1e12, 3), "net_tflops": round(flops / (mean["net"] * 1e-3) / 1e12, 2),
        "net_frac_of_peak": round(flops / (mean["net"] * 1e-3) / peak, 3),
        "roofline": {
            "expand_bytes_per_candidate": round(expand_b, 2), "expand_frac_hbm": round(cands * expand_b / (mean["expand"] * 1e-3) / HBM_PEAK, 3),
            "select_bytes_per_candidate_min": select_b, "select_frac_hbm": round(cands * select_b / (mean["select"] * 1e-3) / HBM_PEAK, 3),
            "advance_bytes_per_slot": advance_b, "advance_frac_hbm": round(nbp * advance_b / (mean["advance"] * 1e-3) / HBM_PEAK, 3),
            "onehot_bytes_per_candidate": plan.R * plan.C * plan.dense.element_size(),
            "onehot_frac_hbm": round(cands * plan.R * plan.C * plan.dense.element_size() / (mean["onehot"] * 1e-3) / HBM_PEAK, 3),
        },
        "solved": int((plan.length >= 0).sum()),
    }
    over = {k: round(mean[k] / depth_ms, 4) for k in ("expand", "select", "advance") if mean[k] / depth_ms > 0.10}
    if over:
        rec["search_kernel_over_10pct"] = over
    return rec


# ----------------------------------------------------------------------------------------------- --front
FRONT_PHASES = ("expand", "onehot", "first_layer", "rest_of_net", "select", "advance")
LDS_BYTES_PER_CLK_CU, N_CU, CLOCK_HZ = 256, 256, 2.4e9     # ds_read_b128: 256 B/clk/CU; 256 CUs; ~2.4 GHz (about 150 TB/s chip-wide)
HBM_ACHIEVABLE = 6.3e12                                     # bytes/s a streaming kernel reaches (8.0e12 is the spec)


def stats(ms):
    a = np.asarray(ms, np.float64)
    return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "samples": len(a)}


@torch.no_grad()
def step_times(model, env, width, fronts, warmup=2, steps=9):
    """Whole depth steps (plan.step: expand, score, select, advance, no host work in between), one event pair per step; the fronts
    alternate depth by depth on plans of their own so that both see the same machine.  -> {front: [ms per step]}"""
    plans = {}
    for f in fronts:
        kw = dict(front="codes", hidden=model.encoder_net[1].out_features) if f == "codes" else {}
        plans[f] = search.BeamPlan(env.num_envs, env.cube_size, width, warmup + steps, env.device, _module_dtype(model), **kw)
        plans[f].init(env.stickers, env.stickers.shape[-1])
    marks = {f: [] for f in fronts}
    for t in range(1, warmup + steps + 1):
        for f in fronts:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); plans[f].step(model, (t - 1) & 1); b.record()
            marks[f].append((a, b))
    torch.cuda.synchronize()
    out = {f: [x.elapsed_time(y) for x, y in marks[f][warmup:]] for f in fronts}
    return out, {f: int((plans[f].length >= 0).sum()) for f in fronts}


@torch.no_grad()
def split_times(model, env, width, front, warmup=2, steps=7):
    """The same depth step with an event pair around every launch group -> median ms per phase.  front="dense": the first layer is
    encoder_net[:3] on the dense one-hot and the rest is what model() does behind it (both heads); front="codes": rc_net_first_layer
    and CodeNet.value_codes' tail (the value head only)."""
    from rubiks_cube_solver_amd.codenet import CodeNet
    D = warmup + steps
    kw = dict(front="codes", hidden=model.encoder_net[1].out_features) if front == "codes" else {}
    plan = search.BeamPlan(env.num_envs, env.cube_size, width, D, env.device, _module_dtype(model), **kw)
    plan.init(env.stickers, env.stickers.shape[-1])
    net = CodeNet(model) if front == "codes" else None
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = []

    def timed(e, key, fn):
        a, b = ev(), ev()
        a.record(); r = fn(); b.record()
        e[key].append((a, b))
        return r

    for t in range(1, D + 1):
        parity = (t - 1) & 1
        e = {k: [] for k in FRONT_PHASES}
        timed(e, "expand", lambda: plan.expand(parity))
        total, flat = plan.A * plan.nbp, plan.scores.view(-1)
        for j0 in range(0, total, plan.chunk):
            m = min(plan.chunk, total - j0)
            code = plan.code[j0 // plan.pitch:(j0 + m) // plan.pitch]
            if front == "codes":
                h = timed(e, "first_layer", lambda: net.hidden_codes(code, m, plan.hidden))
                timed(e, "rest_of_net", lambda: flat[j0:j0 + m].copy_(model.value_net(net.tail(h))[:, 0]))
            else:
                timed(e, "onehot", lambda: search.ops.onehot_from_code(code, m, plan.cs, plan.dense[:m]))
                h = timed(e, "first_layer", lambda: model.encoder_net[:3](plan.dense[:m]))

                def rest():
                    x = model.encoder_net[3:](h)
                    model.policy_net(x)
                    flat[j0:j0 + m].copy_(model.value_net(x)[:, 0])
                timed(e, "rest_of_net", rest)
        timed(e, "select", plan.select)
        timed(e, "advance", lambda: (plan.advance(parity), plan.depth.add_(1)))
        marks.append(e)
    torch.cuda.synchronize()
    per_depth = [{k: sum(x.elapsed_time(y) for x, y in e[k]) for k in FRONT_PHASES} for e in marks[warmup:]]
    return {k: round(float(np.median([d[k] for d in per_depth])), 3) for k in FRONT_PHASES}, plan.chunk


@torch.no_grad()
def kernel_alone(model, env, width, reps=7):
    """rc_net_first_layer on every candidate of one depth, ONE launch into an [n, H1] buffer, against the two bounds of the issue:
    the table rows read from LDS and the output written to HBM."""
    from rubiks_cube_solver_amd.codenet import CodeNet
    net = CodeNet(model)
    plan = search.BeamPlan(env.num_envs, env.cube_size, width, 1, env.device, _module_dtype(model), front="codes", hidden=net.hidden,
                           dense_budget_bytes=1 << 20)
    plan.init(env.stickers, env.stickers.shape[-1])
    plan.expand(0)
    n = plan.A * plan.nbp
    try:
        out = torch.empty((n, net.hidden), dtype=net.dtype, device=env.device)
    except torch.OutOfMemoryError:                             # 51.5 GB in fp32 at 12.6 M x 1024: a quarter of the states, recorded as such
        n = n // 4 // plan.pitch * plan.pitch
        out = torch.empty((n, net.hidden), dtype=net.dtype, device=env.device)
    ms = []
    for i in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); net.hidden_codes(plan.code, n, out); b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    esz = out.element_size()
    lds_bytes, hbm_bytes = n * plan.SL * net.hidden * 4, n * net.hidden * esz      # the slab is fp32 in LDS whatever the weight's format
    lds_ms = lds_bytes / (LDS_BYTES_PER_CLK_CU * N_CU * CLOCK_HZ) * 1e3
    hbm_ms, hbm_spec_ms = hbm_bytes / HBM_ACHIEVABLE * 1e3, hbm_bytes / HBM_PEAK * 1e3
    med = float(np.median(ms))
    bound = max(lds_ms, hbm_ms)
    return {"states": n, "hidden": net.hidden, "ms": stats(ms), "lds_read_bytes": lds_bytes, "hbm_write_bytes": hbm_bytes,
            "bound_lds_reads_ms": round(lds_ms, 3), "bound_hbm_writes_ms": round(hbm_ms, 3), "bound_hbm_writes_at_spec_ms": round(hbm_spec_ms, 3),
            "binding_bound": "hbm_writes" if hbm_ms >= lds_ms else "lds_reads", "time_over_binding_bound": round(med / bound, 3),
            "achieved_write_TBps": round(hbm_bytes / (med * 1e-3) / 1e12, 3), "achieved_lds_read_TBps": round(lds_bytes / (med * 1e-3) / 1e12, 2),
            "constants": {"lds_bytes_per_clk_per_cu": LDS_BYTES_PER_CLK_CU, "cus": N_CU, "clock_hz": CLOCK_HZ, "hbm_achievable_Bps": HBM_ACHIEVABLE,
                          "hbm_spec_Bps": HBM_PEAK}}


def front_case(model, env, width, fronts, alone=True):
    times, solved = step_times(model, env, width, fronts)
    rec = {"problems": env.num_envs, "width": width, "dtype": rec_name(_module_dtype(model)), "hidden": [m.out_features for m in model.encoder_net if isinstance(m, torch.nn.Linear)],
           "per_depth_ms": {f: stats(v) for f, v in times.items()}, "per_depth_ms_samples": {f: [round(x, 3) for x in v] for f, v in times.items()},
           "solved_after_timed_steps": solved, "split_ms_median": {}}
    for f in fronts:
        rec["split_ms_median"][f], chunk = split_times(model, env, width, f)
        rec.setdefault("chunk_rows", {})[f] = chunk
    if len(fronts) == 2:
        d, c = rec["per_depth_ms"]["dense"], rec["per_depth_ms"]["codes"]
        rec["codes_over_dense"] = round(c["median"] / d["median"], 4)
        rec["codes_faster_by_more_than_the_spread"] = bool(c["max"] < d["min"])
    if alone and "codes" in fronts:
        rec["first_layer_kernel_alone"] = kernel_alone(model, env, width)
    return rec


def main_front(args):
    fronts = ["dense", "codes"] if args.front == "both" else [args.front]
    torch.manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "method": "device events; per_depth_ms: whole plan.step() calls, fronts alternating, 2 warm-up "
           "depths then 9 samples; split_ms_median: a second pass with an event pair per launch group, 7 samples", "cases": {}}
    env = VecCubeEnv(1000, "cuda", 3, obs=None)
    env.reset(scramble_count=100)
    for dtype in (torch.float32, torch.bfloat16):
        model = DeepCubeStandIn().cuda().to(dtype).eval()
        name = f"333_P1000_W1024_{rec_name(dtype)}"
        rec["cases"][name] = front_case(model, env, 1024, fronts)
        torch.cuda.empty_cache()
        print(json.dumps({name: rec["cases"][name]}), flush=True)
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        sd = {k: z[k] for k in z.files}
    model = DeepCubeStandIn((7, 21), sd=sd).cuda().eval()
    env2 = VecCubeEnv(10000, "cuda", 2, obs=None)
    env2.reset(seeds=list(range(10000)), scramble_count=14)
    rec["cases"]["222_checkpoint_P10000_W16_k14"] = front_case(model, env2, 16, fronts)
    print(json.dumps({"222_checkpoint_P10000_W16_k14": rec["cases"]["222_checkpoint_P10000_W16_k14"]}), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "beam_search_front.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


def rates_222(sd, width=16, max_depth=30):
    """Solve rate per fixture depth of the beam search with the checkpoint, on the fixture's own scrambles (40 seeds per depth)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    env = VecCubeEnv(len(g["ks"]), "cuda", 2, obs=None)
    env.reset(actions=g["scramble"].astype(np.uint8))
    model = DeepCubeStandIn((7, 21), sd=sd).cuda().eval()
    res = search.beam_search(model, env, width, max_depth)
    solved, length = res["solved"].cpu().numpy(), res["length"].cpu().numpy()
    out = []
    for di, k in enumerate(g["depths"]):
        m = g["ks"] == k
        out.append({"k": int(k), "beam_w16": float(solved[m].mean()), "beam_mean_length": round(float(length[m][solved[m]].mean()), 3),
                    "greedy": float(g["greedy_rate"][0, di]), "mcts_50_sims": float(g["mcts_rate"][0, di])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/beam_search.json; with --front codes | both profiles/beam_search_front.json")
    ap.add_argument("--quick", action="store_true", help="3 depths of each 3x3x3 case (for a profiler run)")
    ap.add_argument("--front", choices=("dense", "codes", "both"), default="dense",
                    help="dense: the record of the dense path (default); codes | both: the net front's record (DESIGN.md 'Net front')")
    args = ap.parse_args()
    if args.front != "dense":
        return main_front(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "beam_search.json")
    torch.manual_seed(0)
    D = 3 if args.quick else 30
    rec = {"device": torch.cuda.get_device_name(0), "cases": {}}
    env = VecCubeEnv(1000, "cuda", 3, obs=None)
    env.reset(scramble_count=100)
    for dtype in (torch.float32, torch.bfloat16):
        model = DeepCubeStandIn().cuda().to(dtype).eval()
        timed_search(model, env, 1024, 2)                          # warm-up: libraries pick their kernels
        plan, per_depth, wall = timed_search(model, env, 1024, D, sync_every=10 ** 9)
        rec["cases"][f"333_P1000_W1024_{rec_name(dtype)}"] = summarize(plan, model, per_depth, wall, dtype)
        del plan
        torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in rec["cases"][f"333_P1000_W1024_{rec_name(dtype)}"].items() if k != "per_depth_ms"}), flush=True)
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        sd = {k: z[k] for k in z.files}
    model = DeepCubeStandIn((7, 21), sd=sd).cuda().eval()
    env2 = VecCubeEnv(10000, "cuda", 2, obs=None)
    env2.reset(seeds=list(range(10000)), scramble_count=14)
    timed_search(model, env2, 16, 2)
    plan, per_depth, wall = timed_search(model, env2, 16, 30)
    r = summarize(plan, model, per_depth, wall, torch.float32)
    r["solved_fraction"] = round(r["solved"] / 10000, 4)
    rec["cases"]["222_checkpoint_P10000_W16_k14"] = r
    print(json.dumps({k: v for k, v in r.items() if k != "per_depth_ms"}), flush=True)
    if not args.quick:
        rec["solve_rate_222_w16"] = rates_222(sd)
        print(json.dumps(rec["solve_rate_222_w16"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


def rec_name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


if __name__ == "__main__":
    main()
