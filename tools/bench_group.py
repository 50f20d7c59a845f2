#!/usr/bin/env python3
"""What the cube-group kernels cost on one GPU, and what the solvers gain from them (development tool; DESIGN.md "Cube group").

    python tools/bench_group.py [--out profiles/group.json] [--batch 20] [--batches 7] [--log2n 22] [--skip-solvers]

Kernels: cg_product, cg_inverse, cg_random and, as the yardstick of the same process, rcc_from_cubies, at 2^22 cubes of both sizes
(uniform cubes from cg_random, the default tiling).  Device events around batches that ALTERNATE between the legs, median of the
batches.  Each leg stands beside its byte model (SLOTS bytes per operand row set: 3 / 2 / 1 of them, S + SLOTS for the yardstick) over
the achievable HBM rate, and cg_random beside its instruction count (tools/kernel_usage.py) over the VALU issue rate.
Solvers (3x3x3, the defaults of two_phase_solve): two_phase_solve_both against two_phase_solve on the same 1000 uniform cubes, and
random_state_scramble for 1000 and 65 536 cubes; a host clock to the synchronise, second repetition."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rubiks_cube_solver_amd import _cubie_lib, _group_lib, _lib, ops  # noqa: E402

HBM_ACHIEVABLE = 6.3e12                 # bytes / s: what a float4 copy reaches of the 8.0e12 peak
S_OF, SL_OF = {2: 24, 3: 54}, {2: 7, 3: 20}
SIMDS, CLOCK, LANE_CYCLES = 1024, 2.4e9, 4          # 256 CUs x 4 SIMDs; a wave64 VALU instruction issues in 4 cycles


def kernels(a, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    G, C, sp, P = _group_lib.group_lib(), _cubie_lib.cubie_lib(), _lib.stream_ptr(dev), _lib.ptr
    cases = []
    for cs in (3, 2):
        S, SL = S_OF[cs], SL_OF[cs]
        n = 1 << a.log2n
        x, y = ops.random_cubies(n, cs, dev, seed=1), ops.random_cubies(n, cs, dev, seed=2)
        out, st = torch.empty_like(x), ops.alloc_states(n, cs, dev, x.shape[-1])
        bad = torch.zeros(16, dtype=torch.uint8, device=dev)
        pitch = int(x.shape[-1])
        a_x, a_y, a_out, a_st, a_bad = P(x), P(y), P(out), P(st), P(bad)
        legs = {"from_cubies": lambda: C.rcc_from_cubies(a_x, n, pitch, cs, a_st, pitch, a_bad, sp),
                "product": lambda: G.cg_product(a_x, pitch, a_y, pitch, n, cs, a_out, pitch, a_bad, sp),
                "inverse": lambda: G.cg_inverse(a_x, pitch, n, cs, a_out, pitch, a_bad, sp),
                "random": lambda: G.cg_random(3, 0, 0, n, cs, a_out, pitch, sp)}
        assert all(fn() == 0 for fn in legs.values())
        for fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        assert int(bad[0]) == 0
        times = {k: [] for k in legs}
        for _ in range(a.batches):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.batch):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.batch)     # us per call
        med = {k: statistics.median(v) for k, v in times.items()}
        per_cube = {"from_cubies": SL + S, "product": 3 * SL, "inverse": 2 * SL, "random": SL}
        cases.append({
            "cube_size": cs, "n_cubes": n, "pitch": pitch,
            "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "bytes_per_cube": per_cube,
            "byte_model_us_at_6.3TBps": {k: round(per_cube[k] * n / HBM_ACHIEVABLE * 1e6, 2) for k in legs},
            "over_byte_model": {k: round(med[k] / (per_cube[k] * n / HBM_ACHIEVABLE * 1e6), 2) for k in legs},
            "over_from_cubies": {k: round(med[k] / med["from_cubies"], 3) for k in legs if k != "from_cubies"},
            "byte_model_over_from_cubies": {k: round(per_cube[k] / per_cube["from_cubies"], 3) for k in legs if k != "from_cubies"},
            "TBps": {k: round(per_cube[k] * n / (med[k] * 1e-6) / 1e12, 3) for k in legs},
        })
        del x, y, out, st
    return cases


def valu_models(cases):
    """The VALU issue time of every cg_* kernel from the instruction counts in profiles/group_usage.json, which
    `python tools/kernel_usage.py k_cg_ --json profiles/group_usage.json` writes (a cross-compile: no GPU needed, so not made here)."""
    usage = json.load(open(os.path.join(ROOT, "profiles", "group_usage.json")))["kernels"]
    name = {"product": "k_cg_product", "inverse": "k_cg_inverse", "random": "k_cg_random"}
    for c in cases:
        waves_per_simd = c["n_cubes"] / 64 / SIMDS
        c["valu_issue_us"] = {}
        for leg, kern in name.items():
            row = next(r for r in usage if r["kernel"] == f"{kern}<Cube{c['cube_size']}>")
            c["valu_issue_us"][leg] = {"valu_instructions": row["valu_instructions"],
                                       "us": round(waves_per_simd * row["valu_instructions"] * LANE_CYCLES / CLOCK * 1e6, 2)}
    return usage


def clock(fn):
    fn()                                                                     # first repetition: allocations, warm caches
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def solvers(dev):
    from rubiks_cube_solver_amd import VecCubeEnv, pattern, search
    tp, chain = pattern.TwoPhaseTables.build(dev), pattern.ChainTables.build(dev)
    env = VecCubeEnv(1000, dev, 3, obs=None)
    env.reset_uniform(2026)
    plain, t_plain = clock(lambda: search.two_phase_solve(tp, chain, env))
    both, t_both = clock(lambda: search.two_phase_solve_both(tp, chain, env))
    chain_res, t_chain = clock(lambda: search.chain_solve(chain, env))
    assert bool(plain["solved"].all()) and bool(both["solved"].all()) and bool((both["length"] <= plain["length"]).all())
    stat = lambda length: {"mean": round(float(length.float().mean()), 3), "min": int(length.min()), "max": int(length.max())}
    rec = {"both_against_plain": {"cubes": 1000, "draw": "reset_uniform(2026)", "settings": "two_phase_solve's defaults",
                                  "two_phase_solve": {"seconds": round(t_plain, 3), "length": stat(plain["length"])},
                                  "two_phase_solve_both": {"seconds": round(t_both, 3), "length": stat(both["length"]),
                                                           "share_won_by_the_inverse_side": round(float(both["side"].float().mean()), 4)},
                                  "chain_solve": {"seconds": round(t_chain, 4), "length": stat(chain_res["length"])}},
           "random_state_scramble": []}
    for n in (1000, 65536):
        out, t = clock(lambda: search.random_state_scramble(tp, chain, n, seed=7, device=dev))
        rec["random_state_scramble"].append({"cubes": n, "seconds": round(t, 3), "us_per_cube": round(t / n * 1e6, 2), "length": stat(out["length"])})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group.json"))
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--skip-solvers", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_group needs a GPU: nothing is estimated"
    assert a.batches >= 5
    dev = torch.device("cuda", 0)
    _lib.init(dev)
    cases = kernels(a, dev)
    rec = {"command": "python tools/bench_group.py", "device": torch.cuda.get_device_name(0), "librubikhip_build_id": _lib.build_id(),
           "cubes": "uniform, from cg_random; default tiling",
           "timing": f"device events, {a.batches} batches of {a.batch} calls per leg, legs alternating batch by batch; us per call",
           "byte_model": "SLOTS bytes per row set read or written (product 3, inverse 2, random 1; rcc_from_cubies S + SLOTS) over 6.3e12 B/s",
           "valu_model": "waves per SIMD x VALU instructions of the kernel x 4 cycles at 2.4 GHz: every instruction issued once, no overlap",
           "kernels": cases}
    try:
        rec["kernel_usage"] = valu_models(cases)
    except OSError as e:                                                     # the usage record was not made: the record says so
        rec["kernel_usage"] = f"not available: {type(e).__name__}: {e}"
    if not a.skip_solvers:
        rec["solvers"] = solvers(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
