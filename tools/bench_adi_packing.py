#!/usr/bin/env python3
"""adi.AdiPlan(front="codes"): pack the hidden rows of a block to the walk count before the second layer, or feed the layers the
512-multiple the first-layer kernel wrote (adi.COMPACT_PAD_SHARE)?  200 x 30 (one chunk, 61 % padding) and
2 000 x 30 (chunks of 1024 and 976 walks, 4.7 % padding in the second), 3x3x3 [1024, 256, 128], fp32 and bf16, eager and graph: three
kept plans (never packed, always packed, front="dense") run alternately, 3 warm-up runs, 9 timed runs each, wall ms incl. the final
synchronisation.

    python tools/bench_adi_packing.py [OUT.json]      (default profiles/adi_front_packing.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from bench_adi_pipeline import stand_in
from rubiks_cube_solver_amd import adi


def main():
    dev = torch.device("cuda")
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        model = stand_in(3, dev, dtype)
        for W in (200, 2000):
            for graph in (False, True):
                plans = {}
                for name, share in (("padded", 1.0), ("packed", 0.0)):
                    adi.COMPACT_PAD_SHARE = share
                    plans[name] = adi.AdiPlan(model, 3, W, 30, 1.0, front="codes", graph=graph)
                plans["dense"] = adi.AdiPlan(model, 3, W, 30, 1.0, graph=graph)
                bs = {k: p.chunks[0][2]["bs"] for k, p in plans.items()}
                for p in plans.values():
                    for _ in range(3):
                        p.run(seed=1)
                torch.cuda.synchronize()
                t = {k: [] for k in plans}
                for r in range(9):
                    for k, p in plans.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        p.run(seed=2 + r)
                        torch.cuda.synchronize()
                        t[k].append(round((time.perf_counter() - t0) * 1e3, 4))
                key = f"{str(dtype).split('.')[1]} {W}x30 {'graph' if graph else 'eager'}"
                out[key] = {"bs": bs, "ms": t, "median_ms": {k: sorted(v)[len(v) // 2] for k, v in t.items()}}
                print(key, out[key]["median_ms"], bs, flush=True)
                del plans
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adi_front_packing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
