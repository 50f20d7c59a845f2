#!/usr/bin/env python3
"""N1 end to end: batched get_random_samples (walks + expansion + one-hots + value-net forward + target assembly)
with a random-init stand-in of the reference's DeepCube (model.py, hidden [1024,256,128]).  The reference does
393 samples/s on one CPU core with the same net; its own size is 200 cubes x depth 30
(config/config.yaml:7-8, called once per epoch by train.py:152-155).

    python tools/bench_adi_pipeline.py [walks ...] [--graph] [--reps R] [--depth D] [--cube-size 2|3]
                                       [--front dense|codes|both] [--dtype float32|bfloat16] [--out FILE]

--front both compares the two net fronts (adi.py front=) in ONE process: per size two warm-up calls per front,
then the timed calls alternate dense, codes, dense, ... (--reps per front), and every sample -- not only the median -- is appended
to profiles/adi_pipeline_front.json (--out) under a key that names dtype, cube size, graph and size.

Under `rocprofv3 --kernel-trace` every timed call is bracketed by three k_fill_solved launches on a 1-cube buffer (a kernel the
pipeline itself never launches), so tools/adi_split.py can cut the trace at the call's boundaries."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from bench_cfg5 import DeepCubeStandIn
from rubiks_cube_solver_amd import ops
from rubiks_cube_solver_amd.adi import adi_samples

SIZES = ((200, 30), (20_000, 30), (100_000, 30))


def stand_in(cube_size, dev, dtype=torch.float32):
    """Random-init DeepCube: [1024, 256, 128] (3x3x3) or the shipped 2x2x2 checkpoint's layer sizes (147 -> 512 -> 128 -> {64 -> 6, 64 -> 1})."""
    return (DeepCubeStandIn() if cube_size == 3 else DeepCubeStandIn((7, 21), 6, (512, 128, 64))).to(dev).to(dtype).eval()


def run(sizes=SIZES, reps=3, graph=False, model=None, dev=None, markers=False, cube_size=3, front="dense"):
    """-> {"WxD": {"seconds": median wall time of one adi_samples call (synchronised), "samples_per_s": ...}}
    cube_size 2: the shipped 2x2x2 checkpoint's layer sizes (pretrained/222model.pt: 147 -> 512 -> 128 -> {64 -> 6, 64 -> 1})."""
    dev = dev or torch.device("cuda")
    if model is None:
        model = stand_in(cube_size, dev)
    mark = ops.alloc_states(1, 3, dev)
    kw = {"graph": True} if graph else {}
    if front != "dense":
        kw["front"] = front
    out = {}
    for walks, depth in sizes:
        for _ in range(2):
            adi_samples(model, cube_size, walks if graph else min(walks, 2000), depth, 1.0, device=dev, seed=1, **kw)   # warm-up (graph: the capture)
        torch.cuda.synchronize()
        times = []
        for r in range(reps):
            if markers:
                for _ in range(3):
                    ops.fill_solved(mark, 1, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = adi_samples(model, cube_size, walks, depth, 1.0, device=dev, seed=2 + r, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            if markers:
                for _ in range(3):
                    ops.fill_solved(mark, 1, 3)
                torch.cuda.synchronize()
            assert res["target_value"].shape == (walks, depth)
        dt = sorted(times)[len(times) // 2]
        out[f"{walks}x{depth}"] = {"seconds": round(dt, 5), "samples_per_s": round(walks * depth / dt, 1), "best_seconds": round(min(times), 5)}
    return out


def run_both(sizes=SIZES, reps=5, graph=False, dev=None, cube_size=3, dtype=torch.float32):
    """The two fronts in one process, alternating call by call (same model, same seeds per rep) ->
    {"WxD": {"dense": {...}, "codes": {...}, "codes_over_dense": ratio of the medians, "disjoint": every codes sample < every dense sample}}
    with every sample in "seconds"."""
    dev = dev or torch.device("cuda")
    model = stand_in(cube_size, dev, dtype)
    fronts = ("dense", "codes")
    out = {}
    for walks, depth in sizes:
        for front in fronts:
            for _ in range(2):                        # warm-up at the full size: allocator, GEMM selection, with --graph the capture
                adi_samples(model, cube_size, walks, depth, 1.0, device=dev, seed=1, graph=graph, front=front)
        torch.cuda.synchronize()
        times = {f: [] for f in fronts}
        for r in range(reps):
            for front in fronts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = adi_samples(model, cube_size, walks, depth, 1.0, device=dev, seed=2 + r, graph=graph, front=front)
                torch.cuda.synchronize()
                times[front].append(time.perf_counter() - t0)
                assert res["target_value"].shape == (walks, depth)
                del res
        row = {}
        for front in fronts:
            t = times[front]
            med = sorted(t)[len(t) // 2]
            row[front] = {"seconds": [round(x, 6) for x in t], "median_seconds": round(med, 6), "min_seconds": round(min(t), 6),
                          "max_seconds": round(max(t), 6), "samples_per_s": round(walks * depth / med, 1)}
        row["codes_over_dense"] = round(row["codes"]["median_seconds"] / row["dense"]["median_seconds"], 4)
        row["disjoint"] = max(times["codes"]) < min(times["dense"])
        out[f"{walks}x{depth}"] = row
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("walks", type=int, nargs="*")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--cube-size", type=int, default=3)
    ap.add_argument("--front", choices=("dense", "codes", "both"), default="dense")
    ap.add_argument("--dtype", choices=("float32", "bfloat16"), default="float32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adi_pipeline_front.json"), help="--front both: the file the samples are merged into")
    a = ap.parse_args()
    sizes = tuple((w, a.depth) for w in a.walks) or SIZES
    dtype = getattr(torch, a.dtype)
    if a.front != "both":
        model = stand_in(a.cube_size, torch.device("cuda"), dtype)
        print(json.dumps(run(sizes, a.reps, graph=a.graph, model=model, markers=True, cube_size=a.cube_size, front=a.front)))
        return
    res = run_both(sizes, max(a.reps, 5), graph=a.graph, cube_size=a.cube_size, dtype=dtype)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("what", "tools/bench_adi_pipeline.py --front both: wall seconds of one adi_samples call incl. its final synchronisation, "
                           "front='dense' and front='codes' alternating call by call in one process after two warm-up calls per front; "
                           "random-init DeepCube ([1024, 256, 128] at 3x3x3, [512, 128, 64] at 2x2x2)")
    for size, row in res.items():
        doc[f"{a.cube_size}x{a.cube_size}x{a.cube_size} {a.dtype} {'graph' if a.graph else 'eager'} {size}"] = row
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
