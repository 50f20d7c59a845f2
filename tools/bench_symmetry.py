#!/usr/bin/env python3
"""What the symmetry kernels cost on one GPU (development tool; DESIGN.md "Symmetries").

    python tools/bench_symmetry.py [--out profiles/symmetry.json] [--log2n 22] [--batch 100] [--batches 7]

2^22 3x3x3 cubes (20-move device walks), two state buffers in the default tiling.  Four things are timed with device events, in
batches that ALTERNATE between them in one process, median of the batches:
  step       an out-of-place rc_apply_moves without outputs (in -> out): the yardstick, it moves the same 2 x S bytes per cube;
  uniform    rcs_sym_apply with one symmetry for every cube (rotation 9);
  per_cube   rcs_sym_apply with a random symmetry per cube;
  canonical  rcs_sym_canonical, indices only (no image).
The record holds the times, the ratios to the step kernel and the LDS-cycle models of csrc/rc_sym.h (MI355X_MICROARCH "LDS": a wave's
ds_read of up to 4 bytes per lane takes 2 LDS cycles, a ds_write_b32 4; 256 CUs at 2.4 GHz).  The canonical search stops a wave's
comparison at the first row that decides all its cubes, so its model needs the mean number of rows compared per (wave, s): that is
counted exactly, by running the search rule in numpy on the first waves of the same states."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rubiks_cube_solver_amd import _search_lib, ops  # noqa: E402
from rubiks_cube_solver_amd.tables import get_symmetries  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, the figure bench.py's roofline uses
CUS, CLOCK = 256, 2.4e9
S, CS, K, PW = 54, 3, 48, 14
READ, WRITE = 2, 4                      # LDS cycles per wave-instruction
STAGE = S * WRITE                       # per wave: S ds_write_b32
EMIT = (S * 4 + PW * 4 + 8) * READ      # per wave: S x 4 sticker bytes, PW x 4 perm dwords, 4 x 2 relabel dwords
ROW = (1 + 1 + 4 + 4) * READ            # per compared row: the candidate's perm byte and packed row, the best's 4 perm + 4 sticker bytes
SETUP = (2 + 8) * READ                  # per s: the candidate's and the four bests' relabel rows


def rows_compared(states, waves):
    """Mean rows compared per (wave, s) by the rule of k_sym_cubes, counted on the first `waves` waves (256 cubes each)."""
    y = get_symmetries(CS)
    total = 0
    for w in range(waves):
        x = states[w * 256:(w + 1) * 256]
        img = np.stack([y.apply(x, s) for s in range(K)]).astype(np.int16)       # [K, 256, S]
        best = np.zeros(len(x), np.int64)
        for s in range(1, K):
            cur = img[best, np.arange(len(x))]
            diff = img[s] != cur
            first = np.where(diff.any(axis=1), diff.argmax(axis=1), S - 1)         # equal images are compared to the last row
            total += int(first.max()) + 1
            d = np.take_along_axis(img[s] - cur, first[:, None], axis=1)[:, 0]
            best = np.where(d < 0, s, best)
    return total / (waves * (K - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetry.json"))
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--model-waves", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_symmetry needs a GPU: nothing is estimated"
    assert a.batches >= 7
    n, dev = 1 << a.log2n, torch.device("cuda", 0)
    src = ops.alloc_states(n, CS, dev)
    dst = torch.empty_like(src)
    ops.fill_solved(src, n, CS)
    ops.scramble(src, n, CS, 20, seed=5)
    g = torch.Generator(device=dev).manual_seed(1)
    sym = torch.randint(0, K, (n,), dtype=torch.uint8, device=dev, generator=g)
    acts = torch.randint(0, 12, (n,), dtype=torch.uint8, device=dev, generator=g)
    sym_out = torch.empty(n, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.uint8, device=dev)
    legs = {"step": lambda: ops.apply_moves(src, dst, acts, n, CS),
            "uniform": lambda: ops.apply_symmetry(src, n, None, CS, 9, out=dst),
            "per_cube": lambda: ops.apply_symmetry(src, n, None, CS, sym, out=dst, bad=flag),
            "canonical": lambda: ops.canonical_symmetry(src, n, None, CS, sym_out=sym_out)}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up of every shape the timed window uses
        for _ in range(10):
            fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.batches):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.batch)     # us per call
    assert int(flag) == 0
    med = {k: statistics.median(v) for k, v in times.items()}
    rows = rows_compared(ops.to_aos(src, a.model_waves * 256).cpu().numpy(), a.model_waves)
    waves_per_cu = n / 256 / CUS
    lds_us = lambda cycles: cycles * waves_per_cu / CLOCK * 1e6
    per_cube_cycles = STAGE + EMIT
    canonical_cycles = STAGE + (K - 1) * (SETUP + rows * ROW)
    hbm_us = lambda b: b / HBM_PEAK * 1e6
    rec = {
        "command": "python tools/bench_symmetry.py", "device": torch.cuda.get_device_name(0), "librubiksearch_build_id": _search_lib.build_id(),
        "n_cubes": n, "cube_size": CS, "states": "20-move device walks", "pitch": int(src.shape[-1]),
        "timing": f"device events, {a.batches} batches of {a.batch} calls per leg, legs alternating batch by batch; us per call",
        "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "over_step": {k: round(med[k] / med["step"], 3) for k in ("uniform", "per_cube", "canonical")},
        "bytes": {"step": 2 * S * n + n, "uniform": 2 * S * n, "per_cube": 2 * S * n + n, "canonical": S * n + n},
        "us_at_hbm_peak_8TBps": {"uniform": round(hbm_us(2 * S * n), 2), "per_cube": round(hbm_us(2 * S * n + n), 2), "canonical": round(hbm_us(S * n + n), 2)},
        "lds_model": {"read_cycles": READ, "write_b32_cycles": WRITE, "cus": CUS, "clock_hz": CLOCK,
                      "per_cube_cycles_per_wave": per_cube_cycles, "per_cube_bound_us": round(lds_us(per_cube_cycles), 2),
                      "canonical_rows_compared_per_wave_and_s": round(rows, 3), "canonical_rows_counted_on_waves": a.model_waves,
                      "canonical_cycles_per_wave": round(canonical_cycles, 1), "canonical_bound_us": round(lds_us(canonical_cycles), 2)},
    }
    rec["over_lds_bound"] = {"per_cube": round(med["per_cube"] / lds_us(per_cube_cycles), 2), "canonical": round(med["canonical"] / lds_us(canonical_cycles), 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
