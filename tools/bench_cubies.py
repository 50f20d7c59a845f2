#!/usr/bin/env python3
"""What the cubie kernel costs on one GPU (development tool; DESIGN.md "Cubie coordinates").

    python tools/bench_cubies.py [--out profiles/cubies.json] [--batch 50] [--batches 7]

2^20 and 2^22 cubes of both sizes (20-move device walks, the default tiling).  Per size three things are timed with device events, in
batches that ALTERNATE between them in one process, median of the batches:
  encode   rc_encode(..., RC_FMT_CODE) on the same state buffer: the yardstick -- it reads the same S bytes per cube and writes the
           same SLOTS bytes;
  cubies   rcc_cubies with cubies + status                      (S + SLOTS + 1 bytes per cube);
  all      rcc_cubies with cubies + status + both indices      (+ 4, and + 8 on the 3x3x3).
The record holds the times, the ratios to rc_encode next to the ratios of the byte models, and the fraction of the HBM peak each
leg's byte model gives.  Before timing, the legs' outputs are compared once: the edge rows of the cubies are RC_FMT_CODE's, every
walked cube is legal."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rubiks_cube_solver_amd import _cubie_lib, _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, the figure bench.py's roofline uses
S_OF, SL_OF, NC_OF = {2: 24, 3: 54}, {2: 7, 3: 20}, {2: 7, 3: 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cubies.json"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 22])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cubies needs a GPU: nothing is estimated"
    assert a.batches >= 7
    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cases = []
    for cs in (3, 2):
        S, SL = S_OF[cs], SL_OF[cs]
        for log2n in a.log2n:
            n = 1 << log2n
            st = ops.alloc_states(n, cs, dev)
            ops.fill_solved(st, n, cs)
            ops.scramble(st, n, cs, 20, seed=5)
            code, cub = ops.alloc_code(n, cs, dev), ops.alloc_code(n, cs, dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)
            ci = torch.empty(n, dtype=torch.int32, device=dev)
            ei = torch.empty(n, dtype=torch.int64, device=dev) if cs == 3 else None
            # the C entry points themselves, arguments prepared once: at 2^20 cubes a launch is short enough for Python's share of an
            # ops.* call to show
            L, C, sp, P = _lib.lib(), _cubie_lib.cubie_lib(), _lib.stream_ptr(dev), _lib.ptr
            pitch, cpitch = int(st.shape[-1]), int(cub.shape[-1])
            a_st, a_code, a_cub, a_status, a_ci, a_ei = P(st), P(code), P(cub), P(status), P(ci), P(ei)
            legs = {"encode": lambda: L.rc_encode(a_st, n, pitch, cs, a_code, _lib.FMT_CODE, cpitch, sp),
                    "cubies": lambda: C.rcc_cubies(a_st, n, pitch, cs, a_cub, cpitch, a_status, None, None, sp),
                    "all": lambda: C.rcc_cubies(a_st, n, pitch, cs, a_cub, cpitch, a_status, a_ci, a_ei, sp)}
            _lib.init(dev)
            assert all(fn() == 0 for fn in legs.values())
            for fn in legs.values():                                    # warm-up of every shape the timed window uses
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            nc = NC_OF[cs]
            assert int(status.max()) == 0 and int(ci.min()) >= 0 and torch.equal(code[:, nc:], cub[:, nc:])
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
            per_cube = {"encode": S + SL, "cubies": S + SL + 1, "all": S + SL + 1 + 4 + (8 if cs == 3 else 0)}
            cases.append({
                "cube_size": cs, "n_cubes": n, "pitch": int(st.shape[-1]),
                "kernels": {"encode": _lib.describe(_lib.OP_STEP, cs, n, outputs=_lib.OUT_CODE, fmt=_lib.FMT_CODE)},
                "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
                "bytes_per_cube": per_cube,
                "over_encode": {k: round(med[k] / med["encode"], 3) for k in ("cubies", "all")},
                "byte_model_over_encode": {k: round(per_cube[k] / per_cube["encode"], 3) for k in ("cubies", "all")},
                "fraction_of_hbm_peak_8TBps": {k: round(per_cube[k] * n / (med[k] * 1e-6) / HBM_PEAK, 3) for k in legs},
            })
            del st, code, cub, status, ci, ei
    rec = {"command": "python tools/bench_cubies.py", "device": torch.cuda.get_device_name(0), "librubikhip_build_id": _lib.build_id(),
           "states": "20-move device walks, default tiling",
           "timing": f"device events, {a.batches} batches of {a.batch} calls per leg, legs alternating batch by batch; us per call",
           "byte_model": "S + SLOTS + 1 [+ 4 + 8] bytes per cube: the sticker rows in, the cubie rows and the status byte out [the indices]",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
