#!/usr/bin/env python3
"""What auto-reset costs per env step on one GPU (development tool; DESIGN.md "Episodes").

    python tools/bench_episode.py [--out profiles/episode_autoreset.json] [--log2n 22] [--batch 200] [--batches 9]

2^22 3x3x3 cubes, obs="code", random actions, scramble_count=(1, 3), max_episode_steps=30.  Three things are timed with device
events, in batches that ALTERNATE between them in one process, median of the batches:
  plain   VecCubeEnv.step of an env without auto-reset (one launch: move + reward + done + code);
  auto    VecCubeEnv(auto_reset=True).step (three launches: move, rcx_episode_end, encode), its time limits desynchronised (elapsed
          starts uniform in [0, 30)) so that every step sees the steady share of ended cubes, which is measured first;
  end     rcx_episode_end alone on done masks with exactly that share of ended cubes (no time limit: the masks decide).
The record holds the three times, the ended share, the bytes rcx_episode_end moves by the model of csrc/rc_episode.h (14 B per
cube, 2 x S x 4 B per lane with an ended cube, 8 B per ended cube) and the time that traffic would take at the HBM peak."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from rubiks_cube_solver_amd import _lib, ops  # noqa: E402
from rubiks_cube_solver_amd.vec_env import VecCubeEnv  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, the figure bench.py's roofline uses
S, CS, MAX_STEPS, DEPTH = 54, 3, 30, (1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_autoreset.json"))
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--batches", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_episode needs a GPU: nothing is estimated"
    assert a.batches >= 7
    n, dev = 1 << a.log2n, torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    acts = torch.randint(0, 12, (16, n), dtype=torch.uint8, device=dev, generator=g)
    plain = VecCubeEnv(n, dev, CS, obs="code", seed=3)
    plain.reset(scramble_count=3)
    auto = VecCubeEnv(n, dev, CS, obs="code", seed=3, auto_reset=True, scramble_count=DEPTH, max_episode_steps=MAX_STEPS)
    auto.reset(scramble_count=3)
    auto.elapsed.copy_(torch.randint(0, MAX_STEPS, (n,), dtype=torch.int32, device=dev, generator=g))
    # the steady share of ended cubes per step (and of lanes = 4-packs with one): 2 x MAX_STEPS warm-up steps, then MAX_STEPS measured ones
    for i in range(2 * MAX_STEPS):
        auto.step(acts[i % 16])
    ended = lanes = term = 0
    for i in range(MAX_STEPS):
        e = auto.step(acts[i % 16])[3]["ended"]
        ended += int((e != 0).sum())
        term += int((e == 1).sum())
        lanes += int((e.view(-1, 4) != 0).any(dim=1).sum())
    share, lane_share = ended / (MAX_STEPS * n), lanes / (MAX_STEPS * (n // 4))
    # rcx_episode_end alone: 16 done masks with that share, buffers of its own
    st = auto.stickers.clone()
    masks = (torch.rand((16, n), device=dev, generator=g) < share).to(torch.uint8)
    mask_share = float(masks.float().mean())
    mask_lane_share = float((masks.view(16, -1, 4) != 0).any(dim=2).float().mean())
    el, ep = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    en, ln = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def end_alone(i):
        ops.episode_end(st, n, CS, masks[i % 16], el, ep, en, ln, max_steps=0, depth=DEPTH, seed=3, stream_id=1, walk_offset=0, walk_stride=n)

    legs = {"plain_step": lambda i: plain.step(acts[i % 16]), "auto_reset_step": lambda i: auto.step(acts[i % 16]), "episode_end_alone": end_alone}
    times = {k: [] for k in legs}
    for fn in legs.values():                                        # warm-up of every shape the timed window uses
        for i in range(20):
            fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.batches):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.batch):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.batch)     # us per call
    plain.check_actions()
    bytes_end = n * 14 + mask_lane_share * (n // 4) * 2 * S * 4 + mask_share * n * 8
    rec = {
        "command": "python tools/bench_episode.py", "device": torch.cuda.get_device_name(0), "librubikhip_build_id": _lib.build_id(),
        "n_cubes": n, "cube_size": CS, "obs": "code", "scramble_count": list(DEPTH), "max_episode_steps": MAX_STEPS,
        "timing": f"device events, {a.batches} batches of {a.batch} calls per leg, legs alternating batch by batch; us per call",
        "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
        "auto_over_plain": round(statistics.median(times["auto_reset_step"]) / statistics.median(times["plain_step"]), 3),
        "ended_share_per_step": share, "terminated_share_per_step": term / (MAX_STEPS * n), "lanes_with_an_ended_cube_share": lane_share,
        "episode_end_alone": {"ended_share": mask_share, "lanes_with_an_ended_cube_share": mask_lane_share, "bytes_moved": int(bytes_end),
                              "bytes_model": "14 B x cubes + 2 x 54 x 4 B x lanes with an ended cube + 8 B x ended cubes",
                              "us_at_hbm_peak_8TBps": round(bytes_end / HBM_PEAK * 1e6, 2),
                              "fraction_of_hbm_peak": round(bytes_end / HBM_PEAK * 1e6 / statistics.median(times["episode_end_alone"]), 3)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
