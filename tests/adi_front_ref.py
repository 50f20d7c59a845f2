"""numpy side of the ADI net-front tests (tests/test_gpu_adi_front.py, tests/test_adi_front_host.py): the two nets and the two sets of
walks the issue fixes, the exact-integer first layer, and the ADI target rule (cube_env.py:229-251) restated in float64 on the oracle's
codes with net_ref.deepcube_f64 as the net.  Test infrastructure only."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import net_ref  # noqa: E402

# (cube size, hidden sizes, walks, depth): the real-valued cases; both use seed 5, stream 1 for the walks and seed 3 for the weights
REAL_CASES = {3: ((1024, 256, 128), 300, 30), 2: ((512, 128, 64), 600, 14)}
WALK_SEED, WALK_STREAM, WEIGHT_SEED, TEMPERATURE = 5, 1, 3, 0.7


def integer_first_layer(sd, seed=0):
    """A copy of the state dict whose first layer holds integers: weights in 0..8, bias in 1..8.  Every pre-activation is then a
    positive integer <= 8 + 20 * 8 = 168: exact in float32 and in bfloat16 in any summation order, and ELU is the identity on it."""
    rng = np.random.default_rng(seed)
    sd = dict(sd)
    sd["encoder_net.1.weight"] = rng.integers(0, 9, sd["encoder_net.1.weight"].shape).astype(np.float32)
    sd["encoder_net.1.bias"] = rng.integers(1, 9, sd["encoder_net.1.bias"].shape).astype(np.float32)
    return sd


def f64_targets(sd, cube_size, exp, temperature):
    """The float64 yardstick on the oracle's walks `exp` (Oracle.adi): dict of
      target_value [W, D], target_policy [W, D], error [W, D], solved [W, D] (a child is solved),
      gap [W, D]: best minus second best child value (the policy's margin; inf where a child is solved)."""
    cc, pc = exp["child_code"], exp["parent_code"]
    W, D, A, SL = cc.shape
    v_child = net_ref.deepcube_f64(sd, cube_size, cc.reshape(-1, SL))[0].reshape(W, D, A) - 1.0
    v_par = net_ref.deepcube_f64(sd, cube_size, pc.reshape(-1, SL))[0].reshape(W, D)
    solved = exp["child_solved"].astype(bool)
    any_solved = solved.any(-1)
    tv = np.where(any_solved, 1.0, v_child.max(-1))
    tp = np.where(any_solved, np.argmax(solved, -1), np.argmax(v_child, -1))
    srt = np.sort(v_child, -1)
    gap = np.where(any_solved, np.inf, srt[..., -1] - srt[..., -2])
    err = np.abs(v_par - tv) * np.arange(1, D + 1, dtype=np.float64)[None, :] ** (-1 * temperature)
    return {"target_value": tv, "target_policy": tp, "error": err, "solved": any_solved, "gap": gap}
