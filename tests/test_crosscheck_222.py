"""the only evidence available for the UNPINNED 2x2x2 convention.

The reference ships a trained 2x2x2 DeepCube checkpoint (pretrained/222model.pt) but not the
py222 module that defined its state encoding.  If our restated 2x2x2 tables / one-hot convention
match the authors', their policy net must solve shallow scrambles of OUR cubes greedily.

The checkpoint's float32 weights are the fixture tests/golden/crosscheck_222_weights.npz (tensor name -> array), which
tests/golden/make_crosscheck_222.py reads from the checkpoint statically: nothing is unpickled or executed."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_weights():
    """the checkpoint's state dict (model weights only) from the fixture"""
    with np.load(os.path.join(GOLDEN, "crosscheck_222_weights.npz")) as z:
        return {k: z[k] for k in z.files}


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def policy_logits(sd, x):
    """model.py:13-45: Flatten -> Linear/ELU x2 -> policy head Linear/ELU/Linear."""
    h = elu(x.reshape(len(x), -1) @ sd["encoder_net.1.weight"].T + sd["encoder_net.1.bias"])
    h = elu(h @ sd["encoder_net.3.weight"].T + sd["encoder_net.3.bias"])
    p = elu(h @ sd["policy_net.0.weight"].T + sd["policy_net.0.bias"])
    return p @ sd["policy_net.2.weight"].T + sd["policy_net.2.bias"]


def test_checkpoint_policy_solves_our_222_cubes():
    from oracle.oracle_np import OracleCubeEnv
    sd = load_weights()
    assert sd["encoder_net.1.weight"].shape == (512, 147) and sd["policy_net.2.weight"].shape == (6, 64)
    env = OracleCubeEnv(None, 2)
    rates = {}
    for k in (1, 2, 3, 4, 6, 8):
        solved = 0
        for seed in range(40):
            state, done = env.reset(seed=seed, scramble_count=k), False
            for _ in range(30):
                a = int(np.argmax(policy_logits(sd, state[None].astype(np.float32))[0]))
                state, _, done, _ = env.step(a)
                if done:
                    break
            solved += done
        rates[k] = solved / 40
    print("2x2x2 greedy solve rate of the shipped checkpoint on the restated env:", rates)
    # a convention mismatch leaves the net blind: solve rates would sit near chance even at depth 1-2
    assert rates[1] >= 0.9 and rates[2] >= 0.9 and rates[4] >= 0.8


def _fixture():
    return np.load(os.path.join(GOLDEN, "crosscheck_222.npz"))


def test_fixture_matches_live_checkpoint_run():
    """tests/golden/crosscheck_222.npz (actions and outcomes of the run above, no weights) is what the checkpoint does
    on the restated env today: regenerate a slice and compare."""
    from oracle.oracle_np import OracleCubeEnv
    g = _fixture()
    sd = load_weights()
    env = OracleCubeEnv(None, 2)
    for i in range(0, len(g["seeds"]), 7):
        state = env.reset(seed=int(g["seeds"][i]), scramble_count=int(g["ks"][i]))
        for t in range(int(g["solve_step"][i])):
            a = int(np.argmax(policy_logits(sd, state[None].astype(np.float32))[0]))
            assert a == g["actions"][i, t]
            state, _, d, _ = env.step(a)
            assert (np.argmax(state, 1) == g["cols"][i, t]).all() and d == g["done"][i, t]


def test_negative_controls_regenerate():
    """The control conventions of the fixture are re-run here on a slice (greedy, depths 2 and 6, 20 seeds): the live rates
    equal what the fixture recorded for those seeds' population within sampling, and every control stays far below the
    shipped convention."""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_crosscheck_222 as mk
    sd = load_weights()
    live = {}
    for conv in mk.CONVENTIONS:
        env = mk.ConventionEnv(conv)
        live[conv] = [np.mean([mk.greedy(sd, env, seed, k)[3] > 0 for seed in range(20)]) for k in (2, 6)]
    assert live["shipped"] == [1.0, 1.0]
    for conv in mk.CONVENTIONS[1:]:
        assert live[conv][0] <= 0.5 and live[conv][1] <= 0.15, (conv, live[conv])
