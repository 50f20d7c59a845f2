"""The ADI net front (adi.py front=, CubeEnv.adi_front) as far as a machine without a GPU can see it: the parameters and their
defaults, the facade's plan key, the refusal of a bad front before any device is touched, and that the policy condition of
tests/test_gpu_adi_front.py holds by the float64 reference alone on the inputs it uses."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adi_front_ref as ref  # noqa: E402
from test_gpu_net_front import random_sd  # noqa: E402  (a helper: nothing of that module is collected here)


def test_front_is_a_parameter_defaulting_to_dense():
    from rubiks_cube_solver_amd.adi import AdiPlan, adi_samples
    for fn in (AdiPlan.__init__, adi_samples):
        prm = inspect.signature(fn).parameters
        assert "front" in prm and prm["front"].default == "dense", fn


def _env(cs):
    from tests.fake_backend import HostLogicCubeEnv
    return HostLogicCubeEnv(torch.device("cpu"), cube_size=cs)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(480, 1)

    def forward(self, x):
        if x.dim() == 2:
            x = x.unsqueeze(0)
        return self.lin(x.reshape(x.shape[0], -1).float()), torch.zeros(x.shape[0], 12)


def test_cube_env_adi_front_defaults_to_dense_and_is_part_of_the_plan_key():
    """A fresh env has adi_front == "dense"; the same call twice keeps the plan; a changed adi_front makes the next
    get_random_samples call _new_adi_plan again (with its unchanged five-argument signature) and keeps one plan."""
    env = _env(3)
    assert env.adi_front == "dense"
    made = []
    orig = type(env)._new_adi_plan

    def counting(self, model, n_walks, depth, temperature, want_state_dense):
        made.append(self.adi_front)
        return orig(self, model, n_walks, depth, temperature, want_state_dense)

    net = Net()
    type(env)._new_adi_plan = counting
    try:
        sink = []
        env.get_random_samples(sink, net, 3, 2, 1.0)
        env.get_random_samples(sink, net, 3, 2, 1.0)
        assert made == ["dense"] and len(sink) == 12
        env.adi_front = "codes"
        env.get_random_samples(sink, net, 3, 2, 1.0)
        env.get_random_samples(sink, net, 3, 2, 1.0)
        assert made == ["dense", "codes"] and len(sink) == 24 and len(env._adi_plans) == 1
        env.adi_front = "dense"
        env.get_random_samples(sink, net, 3, 2, 1.0)
        assert made == ["dense", "codes", "dense"]
    finally:
        type(env)._new_adi_plan = orig


def test_a_bad_front_is_refused_before_any_device_is_touched(monkeypatch):
    """ValueError from AdiPlan and adi_samples (eager and graph) although every torch.cuda entry point a plan would need raises."""
    from rubiks_cube_solver_amd.adi import AdiPlan, adi_samples

    def touched(*a, **k):
        raise AssertionError("a device was touched")

    for name in ("current_device", "init", "_lazy_init", "synchronize", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, touched)
    net = Net()
    with pytest.raises(ValueError, match="front must be"):
        AdiPlan(net, 3, 10, 2, 1.0, front="sparse")
    for graph in (False, True):
        with pytest.raises(ValueError, match="front must be"):
            adi_samples(net, 3, 10, 2, 1.0, graph=graph, front="family")
    with pytest.raises(ValueError, match="float16"):           # needs no device either
        AdiPlan(Net().half(), 3, 10, 2, 1.0, front="codes")


@pytest.mark.parametrize("cs", [3, 2])
def test_the_policy_condition_holds_by_the_reference_alone(oracle, cs):
    """test_gpu_adi_front compares target_policy with the float64 argmax where the float64 top-two gap is >= 8 * E_dense and caps the
    excluded share at 1 %.  On its inputs fewer than 1 % of the samples have a gap below 1e-4: E_dense (about 3e-7 in float32) would
    have to be 40 x its expected size before the cap could bind."""
    hidden, W, D = ref.REAL_CASES[cs]
    sd = random_sd(cs, hidden, seed=ref.WEIGHT_SEED)
    exp = oracle.adi(cs, W, D, seed=ref.WALK_SEED, stream=ref.WALK_STREAM, want_children=False, threads=4)
    want = ref.f64_targets(sd, cs, exp, ref.TEMPERATURE)
    gap = want["gap"]
    share = float((gap < 1e-4).mean())
    print(f"{cs}x{cs}x{cs}: {W} x {D} samples, {int(want['solved'].sum())} with a solved child; smallest gap {gap.min():.3e}, "
          f"1 % quantile {np.quantile(gap[np.isfinite(gap)], 0.01):.3e}, share below 1e-4: {share:.5f}")
    assert share < 0.01
    assert want["solved"][:, 0].all() and (want["target_value"][want["solved"]] == 1.0).all()      # depth 1: the inverse move solves
