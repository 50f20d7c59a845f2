"""ADI sample generation with the net fed from compact codes (adi.py front="codes", CubeEnv.adi_front):

  exact      with an integer first layer both fronts hand bit-identical inputs to identical layers: every result tensor is bit-equal
             to front="dense" across groups, chunks, the graph, the edge sizes and the three forms of `actions`
  real nets  target_value / error against the net in float64 on the oracle's walks, allowed twice the dense front's own error
             (fp32 and bf16); target_policy against the float64 argmax where the margin allows (fp32)
  graph      an in-place weight update is seen by a captured plan
  facade     CubeEnv.adi_front
  refusals   the errors of the interface, and what a codes plan holds in memory
GPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adi_front_ref as ref  # noqa: E402
import test_gpu_search as base  # noqa: E402  (DeepCube, Stub: helpers only, nothing is re-collected)
from test_gpu_net_front import random_sd  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("state_code", "target_value", "target_policy", "scramble_count", "error", "actions")
DTYPES = [torch.float32, torch.bfloat16]


def adi_mod():
    from rubiks_cube_solver_amd import adi
    return adi


def geometry(cs):
    """(A, SLOTS, R * C)"""
    return (12, 20, 480) if cs == 3 else (6, 7, 147)


def model_of(sd, dtype):
    return base.DeepCube(sd).to(DEV).to(dtype).eval()


def same(a, b, what, keys=KEYS):
    assert set(a) == set(b), what
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------ a. exact plumbing
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cs", [3, 2])
def test_codes_front_is_bit_equal_to_dense_with_an_integer_first_layer(cs, dtype):
    """First-layer weights are integers in 0..8 and the bias integers in 1..8 (the later layers are random): every pre-activation is a
    positive integer <= 168, exact in fp32 and bf16 in any summation order, and ELU is the identity on it.  Both fronts therefore feed
    bit-identical rows to the same layers, and every tensor of the result dict must be bit-equal between front="codes" and
    front="dense": 333 x 11 in several groups, 2 500 x 5 in chunks with a ragged last one, 777 x 9 through a captured graph (run
    twice), 1 x 1, 0 walks, and `actions` as a host array, a device tensor and None.  In bf16 this is also the whole check of the
    policy plumbing (see test_real_nets_bf16)."""
    adi = adi_mod()
    A, SL, RC = geometry(cs)
    hidden = ref.REAL_CASES[cs][0]
    model = model_of(ref.integer_first_layer(random_sd(cs, hidden, seed=11)), dtype)
    es = 4 if dtype == torch.float32 else 2
    T = 0.7
    plan_of = lambda W, D, front, budget=1 << 30, **kw: adi.AdiPlan(model, cs, W, D, T, dense_budget_bytes=budget, front=front, **kw)

    # 333 x 11: groups of 4 + a rest of 3 on both fronts (each front's budget in its own rows); the three forms of actions
    codes = plan_of(333, 11, "codes", 4 * (A + 1) * 512 * hidden[0] * es + 5)
    dense = plan_of(333, 11, "dense", 4 * (A + 1) * 336 * RC * es + 5)
    assert codes.group == 4 and dense.group == 4 and len(codes.chunks) == 1
    assert codes.hidden.shape == (4 * (A + 1) * 512, hidden[0]) and codes.hidden.dtype == dtype and not hasattr(codes, "dense")
    acts = np.random.default_rng(2).integers(0, A, (333, 11), dtype=np.uint8)
    for what, kw in (("device draws", dict(seed=5, stream_id=3)), ("host actions", dict(actions=acts)),
                     ("device actions", dict(actions=torch.from_numpy(acts).to(DEV)))):
        same(codes.run(**kw), dense.run(**kw), (cs, dtype, "333 x 11", what))
    assert (codes.out["actions"].cpu().numpy() == acts).all()

    # 2 500 x 5: chunks of 1024 walks + a rest of 452
    codes = plan_of(2500, 5, "codes", (A + 1) * hidden[0] * es * 1100)
    dense = plan_of(2500, 5, "dense", (A + 1) * RC * es * 1100)
    assert codes.chunk == 1024 and [c[1] for c in codes.chunks] == [1024, 1024, 452] and [c[1] for c in dense.chunks] == [1024, 1024, 452]
    same(codes.run(seed=8, stream_id=2), dense.run(seed=8, stream_id=2), (cs, dtype, "2500 x 5"))

    # 777 x 9 through a captured graph: run 1 captures, run 2 replays
    codes, dense = plan_of(777, 9, "codes", graph=True), plan_of(777, 9, "dense")
    for seed in (21, 22):
        same(codes.run(seed=seed, stream_id=1), dense.run(seed=seed, stream_id=1), (cs, dtype, "777 x 9 graph", seed))
    assert len(codes._graphs) == 1

    # the edges: one sample, no walks, and adi_samples itself (with the sample states as dense one-hots)
    same(plan_of(1, 1, "codes").run(seed=3), plan_of(1, 1, "dense").run(seed=3), (cs, dtype, "1 x 1"))
    empty = adi.adi_samples(model, cs, 0, 4, T, front="codes")
    same(empty, adi.adi_samples(model, cs, 0, 4, T), (cs, dtype, "0 walks"))
    assert tuple(empty["target_value"].shape) == (0, 4) and tuple(empty["state_code"].shape) == (0, 4, SL)
    a = adi.adi_samples(model, cs, 50, 6, T, seed=4, want_state_dense=True, front="codes")
    b = adi.adi_samples(model, cs, 50, 6, T, seed=4, want_state_dense=True)
    same(a, b, (cs, dtype, "adi_samples"), KEYS + ("state",))
    adi.release_plans()
    g = adi.adi_samples(model, cs, 50, 6, T, seed=4, graph=True, front="codes")
    same(g, {k: v for k, v in b.items() if k != "state"}, (cs, dtype, "adi_samples graph"))
    adi.adi_samples(model, cs, 50, 6, T, seed=4, graph=True)
    assert len(adi._plans) == 2                                                        # the front is part of the plan cache's key
    adi.release_plans()


# ------------------------------------------------------------------------------------------------ b, c. real-valued nets
def real_case(oracle, cs, dtype):
    """Both fronts and the float64 yardstick on the case of ref.REAL_CASES -> (dense result, codes result, float64 targets) as numpy."""
    adi = adi_mod()
    hidden, W, D = ref.REAL_CASES[cs]
    model = model_of(random_sd(cs, hidden, seed=ref.WEIGHT_SEED), dtype)
    held = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}         # the weights the device holds
    exp = oracle.adi(cs, W, D, seed=ref.WALK_SEED, stream=ref.WALK_STREAM, want_children=False, threads=4)
    want = ref.f64_targets(held, cs, exp, ref.TEMPERATURE)
    res = {}
    for front in ("dense", "codes"):
        r = adi.adi_samples(model, cs, W, D, ref.TEMPERATURE, seed=ref.WALK_SEED, stream_id=ref.WALK_STREAM, front=front)
        assert (r["actions"].cpu().numpy() == exp["actions"]).all() and (r["state_code"].cpu().numpy() == exp["parent_code"]).all(), front
        res[front] = {k: r[k].cpu().numpy() for k in ("target_value", "target_policy", "error")}
    return res["dense"], res["codes"], want


def check_values(tag, dense, codes, want):
    """max |codes - f64| <= 2 * max |dense - f64| for target_value and for error; samples with a solved child equal dense exactly."""
    E = {}
    for k in ("target_value", "error"):
        e_dense = float(np.abs(dense[k].astype(np.float64) - want[k]).max())
        e_codes = float(np.abs(codes[k].astype(np.float64) - want[k]).max())
        print(f"{tag}: max |{k} - f64|: dense {e_dense:.3e} (= E_dense), codes {e_codes:.3e}, allowed {2 * e_dense:.3e}")
        E[k] = (e_dense, e_codes)
    s = want["solved"]
    assert s.any()
    assert (codes["target_value"][s] == 1.0).all() and (dense["target_value"][s] == 1.0).all()
    assert (codes["target_policy"][s] == want["target_policy"][s]).all() and (dense["target_policy"][s] == want["target_policy"][s]).all()
    for k, (e_dense, e_codes) in E.items():
        assert e_codes <= 2 * e_dense, (tag, k, e_dense, e_codes)
    return E["target_value"][0]


@pytest.mark.parametrize("cs", [3, 2])
def test_real_nets_fp32(oracle, cs):
    """random_sd(seed 3): [1024, 256, 128] at 3x3x3 with 300 x 30, [512, 128, 64] at 2x2x2 with 600 x 14; walks of seed 5, stream 1,
    which the oracle repeats.  Yardstick: the net in float64 on the oracle's codes with the target rule restated in numpy.  With
    E_dense = max |target_value(dense) - f64| measured here on the dense front: max |target_value(codes) - f64| <= 2 * E_dense, the
    same for `error`; samples with a solved child are exactly 1.0 with the lowest solved action; target_policy equals the float64
    argmax on every sample whose float64 top-two gap is >= 8 * E_dense, and at most 1 % of the samples may fall below that gap
    (tests/test_adi_front_host.py shows on the CPU that the inputs leave a factor of 40 of room)."""
    dense, codes, want = real_case(oracle, cs, torch.float32)
    e_dense = check_values(f"{cs}x{cs}x{cs} fp32", dense, codes, want)
    excluded = ~want["solved"] & (want["gap"] < 8 * e_dense)
    print(f"{cs}x{cs}x{cs} fp32: E_dense {e_dense:.3e}; {int(excluded.sum())} of {excluded.size} samples excluded from the policy comparison "
          f"(gap < {8 * e_dense:.3e}); codes = dense policy on {int((codes['target_policy'] == dense['target_policy']).sum())}")
    assert excluded.mean() <= 0.01
    assert (codes["target_policy"][~excluded] == want["target_policy"][~excluded]).all()


@pytest.mark.parametrize("cs", [3, 2])
def test_real_nets_bf16(oracle, cs):
    """The same two nets in bf16 (yardstick: float64 on the bf16-rounded weights the device holds): the value rule and the error rule of
    the fp32 test.  target_policy is NOT compared here: a bf16 error of about 3e-3 is larger than the top-two gap of a third of the
    samples, so a comparison with the float64 argmax would exclude them; the policy plumbing in bf16 is covered by the bit-equal
    test above alone."""
    dense, codes, want = real_case(oracle, cs, torch.bfloat16)
    check_values(f"{cs}x{cs}x{cs} bf16", dense, codes, want)


# ------------------------------------------------------------------------------------------------ d. weight updates under a captured plan
@pytest.mark.parametrize("cs", [3, 2])
def test_a_captured_codes_plan_sees_in_place_weight_updates(cs):
    """AdiPlan(graph=True, front="codes"): run, add noise in place to every parameter (an optimiser step), run again with the same
    seed: the result is that of a fresh eager front="codes" plan on the updated model, bit for bit, and not that of the first run.
    The graph is not captured again: the wrapper's W1 table is refreshed eagerly, in the storage the graph reads."""
    adi = adi_mod()
    hidden = ref.REAL_CASES[cs][0]
    model = model_of(random_sd(cs, hidden, seed=ref.WEIGHT_SEED), torch.float32)
    plan = adi.AdiPlan(model, cs, 700, 8, 0.5, graph=True, front="codes")
    first = plan.run(seed=9, stream_id=2, clone=True)
    again = plan.run(seed=9, stream_id=2, clone=True)
    same(first, again, "replay")
    graph, table = plan._graphs[0], plan.net.weight_t.data_ptr()
    gen = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(torch.randn(prm.shape, generator=gen, device=DEV, dtype=prm.dtype) * 0.05)
    second = plan.run(seed=9, stream_id=2, clone=True)
    assert plan._graphs[0] is graph and plan.net.weight_t.data_ptr() == table
    fresh = adi.AdiPlan(model, cs, 700, 8, 0.5, front="codes").run(seed=9, stream_id=2)
    same(second, fresh, "after the update")
    assert not torch.equal(second["target_value"], first["target_value"]) and not torch.equal(second["error"], first["error"])
    # only the FIRST layer changed: the table is what the graph cannot see by itself
    with torch.no_grad():
        model.encoder_net[1].weight.mul_(1.5)
    third = plan.run(seed=9, stream_id=2, clone=True)
    same(third, adi.AdiPlan(model, cs, 700, 8, 0.5, front="codes").run(seed=9, stream_id=2), "after the first-layer update")
    assert not torch.equal(third["target_value"], second["target_value"])


# ------------------------------------------------------------------------------------------------ e. facade
@pytest.mark.parametrize("cs", [3, 2])
def test_cube_env_adi_front(cs):
    """env.adi_front = "codes": get_random_samples into a TensorReplayBuffer equals adi_samples(front="codes") on the same legacy draws
    exactly; switching adi_front between two calls builds a new plan (one plan is kept)."""
    import rubiks_cube_solver_amd as rc
    adi = adi_mod()
    A, SL, _ = geometry(cs)
    W, D, T = 60, 9, 0.5
    model = model_of(random_sd(cs, ref.REAL_CASES[cs][0], seed=ref.WEIGHT_SEED), torch.float32)
    env = rc.make_env(torch.device(DEV), cs)
    assert env.adi_front == "dense"
    env.adi_front = "codes"
    buf = rc.TensorReplayBuffer(10_000, 256, cs)
    np.random.seed(77)
    env.get_random_samples(buf, model, D, W, T)
    plan = next(iter(env._adi_plans.values()))
    assert plan.front == "codes" and plan.net is not None and not hasattr(plan, "dense") and plan.model is model
    np.random.seed(77)
    acts = np.random.randint(A, size=(W, D)).astype(np.uint8)
    want = adi.adi_samples(model, cs, W, D, T, actions=acts, front="codes")
    n = W * D
    assert buf.size == n
    assert torch.equal(buf.code[:n], want["state_code"].reshape(n, SL))
    assert torch.equal(buf.target_value[:n], want["target_value"].reshape(n))
    assert torch.equal(buf.target_policy[:n], want["target_policy"].reshape(n).to(torch.int64))
    assert torch.equal(buf.scramble_count[:n], want["scramble_count"].reshape(n))
    assert (buf.error_memory[:n] == want["error"].reshape(n).cpu().numpy()).all()
    env.get_random_samples(buf, model, D, W, T)
    assert next(iter(env._adi_plans.values())) is plan                                  # same front, same shape: the kept plan
    env.adi_front = "dense"
    env.get_random_samples(buf, model, D, W, T)
    other = next(iter(env._adi_plans.values()))
    assert other is not plan and other.front == "dense" and other.net is None and len(env._adi_plans) == 1
    env.adi_graph, env.adi_front = True, "codes"
    np.random.seed(77)
    buf2 = rc.TensorReplayBuffer(10_000, 256, cs)
    for _ in range(2):                                                                  # capture, then replay
        np.random.seed(77)
        env.get_random_samples(buf2, model, D, W, T)
    assert torch.equal(buf2.target_value[n:2 * n], want["target_value"].reshape(n)) and torch.equal(buf2.target_value[:n], buf2.target_value[n:2 * n])
    env.close()


# ------------------------------------------------------------------------------------------------ f. refusals and memory
def test_refusals():
    """TypeError for a module without the reference's layout (no fallback); ValueError for a float16 model, a model that is not on
    the cubes' device and an unknown front -- from AdiPlan and from adi_samples."""
    adi = adi_mod()
    sd = random_sd(2, (64, 32, 16), seed=1)
    good = base.DeepCube(sd).eval()
    for call in (lambda m, **kw: adi.AdiPlan(m, 2, 10, 2, 1.0, **kw), lambda m, **kw: adi.adi_samples(m, 2, 10, 2, 1.0, **kw)):
        with pytest.raises(TypeError, match="encoder_net"):
            call(base.Stub(2).to(DEV), front="codes")
        with pytest.raises(ValueError, match="float16"):
            call(base.DeepCube(sd).to(DEV).half(), front="codes")
        with pytest.raises(ValueError, match="the model is on cpu"):
            call(good, front="codes")
        with pytest.raises(ValueError, match="the model is on cpu"):
            call(base.DeepCube(sd).to(DEV), front="codes", model_device="cpu")
        with pytest.raises(ValueError, match="front must be"):
            call(base.DeepCube(sd).to(DEV), front="sparse")
    with pytest.raises(TypeError, match="in_features"):                                 # a 2x2x2 net for 3x3x3 cubes
        adi.AdiPlan(base.DeepCube(sd).to(DEV), 3, 10, 2, 1.0, front="codes")
    with pytest.raises(ValueError, match="dense_dtype"):
        adi.AdiPlan(base.DeepCube(sd).to(DEV), 2, 10, 2, 1.0, front="codes", dense_dtype=torch.bfloat16)
    # a CodeNet passes through unchanged
    from rubiks_cube_solver_amd.codenet import CodeNet
    net = CodeNet(base.DeepCube(sd).to(DEV).eval())
    plan = adi.AdiPlan(net, 2, 10, 2, 1.0, front="codes")
    assert plan.net is net and plan.model is net
    same(plan.run(seed=1), adi.adi_samples(net.model, 2, 10, 2, 1.0, seed=1, front="codes"), "CodeNet passed through")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cs", [3, 2])
def test_what_a_codes_plan_holds(cs, dtype):
    """No [*, R, C] tensor without want_state_dense; the hidden buffer is [group * (A + 1) * p, H1] of the model's dtype with
    row_bytes = H1 * element size: it stays within dense_budget_bytes, chunks and groups follow from it as on the dense front."""
    adi = adi_mod()
    A, SL, RC = geometry(cs)
    R, C = (20, 24) if cs == 3 else (7, 21)
    hidden = ref.REAL_CASES[cs][0]
    H1 = hidden[0]
    model = model_of(random_sd(cs, hidden, seed=1), dtype)
    row = H1 * (4 if dtype == torch.float32 else 2)

    def tensors(obj):
        if isinstance(obj, torch.Tensor):
            yield obj
        elif isinstance(obj, dict):
            for v in obj.values():
                yield from tensors(v)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                yield from tensors(v)

    for W, D, budget in ((5000, 7, 64 << 20), (5000, 7, 1 << 30), (200, 30, 1 << 30), (200, 30, 100 << 20), (3000, 4, 1 << 20)):
        plan = adi.AdiPlan(model, cs, W, D, 1.0, dense_budget_bytes=budget, front="codes")
        chunk = max(1, min(W, budget // ((A + 1) * row)))
        chunk = min(W, max(1024, chunk // 1024 * 1024)) if W > 1024 else W
        p = -(-chunk // 512) * 512
        group = max(1, min(D, budget // ((A + 1) * p * row)))
        assert (plan.chunk, plan.group) == (chunk, group), (W, D, budget)
        assert plan.hidden.shape == (group * (A + 1) * p, H1) and plan.hidden.dtype == dtype
        if budget >= (A + 1) * 1024 * row:                                              # at least one depth of the smallest chunk fits
            assert plan.hidden.numel() * plan.hidden.element_size() <= budget
        assert plan.chunks[0][2]["bufs"]["child_code"].shape[-1] == 512 and "family" not in plan.chunks[0][2]["bufs"]
        held = list(tensors(vars(plan)))
        assert held and not any(t.dim() >= 2 and tuple(t.shape[-2:]) == (R, C) for t in held)
        res = plan.run(seed=1)
        assert "state" not in res and res["state_code"].data_ptr() == plan.out["state_code"].data_ptr()
    with_state = adi.AdiPlan(model, cs, 40, 3, 1.0, want_state_dense=True, front="codes")
    assert tuple(with_state.run(seed=1)["state"].shape) == (40, 3, R, C) and not hasattr(with_state, "dense")
