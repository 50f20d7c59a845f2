"""The net front on the device (include/rubiknet.h, rubiks-cube-solver_amd/codenet.py, search.py front="codes"):

  exact        rc_net_first_layer without activation is bit-equal to the slot-order float32 restatement (tests/net_ref.py)
  dense        against F.linear(onehot, W1, b1) with the bound derived from the two summations
  ELU          against float64 expm1, allowed twice the error torch's own ELU shows in the same test
  CodeNet      forward_codes = model(onehot) within twice the dense path's own error against float64; weight updates are seen
  search       a BeamPlan(front="codes") in lockstep with beam_ref.Stepper; chunks; graph; the checkpoint solves the fixture
  arguments    every -1 of the header, and that a refused call writes nothing
GPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beam_ref  # noqa: E402
import net_ref  # noqa: E402
import test_gpu_search as base  # noqa: E402  (DeepCube, env_of, scrambles, replay_ok: helpers only, nothing is re-collected)
import test_gpu_search_edges as edges  # noqa: E402  (Lockstep, same_result)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = 4, 5
SENTINEL = 0xA5


def mods():
    from rubiks_cube_solver_amd import _lib, _net_lib, codenet, search
    return _lib, _net_lib, codenet, search


def checkpoint_sd():
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        return {k: z[k] for k in z.files}


def random_sd(cs, hidden, seed=0):
    """base._random_deepcube with a seed of its own."""
    rng = np.random.default_rng(seed)
    R, C = (20, 24) if cs == 3 else (7, 21)
    A = 12 if cs == 3 else 6
    shapes = {"encoder_net.1": (hidden[0], R * C), "encoder_net.3": (hidden[1], hidden[0]), "policy_net.0": (hidden[2], hidden[1]),
              "policy_net.2": (A, hidden[2]), "value_net.0": (hidden[2], hidden[1]), "value_net.2": (1, hidden[2])}
    sd = {}
    for k, (o, i) in shapes.items():
        sd[k + ".weight"] = (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
        sd[k + ".bias"] = (rng.standard_normal(o) * 0.01).astype(np.float32)
    return sd


def raw_first_layer(code, n, pitch, cs, wt, bias, hidden, wfmt, act, out, ofmt, stride):
    """The C entry point itself -> (return code, message)."""
    _lib, _net_lib, _, _ = mods()
    _lib.init(torch.device("cuda", torch.cuda.current_device()))
    L = _net_lib.net_lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    rc = L.rc_net_first_layer(p(code), n, pitch, cs, p(wt), p(bias), hidden, wfmt, act, p(out), ofmt, stride, _lib.stream_ptr(torch.device(DEV)))
    return rc, L.rc_net_last_error().decode()


def hard_table(rng, rows, hidden):
    """float32 [rows, hidden] and a bias: magnitudes from 1e-6 to 1e6 and both signs (the order of the additions decides the low bits),
    1 % special entries (+-0, +-inf, NaN, denormals), one column of -0 only (bias -0: the sum must stay -0) and one of +-inf rows."""
    w = (rng.standard_normal((rows, hidden)) * 10.0 ** rng.integers(-6, 7, (rows, hidden))).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-42, 3.4e38, -3.4e38], np.float32)
    hit = rng.random((rows, hidden)) < 0.01
    w[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    b = (rng.standard_normal(hidden) * 10.0 ** rng.integers(-6, 7, hidden)).astype(np.float32)
    w[:, 3], b[3] = -0.0, -0.0
    w[:, 5] = np.where(rng.random(rows) < 0.5, np.inf, -np.inf)
    b[6] = np.nan
    return w, b


def device_codes(codes, pitch):
    return torch.as_tensor(net_ref.tiled_codes(codes, pitch)).to(DEV)


def run_exact_case(cs, n, hidden, use_bias, fmts, pitch, gap, seed):
    cube = beam_ref.Cube(cs)
    rng = np.random.default_rng(seed)
    codes = cube.codes(net_ref.random_states(cube, n, rng))
    w, b = hard_table(rng, cube.R * cube.C, hidden)
    wfmt, ofmt = fmts
    if wfmt == BF16:                                              # bf16 weights: rounded once on the host, widened exactly on both sides
        wt_dev = torch.tensor(w).to(torch.bfloat16).to(DEV)
        b_dev = torch.tensor(b).to(torch.bfloat16).to(DEV)
        w, b = wt_dev.float().cpu().numpy(), b_dev.float().cpu().numpy()
    else:
        wt_dev, b_dev = torch.tensor(w).to(DEV), torch.tensor(b).to(DEV)
    want = net_ref.first_layer(cs, codes, w, b if use_bias else None)
    osz = 4 if ofmt == F32 else 2
    stride = hidden + gap
    rows = n + 3
    out = torch.full((rows, stride * osz), SENTINEL, dtype=torch.uint8, device=DEV)
    rc, msg = raw_first_layer(device_codes(codes, pitch), n, pitch, cs, wt_dev, b_dev if use_bias else None, hidden, wfmt, 0, out, ofmt, stride)
    assert rc == 0, msg
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    tag = (cs, n, hidden, use_bias, fmts, pitch, gap)
    if ofmt == F32:
        got = host.view(np.float32).reshape(rows, stride)
        assert net_ref.same_bits(np.ascontiguousarray(got[:n, :hidden]), want), tag
    else:
        got = host.view(np.uint16).reshape(rows, stride)
        assert net_ref.same_bits(np.ascontiguousarray(got[:n, :hidden]), net_ref.bf16_bits(want)), tag
    raw = host.reshape(rows, stride, osz)
    assert (raw[:n, hidden:] == SENTINEL).all() and (raw[n:] == SENTINEL).all(), ("sentinel", tag)
    # the special values did occur: the comparison above saw NaN, inf and zeros of both signs
    return np.isnan(want).any(), np.isinf(want).any(), (np.signbit(want) & (want == 0)).any()


FORMATS = [(F32, F32), (BF16, BF16), (BF16, F32)]


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("fmts", FORMATS, ids=["f32", "bf16", "bf16_to_f32"])
def test_first_layer_is_bit_equal_to_the_slot_order_sum(cs, fmts):
    """act = 0: every output bit equals net_ref.first_layer (bf16 outputs: its integer round-to-nearest-even), a NaN is a NaN.
    n in {1, 7, 511, 513} x hidden in {8, 136, 256, 512, 1024, 4096} x bias / NULL, one tile (pitch 16 | 512 | 528) and two (513 at
    pitch 512), out_stride = hidden and hidden + 8 (the gap and the rows past n keep a sentinel)."""
    seen = np.zeros(3, bool)
    for i, n in enumerate((1, 7, 511, 513)):
        for j, hidden in enumerate((8, 136, 256, 512, 1024, 4096)):
            for use_bias in (True, False):
                pitch = {1: 16, 7: 16, 511: 512 if j % 2 else 528, 513: 512}[n]
                seen |= np.array(run_exact_case(cs, n, hidden, use_bias, fmts, pitch, 8 * ((i + j + use_bias) % 2), 1000 * i + 10 * j + use_bias))
    assert seen.all(), seen


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("hidden", [8, 136, 256, 512, 1024, 4096])
def test_first_layer_is_bit_equal_on_40000_states(cs, hidden):
    """n = 40 000: 79 tiles of 512 and two tiles of 32768 (several passes per workgroup, several tiles per pass range), and one tile of
    40 000; the three format pairs, bias and NULL, with and without a gap (4096 columns: one format pair per cube size, 655 MB of
    float32 per call)."""
    cases = [((F32, F32), 512, True, 8), ((BF16, BF16), 32768, False, 0), ((BF16, F32), 40000, True, 8)]
    if hidden == 4096:
        cases = [cases[0] if cs == 3 else cases[2], ((BF16, BF16), 512, True, 0)]
    for k, (fmts, pitch, use_bias, gap) in enumerate(cases):
        run_exact_case(cs, 40000, hidden, use_bias, fmts, pitch, gap, 77 + k)


def net_cases():
    """(name, cube size, state dict): a random [1024, 256, 128] net for the 3x3x3 and the shipped 2x2x2 checkpoint."""
    return [("random_333", 3, random_sd(3, (1024, 256, 128), seed=5)), ("checkpoint_222", 2, checkpoint_sd())]


GAMMA = lambda m: (m - 1) * 2.0 ** -24 / (1 - (m - 1) * 2.0 ** -24)


@pytest.mark.parametrize("case", [0, 1], ids=["random_333", "checkpoint_222"])
def test_first_layer_against_the_dense_gemm_with_a_derived_bound(case):
    """F.linear(onehot, W1, b1) and the kernel both sum the same m = SLOTS + 1 float32 numbers in some order: each is within
    gamma_{m-1} * (|b| + sum |w|) of the exact sum, so they differ by at most twice that.  If the GEMM misses (a reduced-precision
    path), both are compared with a float64 sum and only the kernel's own bound binds."""
    _, _, codenet, _ = mods()
    name, cs, sd = net_cases()[case]
    cube = beam_ref.Cube(cs)
    rng = np.random.default_rng(3)
    st = net_ref.random_states(cube, 20000, rng)
    codes = cube.codes(st)
    n = len(codes)
    w1, b1 = sd["encoder_net.1.weight"], sd["encoder_net.1.bias"]
    W1, B1 = torch.tensor(w1).to(DEV), torch.tensor(b1).to(DEV)
    oh = torch.as_tensor(cube.onehot(st).reshape(n, -1)).to(DEV)
    dense = torch.nn.functional.linear(oh, W1, B1).cpu().numpy()
    out = torch.empty((n, w1.shape[0]), dtype=torch.float32, device=DEV)
    codenet.first_layer(device_codes(codes, 32768), n, cs, W1.t().contiguous(), B1, out, act=False)
    got = out.cpu().numpy()
    k = net_ref.row_index(cs, codes)
    w64 = w1.T.astype(np.float64)
    exact = b1.astype(np.float64)[None, :] + sum(w64[k[:, s]] for s in range(k.shape[1]))
    mag = np.abs(b1.astype(np.float64))[None, :] + sum(np.abs(w64[k[:, s]]) for s in range(k.shape[1]))
    g = GAMMA(cube.slots + 1)
    e_kernel, e_dense = np.abs(got - exact) / mag, np.abs(dense - exact) / mag
    print(f"{name}: gamma {g:.3e}; kernel max |err| / sum|t| {e_kernel.max():.3e}; dense GEMM {e_dense.max():.3e}; "
          f"max |kernel - dense| / (2 gamma sum|t|) {(np.abs(got.astype(np.float64) - dense) / (2 * g * mag)).max():.3f}")
    assert (np.abs(got - exact) <= g * mag).all(), "the kernel misses its own bound"
    if not (np.abs(got.astype(np.float64) - dense) <= 2 * g * mag).all():
        assert e_dense.max() > g, "kernel and GEMM differ by more than 2 gamma although both are within gamma of the exact sum"
        print(f"{name}: the dense GEMM is off its bound ({e_dense.max():.3e} > gamma): only the kernel's bound is binding")


def ulps(got, exact):
    """|got - exact| in units of the float32 spacing at |exact| (float64 arithmetic)."""
    e32 = np.abs(exact).astype(np.float32)
    return np.abs(got.astype(np.float64) - exact) / np.spacing(np.maximum(e32, np.float32(0))).astype(np.float64)


def test_elu_against_float64_expm1_and_torch():
    """act = 1 against float64 expm1 of the kernel's own act = 0 output.  Inputs: the pre-activations of the two nets of the dense
    test, and a table whose rows are -0 and whose bias is a sweep (the sum is then the bias exactly): 3000 points of [-20, 0],
    negative denormals and tiny normals, positives, +-0, +-inf, NaN.  Allowed: twice the largest error (in float32 ulps) of
    torch.nn.functional.elu on the device on the same inputs, at least 2 ulp.  x > 0, +-0, +-inf, NaN: bit-equal to torch."""
    _, _, codenet, _ = mods()
    F = torch.nn.functional
    rng = np.random.default_rng(9)
    worst_k, worst_t = 0.0, 0.0
    pre_list = []
    for name, cs, sd in net_cases():
        cube = beam_ref.Cube(cs)
        codes = cube.codes(net_ref.random_states(cube, 20000, rng))
        W1t, B1 = torch.tensor(sd["encoder_net.1.weight"].T.copy()).to(DEV), torch.tensor(sd["encoder_net.1.bias"]).to(DEV)
        pre_list.append((cs, codes, W1t, B1))
    sweep = np.concatenate([np.linspace(-20, 0, 3000).astype(np.float32), -np.logspace(-45, -30, 500).astype(np.float32),
                            -np.logspace(-30, -1, 500).astype(np.float32), np.logspace(-45, 38, 80).astype(np.float32),
                            np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -87.0, -88.8, -104.0, -1e30], np.float32)])
    sweep = np.concatenate([sweep, np.zeros(4096 - len(sweep), np.float32)])
    cube = beam_ref.Cube(3)
    pre_list.append((3, cube.codes(net_ref.random_states(cube, 600, rng)), torch.full((480, 4096), -0.0, device=DEV),
                     torch.tensor(sweep).to(DEV)))
    for cs, codes, W1t, B1 in pre_list:
        n, H = len(codes), W1t.shape[1]
        code = device_codes(codes, 32768)
        pre, act = torch.empty((n, H), device=DEV), torch.empty((n, H), device=DEV)
        codenet.first_layer(code, n, cs, W1t, B1, pre, act=False)
        codenet.first_layer(code, n, cs, W1t, B1, act, act=True)
        tor = F.elu(pre).cpu().numpy()
        x, got = pre.cpu().numpy(), act.cpu().numpy()
        if H == 4096:
            assert net_ref.same_bits(x[0], sweep) and net_ref.same_bits(x[-1], sweep)     # the sweep reached the activation as it is
        same = ~(x < 0)                                                # x > 0, +-0, +inf, NaN; and -inf below
        same |= np.isinf(x)
        assert net_ref.same_bits(np.ascontiguousarray(got[same]), np.ascontiguousarray(tor[same]))
        neg = x < 0
        exact = np.expm1(x[neg].astype(np.float64))
        worst_k = max(worst_k, float(ulps(got[neg], exact).max()))
        worst_t = max(worst_t, float(ulps(tor[neg], exact).max()))
    print(f"ELU, negative inputs, max error in float32 ulps against float64 expm1: kernel {worst_k:.3f}, torch.nn.functional.elu {worst_t:.3f}")
    assert worst_k <= max(2.0 * worst_t, 2.0), (worst_k, worst_t)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [0, 1], ids=["random_333", "checkpoint_222"])
def test_codenet_forward_equals_the_model_on_one_hots(case, dtype):
    """Value and policy of 100 000 random states (walks of 1..30 moves): the code path's largest error against the same net in float64
    (the weights the device holds, so bf16-rounded ones for bf16) is at most twice the dense device path's.  value_codes is
    forward_codes' value.  Then: a weight changed in place and a model re-allocated by .to(bfloat16) are picked up."""
    _, _, codenet, _ = mods()
    name, cs, sd = net_cases()[case]
    cube = beam_ref.Cube(cs)
    rng = np.random.default_rng(4)
    st = net_ref.random_states(cube, 100000, rng)
    codes = cube.codes(st)
    n = len(codes)
    model = base.DeepCube(sd).to(DEV).to(dtype).eval()
    held = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    v64, p64, _ = net_ref.deepcube_f64(held, cs, codes)
    code = device_codes(codes, 32768)
    oh = torch.as_tensor(cube.onehot(st)).to(DEV).to(dtype)
    net = codenet.CodeNet(model)
    with torch.no_grad():
        dv, dp = model(oh)
        cv, cp = net.forward_codes(code, n)
        only_v = net.value_codes(code, n)
    assert cv.dtype == dtype and cv.shape == (n, 1) and cp.shape == (n, cube.A) and torch.equal(only_v, cv)
    err = lambda t, ref: float(np.abs(t.float().cpu().numpy().astype(np.float64) - ref).max())
    ev_d, ev_c, ep_d, ep_c = err(dv, v64), err(cv, v64), err(dp, p64), err(cp, p64)
    print(f"{name} {dtype}: max |value - f64| dense {ev_d:.3e} codes {ev_c:.3e}; max |policy - f64| dense {ep_d:.3e} codes {ep_c:.3e}")
    assert ev_c <= 2 * ev_d and ep_c <= 2 * ep_d, (ev_d, ev_c, ep_d, ep_c)
    # an in-place update (an optimiser step) is seen by the next call, in the same table storage
    at = net.weight_t.data_ptr()
    m = 4096
    with torch.no_grad():
        model.encoder_net[1].weight.add_(1)
        cv2 = net.forward_codes(code, m)[0]
        dv2 = model(oh[:m])[0]
    tol = (0.03 if dtype == torch.bfloat16 else 1e-4) * float(dv2.float().abs().max())       # loose: "the new weight is in use"
    assert net.weight_t.data_ptr() == at and float((cv2.float() - cv[:m].float()).abs().max()) > 10 * tol
    assert float((cv2.float() - dv2.float()).abs().max()) <= tol
    # a re-allocated model (another dtype, other addresses) with a fresh wrapper
    if dtype == torch.float32:
        model = model.to(torch.bfloat16)
        net2 = codenet.CodeNet(model)
        with torch.no_grad():
            cv3 = net2.forward_codes(code, m)[0]
            dv3 = model(oh[:m].to(torch.bfloat16))[0]
        assert cv3.dtype == torch.bfloat16 and net2.weight_t.dtype == torch.bfloat16
        assert float((cv3.float() - dv3.float()).abs().max()) <= 0.03 * float(dv3.float().abs().max())
        net._sync()                                            # the old wrapper follows its module to the new dtype too
        assert net.weight_t.dtype == torch.bfloat16 and torch.equal(net.weight_t, net2.weight_t)


class CodesLockstep(edges.Lockstep):
    """edges.Lockstep with a BeamPlan(front="codes"): the same stage-by-stage comparison, scores from the code path."""

    def __init__(self, cs, roots_np, roots_dev, root_pitch, W, D, model, dtype, hidden, budget):
        self.cube = beam_ref.Cube(cs)
        self.P = len(roots_np)
        self.sub = np.arange(self.P)
        self.roots, self.model = roots_np, model
        self.plan = mods()[3].BeamPlan(self.P, cs, W, D, DEV, dtype, budget, front="codes", hidden=hidden)
        self.st = beam_ref.Stepper(self.cube, roots_np, W, D)
        self.plan.init(roots_dev, root_pitch)
        self.check_init()
        self.trace = []


def lockstep_case(cs, P, W, D, sd, dtype, counts, budget):
    S = mods()[3]
    scr = base.scrambles(cs, counts, seed=31)
    model = base.DeepCube(sd).to(DEV).to(dtype).eval()
    env = base.env_of(cs, scr)
    hidden = sd["encoder_net.1.weight"].shape[0]
    with torch.no_grad():
        ls = CodesLockstep(cs, beam_ref.Cube(cs).scramble(scr), env.stickers, env.stickers.shape[-1], W, D, model, dtype, hidden, budget)
        assert not hasattr(ls.plan, "dense") and ls.plan.hidden.shape == (ls.plan.chunk, hidden) and ls.plan.hidden.dtype == dtype
        assert ls.plan.chunk % ls.plan.pitch == 0 and ls.plan.A * ls.plan.nbp > 3 * ls.plan.chunk          # several chunks
        res = ls.run()
    assert base.replay_ok(cs, scr, res)
    eager = S.beam_search(model, env, W, D, front="codes", dense_budget_bytes=budget)
    edges.same_result(res, eager)
    edges.same_result(res, S.beam_search(model, env, W, D, front="codes", graph=True))          # one chunk, captured
    dense = S.beam_search(model, env, W, D)
    print(f"{cs}x{cs}x{cs} {P} x {W} {dtype}: lengths equal to front='dense' for {int((dense['length'] == res['length']).sum())} of {P}")
    return ls, res


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_beam_search_from_codes_in_lockstep_333(dtype):
    """3x3x3, 70 problems x W = 1000 (three tiles of 32768), random DeepCube, scrambles of 3..9 moves, D = 5: every buffer after
    expand, select and advance and the backtracked actions equal beam_ref.Stepper fed the device's scores; the budget forces chunks."""
    ls, _ = lockstep_case(3, 70, 1000, 5, base._random_deepcube(3), dtype, [3 + i % 7 for i in range(70)], budget=16 << 20)
    assert max(int(l.max()) for l, _ in ls.trace) == 1000                              # the beam fills: the cut decides


def test_beam_search_from_codes_in_lockstep_222_checkpoint():
    """2x2x2, 300 problems x W = 200, the shipped checkpoint, scrambles of 1..14 moves, D = 14."""
    ls, res = lockstep_case(2, 300, 200, 14, checkpoint_sd(), torch.float32, [1 + i % 14 for i in range(300)], budget=32 << 20)
    assert max(int(l.max()) for l, _ in ls.trace) == 200 and len(ls.trace) >= 8


def test_checkpoint_solves_the_fixture_from_codes():
    """beam_search(..., 16, 30, front="codes") on the 160 fixture scrambles of depths 8, 10, 12, 14: all solved, none longer than its
    scramble, the moves replay.  (On the CPU the restated search solves 160 of 160 with either first layer.)"""
    S = mods()[3]
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    pick = np.isin(g["ks"], (8, 10, 12, 14))
    scr = g["scramble"][pick].astype(np.uint8)
    assert len(scr) == 160
    model = base.DeepCube(checkpoint_sd()).to(DEV).eval()
    res = S.beam_search(model, base.env_of(2, scr), 16, 30, front="codes")
    assert bool(res["solved"].all()) and (res["length"].cpu().numpy() <= g["ks"][pick]).all()
    assert base.replay_ok(2, scr, res)
    dense = S.beam_search(model, base.env_of(2, scr), 16, 30)
    print(f"fixture: mean length codes {float(res['length'].float().mean()):.3f}, dense {float(dense['length'].float().mean()):.3f}, "
          f"equal lengths {int((dense['length'] == res['length']).sum())} of 160")
    pct = S.beam_solve_percentage(model, 2, 3, 4, 16, 10, front="codes")
    assert len(pct) == 3 and pct[0] == 100.0                                          # one move from solved: found at depth 1 whatever the scores


def test_front_codes_refuses_float16_and_foreign_devices():
    S = mods()[3]
    scr = base.scrambles(2, [3, 4], seed=1)
    env = base.env_of(2, scr)
    model = base.DeepCube(checkpoint_sd()).eval()
    with pytest.raises(ValueError, match="float16"):
        S.beam_search(model.to(DEV).half(), env, 4, 3, front="codes")
    with pytest.raises(ValueError, match="the model is on cpu"):
        S.beam_search(model.float().cpu(), env, 4, 3, front="codes")
    with pytest.raises(ValueError, match="front must be"):
        S.beam_search(model.to(DEV), env, 4, 3, front="sparse")
    with pytest.raises(ValueError, match="hidden"):
        S.BeamPlan(2, 2, 4, 3, DEV, front="codes")
    with pytest.raises(TypeError, match="encoder_net"):
        S.beam_search(base.Stub(2).to(DEV), env, 4, 3, front="codes")            # no silent fall-back to the dense path


@pytest.mark.parametrize("cs", [3, 2])
def test_argument_errors_of_rc_net_first_layer(cs):
    """Every -1 the header lists returns -1 with a message and writes nothing; n = 0 returns 0 and writes nothing."""
    SL, rows = net_ref.SLOTS[cs], net_ref.ROWS[cs]
    H, n, pitch = 64, 600, 1024
    code = torch.zeros((1, SL, pitch), dtype=torch.uint8, device=DEV)
    wt = torch.ones((rows, H), dtype=torch.float32, device=DEV)
    bias = torch.ones(H, dtype=torch.float32, device=DEV)
    out = torch.full((n, (H + 8) * 4), SENTINEL, dtype=torch.uint8, device=DEV)
    good = dict(code=code, n=n, pitch=pitch, cs=cs, wt=wt, bias=bias, hidden=H, wfmt=F32, act=1, out=out, ofmt=F32, stride=H + 8)
    bad = [("null code", dict(code=None)), ("null wt", dict(wt=None)), ("null out", dict(out=None)), ("cube size 4", dict(cs=4)),
           ("cube size 0", dict(cs=0)), ("n < 0", dict(n=-1)), ("hidden 0", dict(hidden=0)), ("hidden 4", dict(hidden=4)),
           ("hidden 60", dict(hidden=60)), ("hidden 4104", dict(hidden=4104, stride=4104)), ("hidden < 0", dict(hidden=-8)),
           ("wfmt f16", dict(wfmt=3)), ("wfmt none", dict(wfmt=0)), ("ofmt u8", dict(ofmt=2)), ("ofmt 6", dict(ofmt=6)),
           ("act 2", dict(act=2)), ("act -1", dict(act=-1)), ("stride < hidden", dict(stride=H - 8)), ("stride 0", dict(stride=0)),
           ("row of out not 16-byte aligned", dict(stride=H + 2)), ("bf16 row not aligned", dict(ofmt=BF16, stride=H + 4)),
           ("misaligned out", dict(out=out.data_ptr() + 4)), ("misaligned wt", dict(wt=wt.data_ptr() + 4)),
           ("misaligned bias", dict(bias=bias.data_ptr() + 4)), ("misaligned code", dict(code=code.data_ptr() + 1)),
           ("pitch 0", dict(pitch=0)), ("pitch < 0", dict(pitch=-512)), ("pitch % 16", dict(pitch=1000)),
           ("tiles need a power of two", dict(n=600, pitch=592)), ("tiles need >= 512", dict(n=600, pitch=256)),
           ("SLOTS * pitch >= 2^32", dict(pitch=1 << 30))]
    for what, change in bad:
        rc, msg = raw_first_layer(**dict(good, **change))
        assert rc == -1 and msg.startswith("rc_net_first_layer:"), (what, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert raw_first_layer(**dict(good, n=0))[0] == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    rc, msg = raw_first_layer(**good)                                  # and the call itself is fine: 1 + 20 (7) ones, ELU of a positive
    assert rc == 0, msg
    got = out.cpu().numpy().view(np.float32).reshape(n, H + 8)
    assert (got[:, :H] == 1 + SL).all() and (out.cpu().numpy().reshape(n, H + 8, 4)[:, H:] == SENTINEL).all()
    # an out-of-range code byte is clamped to the slot's largest code: in bounds, that row's value
    code.fill_(0xFF)
    wt.zero_()
    top = net_ref.row_index(cs, np.full((1, SL), net_ref.N_CODES[cs] - 1))[0]
    wt[torch.as_tensor(top).to(DEV)] = 2.0
    rc, msg = raw_first_layer(**dict(good, bias=None, act=0))
    assert rc == 0, msg
    assert (out.cpu().numpy().view(np.float32).reshape(n, H + 8)[:, :H] == 2 * SL).all()
