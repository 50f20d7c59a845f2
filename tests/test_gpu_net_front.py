"""The net front on the device (include/rubiknet.h, rubiks-cube-solver_amd/codenet.py, search.py front="codes"):

  exact        rc_net_first_layer without activation is bit-equal to the slot-order float32 restatement (tests/net_ref.py) in all four
               pairs of weight and output format; codenet.first_layer with mixed dtypes gives the raw entry point's bits
  dense        against F.linear(onehot, W1, b1) with the bound derived from the two summations
  ELU          against float64 expm1, allowed twice the error torch's own ELU shows in the same test
  ELU per pair act = 1 in every format pair against the restated sum alone: bit-equal where the reference fixes every bit, within that
               allowance elsewhere, and a bf16 result inside the band's two roundings (one rounding, after the activation)
  code bytes   every byte value 0..255 in every slot beside valid codes: the clamped row's sum, every table row selected
  CodeNet      forward_codes = model(onehot) within twice the dense path's own error against float64; weight updates are seen
  search       a BeamPlan(front="codes") in lockstep with beam_ref.Stepper; chunks; graph; the checkpoint solves the fixture
  arguments    every -1 of the header, and that a refused call writes nothing
GPU only."""
import ctypes
import functools
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


FORMATS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
FORMAT_IDS = ["f32", "bf16", "bf16_to_f32", "f32_to_bf16"]


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("fmts", FORMATS, ids=FORMAT_IDS)
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
    40 000; the four format pairs, bias and NULL, with and without a gap (4096 columns: one float32-output pair per cube size, 655 MB of
    float32 per call, and float32 weights to bf16 on the 2x2x2, whose restatement has 7 additions)."""
    cases = [((F32, F32), 512, True, 8), ((BF16, BF16), 32768, False, 0), ((BF16, F32), 40000, True, 8), ((F32, BF16), 512, False, 8)]
    if hidden == 4096:
        cases = [cases[0] if cs == 3 else cases[2], ((BF16, BF16), 512, True, 0)] + ([cases[3]] if cs == 2 else [])
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


def test_elu_against_float64_expm1_and_torch():
    """act = 1 against float64 expm1 of the kernel's own act = 0 output.  Inputs: the pre-activations of the two nets of the dense
    test, and a table whose rows are -0 and whose bias is a sweep (the sum is then the bias exactly): 3000 points of [-20, 0],
    negative denormals and tiny normals, positives, +-0, +-inf, NaN.  Allowed: twice the largest error (in float32 ulps) of
    torch.nn.functional.elu on the device on the same inputs, at least 2 ulp.  x > 0, +0, +-inf, NaN: bit-equal to torch; -0 gives -0,
    as expm1f has it (torch's ELU on the device answers +0 there)."""
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
    sweep = net_ref.elu_sweep()
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
        minus0 = np.signbit(x) & (x == 0)                              # expm1f(-0) is -0; the device's expm1, and torch's ELU with it, answers +0
        assert minus0.any() == (H == 4096) and net_ref.same_bits(np.ascontiguousarray(got[minus0]), np.ascontiguousarray(x[minus0]))
        same &= ~minus0
        assert net_ref.same_bits(np.ascontiguousarray(got[same]), np.ascontiguousarray(tor[same]))
        neg = x < 0
        exact = np.expm1(x[neg].astype(np.float64))
        worst_k = max(worst_k, float(net_ref.ulps(got[neg], exact).max()))
        worst_t = max(worst_t, float(net_ref.ulps(tor[neg], exact).max()))
    print(f"ELU, negative inputs, max error in float32 ulps against float64 expm1: kernel {worst_k:.3f}, torch.nn.functional.elu {worst_t:.3f}")
    assert worst_k <= max(2.0 * worst_t, 2.0), (worst_k, worst_t)


def launch_case(cs, codes, pitch, w, b, fmts, act, gap, tag):
    """rc_net_first_layer on a float32 table and bias (or None) that `wfmt` holds exactly -> the n x hidden result as float32 or as bf16
    bit patterns.  The out_stride gap and the 3 rows past n keep the sentinel."""
    wfmt, ofmt = fmts
    dt = torch.bfloat16 if wfmt == BF16 else torch.float32
    wt_dev = torch.tensor(w).to(dt).to(DEV)
    b_dev = None if b is None else torch.tensor(b).to(dt).to(DEV)
    assert net_ref.same_bits(wt_dev.float().cpu().numpy(), w) and (b is None or net_ref.same_bits(b_dev.float().cpu().numpy(), b)), tag
    n, hidden = len(codes), w.shape[1]
    osz = 4 if ofmt == F32 else 2
    stride, rows = hidden + gap, n + 3
    out = torch.full((rows, stride * osz), SENTINEL, dtype=torch.uint8, device=DEV)
    rc, msg = raw_first_layer(device_codes(codes, pitch), n, pitch, cs, wt_dev, b_dev, hidden, wfmt, act, out, ofmt, stride)
    assert rc == 0, msg
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    raw = host.reshape(rows, stride, osz)
    assert (raw[:n, hidden:] == SENTINEL).all() and (raw[n:] == SENTINEL).all(), ("sentinel", tag)
    return np.ascontiguousarray(host.view(np.float32 if ofmt == F32 else np.uint16).reshape(rows, stride)[:n, :hidden])


def torch_elu_error(x):
    """Largest error, in float32 ulps against float64 expm1, of torch.nn.functional.elu on the device on the negative finite x."""
    neg = ~net_ref.elu_fixed(x)
    if not neg.any():
        return 0.0
    tor = torch.nn.functional.elu(torch.tensor(x).to(DEV)).cpu().numpy()
    return float(net_ref.ulps(tor[neg], net_ref.elu_exact(x)[neg]).max())


ELU_N, ELU_HIDDEN = (1, 7, 511, 513), (8, 120, 136, 512)


@functools.lru_cache(maxsize=None)
def elu_inputs(cs, wfmt):
    """The ELU test's inputs for one cube size and weight format, computed once, shared by the two output formats and left unchanged
    -> ([(tag, codes, pitch, table, bias, gap, x = the restated pre-activation)], torch's worst ELU error on all x).
    n in {1, 7, 511, 513}: one state, less than a wave's four, the tail of a pass, two tiles at pitch 512; hidden in {8, 120, 136,
    512}: 2 live lanes, a last slab of 56 and of 8 columns, whole slabs; bias and NULL; with and without a gap; then the sweep."""
    cube = beam_ref.Cube(cs)
    cases = []
    for i, n in enumerate(ELU_N):
        for j, hidden in enumerate(ELU_HIDDEN):
            for use_bias in (True, False):
                pitch = {1: 16, 7: 16, 511: 512 if j % 2 else 528, 513: 512}[n]
                gap = 8 * ((i + j + use_bias) % 2)
                codes, w, b, x = net_ref.elu_case(cs, cube, n, hidden, use_bias, wfmt == BF16, 5000 + 1000 * i + 10 * j + use_bias)
                cases.append(((n, hidden, use_bias, pitch, gap), codes, pitch, w, b, gap, x))
    codes, w, b, x = net_ref.elu_case(cs, cube, 7, 4096, True, wfmt == BF16, 9000, sweep=True)
    assert net_ref.same_bits(x[0], b) and net_ref.same_bits(x[-1], b)                 # the sum is the sweep itself
    cases.append((("sweep", 7, 4096), codes, 16, w, b, 0, x))
    return cases, max(torch_elu_error(c[-1]) for c in cases)


def check_elu_case(cs, case, fmts, T, stats):
    """One launch with act = 1 against the reference alone; -> the number of rejected elements.  stats collects the kernel's worst
    error on the negative finite inputs (float32 ulps, or bf16 ulps for a bf16 output) and how many of them the band pins."""
    tag, codes, pitch, w, b, gap, x = case
    got = launch_case(cs, codes, pitch, w, b, fmts, 1, gap, tag)
    step = max(1, (1 << 22) // x.shape[1])                             # row blocks: the float64 temporaries stay small
    wrong = 0
    for r in range(0, len(x), step):
        bad, neg, err, pinned = net_ref.elu_check(x[r:r + step], got[r:r + step], T)
        wrong += int(bad.sum())
        samples = stats.setdefault("samples", [])                      # the first few rejected elements: (case, row, column, x, got)
        for i, h in list(zip(*np.nonzero(bad)))[:4 - len(samples)] if len(samples) < 4 else []:
            g = got[r + i, h]
            samples.append((tag, int(r + i), int(h), float(x[r + i, h]), float(g) if fmts[1] == F32 else hex(int(g))))
        if neg.any():
            err = np.nan_to_num(err, nan=np.inf) / (1.0 if fmts[1] == F32 else 65536.0)
            stats["worst"] = max(stats["worst"], float(err.max()))
            stats["neg"] += int(neg.sum())
            stats["pinned"] += 0 if pinned is None else int(pinned.sum())
    return wrong


def report_elu(name, fmts, T, worst_t, stats):
    unit = "float32" if fmts[1] == F32 else "bf16"
    print(f"ELU {name} {FORMAT_IDS[FORMATS.index(fmts)]}: T = {T:.3f} float32 ulps; torch.nn.functional.elu on the device {worst_t:.3f}; "
          f"kernel {stats['worst']:.3f} {unit} ulps on {stats['neg']} negative finite inputs"
          + ("" if fmts[1] == F32 else f", {stats['pinned']} of them fixed by the reference alone"))


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("fmts", FORMATS, ids=FORMAT_IDS)
def test_elu_is_rounded_once_after_the_activation(cs, fmts):
    """act = 1 in each of the four format pairs, expected from the restatement alone (x = net_ref.first_layer; the exact tests prove the
    kernel's act = 0 output equal to it): a float32 output is bit-equal where the reference fixes every bit (x > 0, +-0, +-inf, NaN) and
    within T ulps of float64 expm1 on the negative finite x; a bf16 output is bit-equal to the rounded exact value there, and on the
    negative finite x lies between the roundings of the band's two ends, which coincide -- equality -- on more than 99 % of them.
    T = max(2 x the largest error of torch.nn.functional.elu on the device on the same x, 2), the rule of the test above.
    Inputs: elu_inputs.  The reference is required to hold the special values and enough negative inputs."""
    cases, worst_t = elu_inputs(cs, fmts[0])
    T = max(2.0 * worst_t, 2.0)
    tiny = np.finfo(np.float32).tiny
    for tag, *_, x in cases:
        if tag[:2] == (513, 136):
            assert int(((x > -20) & (x < 0)).sum()) >= 10000, tag
    has = lambda f: any(bool(f(c[-1]).any()) for c in cases)
    assert has(np.isnan) and has(np.isposinf) and has(np.isneginf) and has(lambda x: np.signbit(x) & (x == 0))
    assert has(lambda x: (x < 0) & (x > -tiny)) and has(lambda x: (x < -88) & np.isfinite(x))
    stats = dict(worst=0.0, neg=0, pinned=0)
    wrong = [(case[0], k) for case in cases for k in [check_elu_case(cs, case, fmts, T, stats)] if k]
    report_elu(f"{cs}x{cs}x{cs}", fmts, T, worst_t, stats)
    assert not wrong, (stats.get("samples"), wrong)
    assert fmts[1] == F32 or stats["pinned"] >= 0.99 * stats["neg"], stats


@pytest.mark.parametrize("cs,n,fmts", [(3, 5125, (F32, BF16)), (2, 9221, (BF16, BF16))], ids=["333_f32_to_bf16", "222_bf16"])
def test_elu_over_several_passes_of_a_workgroup(cs, n, fmts):
    """hidden = 4096 and n = 5125 (9221) at pitch 512: 6 (10) passes of 1024 states over the 4 (8) state ranges the launcher aims at,
    2 passes per workgroup, so the next pass's codes are fetched while ELU and the bf16 store of this one run.  Checked as above."""
    cube = beam_ref.Cube(cs)
    codes, w, b, x = net_ref.elu_case(cs, cube, n, 4096, True, fmts[0] == BF16, 40 + cs)
    worst_t = torch_elu_error(x)
    T = max(2.0 * worst_t, 2.0)
    assert int(((x > -20) & (x < 0)).sum()) >= 10000
    stats = dict(worst=0.0, neg=0, pinned=0)
    wrong = check_elu_case(cs, ((n, 4096), codes, 512, w, b, 8, x), fmts, T, stats)
    report_elu(f"{cs}x{cs}x{cs} n = {n}", fmts, T, worst_t, stats)
    assert wrong == 0 and stats["pinned"] >= 0.99 * stats["neg"], (wrong, stats)


@pytest.mark.parametrize("cs", [3, 2])
def test_codenet_first_layer_with_mixed_dtypes_is_the_raw_entry_point(cs):
    """codenet.first_layer takes the dtypes of the table and of `out` independently: float32 weights to a bfloat16 out and bf16 weights to
    a float32 out, with and without ELU, give the bits of rc_net_first_layer called directly (without ELU: the restatement's), and
    leave the columns past hidden and the rows past n alone."""
    _, _, codenet, _ = mods()
    n, hidden, pitch = 513, 136, 512
    cube = beam_ref.Cube(cs)
    for wfmt, ofmt in ((F32, BF16), (BF16, F32)):
        codes, w, b, x = net_ref.elu_case(cs, cube, n, hidden, True, wfmt == BF16, 60 + cs)
        wdt, odt = (torch.bfloat16 if f == BF16 else torch.float32 for f in (wfmt, ofmt))
        for act in (False, True):
            raw = launch_case(cs, codes, pitch, w, b, (wfmt, ofmt), int(act), 8, (cs, wfmt, ofmt, act))
            out = torch.full((n + 3, hidden + 8), 7.0, dtype=odt, device=DEV)
            ret = codenet.first_layer(device_codes(codes, pitch), n, cs, torch.tensor(w).to(wdt).to(DEV), torch.tensor(b).to(wdt).to(DEV), out, act=act)
            assert ret is out
            host = out.cpu()
            assert bool((host[n:] == 7).all()) and bool((host[:, hidden:] == 7).all())
            got = host[:n, :hidden].contiguous()
            got = got.numpy() if ofmt == F32 else got.view(torch.int16).numpy().view(np.uint16)
            assert net_ref.same_bits(got, raw), (cs, wfmt, ofmt, act)
            if not act:
                assert net_ref.same_bits(got, x if ofmt == F32 else net_ref.bf16_bits(x)), (cs, wfmt, ofmt)


def byte_sweep_codes(cs, seed):
    """State v * SLOTS + s holds byte v (0 .. 255) in slot s and valid codes, drawn with `seed`, in every other slot."""
    SL, N = net_ref.SLOTS[cs], net_ref.N_CODES[cs]
    codes = np.random.default_rng(seed).integers(0, N, (256 * SL, SL)).astype(np.uint8)
    i = np.arange(256 * SL)
    codes[i, i % SL] = i // SL
    return codes


@pytest.mark.parametrize("cs,fmts", [(3, (F32, F32)), (2, (F32, F32)), (2, (BF16, BF16))], ids=["333_f32", "222_f32", "222_bf16"])
def test_every_code_byte_in_every_slot(cs, fmts):
    """One byte of 0 .. 255 in one slot beside valid codes, 5120 (1792) states in tiles of 512, act = 0: bit-equal to the restatement
    over the clamped rows (a byte at or above N_CODES counts as N_CODES - 1), for a table of mixed magnitudes and for one that makes
    the row readable: wt[k(s, c)][h] = c + 1 where h == s, else 0, no bias, so that out[i][s] = min(code_s, N_CODES - 1) + 1."""
    SL, N, R = net_ref.SLOTS[cs], net_ref.N_CODES[cs], net_ref.ROWS[cs]
    codes = byte_sweep_codes(cs, 7 + cs)
    assert len(codes) == 256 * SL and (codes[np.arange(256 * SL), np.arange(256 * SL) % SL] == np.arange(256 * SL) // SL).all()
    k = net_ref.row_index(cs, codes, clamp=True)
    assert len(np.unique(k)) == R and k.min() == 0 and k.max() == R - 1          # every table row is selected by some state
    rounded = lambda t: net_ref.bf16_to_f32(net_ref.bf16_bits(t)) if fmts[0] == BF16 else t
    expect = lambda want: want if fmts[1] == F32 else net_ref.bf16_bits(want)
    w, b = (rounded(t) for t in hard_table(np.random.default_rng(70 + cs), R, 136))
    got = launch_case(cs, codes, 512, w, b, fmts, 0, 8, ("bytes", cs, fmts))
    assert net_ref.same_bits(got, expect(net_ref.first_layer(cs, codes, w, b, clamp=True)))
    valid = np.tile(np.arange(N)[:, None], (1, SL))
    w = np.zeros((R, 32), np.float32)
    w[net_ref.row_index(cs, valid), np.arange(SL)[None, :]] = (valid + 1).astype(np.float32)
    got = launch_case(cs, codes, 512, w, None, fmts, 0, 0, ("readable", cs, fmts))
    assert net_ref.same_bits(got, expect(net_ref.first_layer(cs, codes, w, None, clamp=True)))
    value = got if fmts[1] == F32 else net_ref.bf16_to_f32(got)
    assert (value[:, :SL] == np.minimum(codes, N - 1) + 1).all() and (value[:, SL:] == 0).all()


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
