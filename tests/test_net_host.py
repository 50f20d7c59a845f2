"""The net front without a GPU: librubiknet.so's ABI and build id, the code -> one-hot index table, what CodeNet refuses, and the
restatement (tests/net_ref.py) against the dense first layer; its ELU checkers accept an honest float32 ELU rounded once and reject
six wrong ones."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beam_ref  # noqa: E402
import net_ref  # noqa: E402


def test_net_library_is_self_contained():
    from rubiks_cube_solver_amd import _build, _net_lib
    L = _net_lib.net_lib()                                            # loads without a GPU
    header = open(os.path.join(ROOT, "include", "rubiknet.h")).read()
    assert L.rc_net_last_error() == b""
    # the header restates the two formats of include/rubikhip.h: same values
    fmt = lambda text: {k: int(v) for k, v in re.findall(r"#define (RC_FMT_F32|RC_FMT_BF16) (\d+)", text)}
    assert fmt(header) == fmt(open(os.path.join(ROOT, "include", "rubikhip.h")).read()) == {"RC_FMT_F32": 4, "RC_FMT_BF16": 5}
    # a library of its own: apart from the host plumbing every library includes (csrc/rc_host.h), it shares no source with the others
    shared = set(_build.NET_SOURCES) & (set(_build.HIP_SOURCES) | set(_build.SEARCH_SOURCES) | set(_build.TREE_SOURCES))
    assert {os.path.basename(p) for p in shared} == {"rc_host.h"}


@pytest.mark.parametrize("cs", [3, 2])
def test_onehot_index_is_where_the_dense_one_hot_has_its_ones(cs):
    """codenet.onehot_index(cs)[s, code_s] = the argmax positions of beam_ref.Cube(cs).onehot, on 1000 random scrambles; the table is
    a bijection onto the R * C inputs where the code ranges allow (3x3x3) and injective per slot; net_ref.row_index agrees."""
    from rubiks_cube_solver_amd import codenet
    cube = beam_ref.Cube(cs)
    tab = codenet.onehot_index(cs)
    assert tab.shape == (cube.slots, net_ref.N_CODES[cs]) and tab.dtype.kind == "i"
    assert tab.min() == 0 and tab.max() == cube.R * cube.C - 1
    rng = np.random.default_rng(cs)
    st = net_ref.random_states(cube, 1000, rng)
    codes = cube.codes(st)
    flat = cube.onehot(st).reshape(len(st), -1)
    assert (flat.sum(1) == cube.slots).all()
    got = tab[np.arange(cube.slots)[None, :], codes]                                  # [n, SLOTS]
    assert (np.sort(got, 1) == np.stack([np.flatnonzero(r) for r in flat])).all()       # the same set of ones per state
    assert (flat[np.arange(len(st))[:, None], got] == 1).all()
    assert (got == net_ref.row_index(cs, codes)).all()
    if cs == 3:
        assert sorted(tab.reshape(-1)) == list(range(480))
    else:                                                                               # every slot's codes hit distinct inputs
        assert all(len(set(row)) == 21 for row in tab)


def _deepcube(in_features=480, alpha=1.0, hidden=(32, 16, 8)):
    import torch
    nn = torch.nn

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder_net = nn.Sequential(nn.Flatten(), nn.Linear(in_features, hidden[0]), nn.ELU(alpha), nn.Linear(hidden[0], hidden[1]), nn.ELU())
            self.policy_net = nn.Sequential(nn.Linear(hidden[1], hidden[2]), nn.ELU(), nn.Linear(hidden[2], 12))
            self.value_net = nn.Sequential(nn.Linear(hidden[1], hidden[2]), nn.ELU(), nn.Linear(hidden[2], 1))

    return M()


def test_codenet_refuses_what_is_not_the_reference_layout():
    import torch
    import rubiks_cube_solver_amd as pkg
    from rubiks_cube_solver_amd.codenet import CodeNet
    assert pkg.CodeNet is CodeNet and "CodeNet" in pkg.__all__
    with pytest.raises(TypeError, match="encoder_net"):
        CodeNet(torch.nn.Linear(480, 1))
    with pytest.raises(TypeError, match="alpha"):
        CodeNet(_deepcube(alpha=0.5))
    with pytest.raises(TypeError, match="in_features"):
        CodeNet(_deepcube(in_features=481))
    with pytest.raises(TypeError, match="in_features"):
        CodeNet(_deepcube(in_features=147), cube_size=3)                 # a 2x2x2 net for 3x3x3 cubes
    no_value = _deepcube()
    del no_value.value_net
    with pytest.raises(TypeError, match="value_net"):
        CodeNet(no_value)
    with pytest.raises(TypeError, match="Flatten, Linear, ELU"):
        m = _deepcube()
        m.encoder_net[2] = torch.nn.ReLU()
        CodeNet(m)
    with pytest.raises(ValueError, match="float16"):
        CodeNet(_deepcube().half())
    # the layout itself is accepted (no GPU needed to build the table), sizes are read off the module
    net = CodeNet(_deepcube())
    assert (net.cube_size, net.hidden) == (3, 32) and net.weight_t.shape == (480, 32) and net.weight_t.is_contiguous()
    assert CodeNet(_deepcube(in_features=147)).cube_size == 2


def test_codenet_table_follows_the_weight_in_the_same_storage():
    """An in-place update (optimiser step) and a re-allocated weight are both seen by _sync(); the table keeps its address."""
    import torch
    from rubiks_cube_solver_amd.codenet import CodeNet
    m = _deepcube()
    net = CodeNet(m)
    w = m.encoder_net[1].weight
    at = net.weight_t.data_ptr()
    assert torch.equal(net.weight_t, w.detach().t())
    with torch.no_grad():
        w.add_(1)
    assert not torch.equal(net.weight_t, w.detach().t())
    net._sync()
    assert torch.equal(net.weight_t, w.detach().t()) and net.weight_t.data_ptr() == at
    m.encoder_net[1].weight = torch.nn.Parameter(torch.zeros_like(w))           # re-allocated: another data_ptr
    net._sync()
    assert float(net.weight_t.abs().sum()) == 0 and net.weight_t.data_ptr() == at
    net._sync()                                                                  # nothing changed: nothing copied
    assert net._seen[0] == m.encoder_net[1].weight._version


def test_row_index_clamps_an_out_of_range_byte_to_the_largest_code():
    for cs in (3, 2):
        SL, N = net_ref.SLOTS[cs], net_ref.N_CODES[cs]
        codes = np.tile(np.arange(256)[:, None], (1, SL))
        k = net_ref.row_index(cs, codes, clamp=True)
        assert (k[:N] == net_ref.row_index(cs, codes[:N])).all() and (k[N:] == k[N - 1]).all()
        assert k.min() == 0 and k.max() == net_ref.ROWS[cs] - 1 and len(np.unique(k)) == net_ref.ROWS[cs]
        with pytest.raises(AssertionError):
            net_ref.row_index(cs, codes[:N + 1])


ELU_SHAPES = [(7, 8, False), (1, 120, False), (513, 136, False), (7, 4096, True)]      # n, hidden, the sweep


def _elu_inputs(cs, bf16):
    cube = beam_ref.Cube(cs)
    return [net_ref.elu_case(cs, cube, n, hidden, True, bf16, 3000 + 100 * cs + i, sweep)[3] for i, (n, hidden, sweep) in enumerate(ELU_SHAPES)]


def _elu32(x):
    """float32 expm1 of the float32 sum.  torch's on the CPU: it stays below 1 ulp, while numpy's float32 expm1 reaches 2.3 ulp near
    -0.011 and would not be an honest stand-in at T = 2."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    return np.where(x > 0, x, torch.expm1(torch.from_numpy(x)).numpy())


def _bits(y):
    return np.ascontiguousarray(y, np.float32).view(np.uint32)


def _honest(x):
    y = _elu32(x)
    return y, net_ref.bf16_bits(y)


def _elu_of_the_rounded_sum(x):                                             # (a)
    return None, net_ref.bf16_bits(_elu32(net_ref.bf16_to_f32(net_ref.bf16_bits(x))))


def _rounded_twice(x):                                                      # (b) to 16 significand bits, then to bf16's 8
    u = _bits(_elu32(x)).astype(np.uint64)
    mid = (((u + 0x7F + ((u >> 8) & 1)) >> 8) << 8).astype(np.uint32).view(np.float32)
    return None, np.where(np.isnan(x), net_ref.bf16_bits(_elu32(x)), net_ref.bf16_bits(mid))


def _truncated(x):                                                          # (c)
    return None, (_bits(_elu32(x)) >> 16).astype(np.uint16)


def _minus_zero_lost(x):                                                    # (d)
    y = _elu32(x)
    y[y == 0] = 0.0
    return y, net_ref.bf16_bits(y)


def _denormal_flushed(x):                                                   # (e) the sign survives, as flush-to-zero hardware has it
    y = _elu32(x)
    y[(y < 0) & (y > -np.finfo(np.float32).tiny)] = -0.0
    return y, net_ref.bf16_bits(y)


def _minus_inf_kept(x):                                                     # (f)
    y = _elu32(x)
    y[np.isneginf(x)] = -np.inf
    return y, net_ref.bf16_bits(y)


MUTANTS = [_elu_of_the_rounded_sum, _rounded_twice, _truncated, _minus_zero_lost, _denormal_flushed, _minus_inf_kept]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32_table", "bf16_table"])
@pytest.mark.parametrize("cs", [3, 2])
def test_elu_checkers_accept_the_restatement_and_reject_six_mutants(cs, bf16):
    """net_ref.elu_wrong at T = 2 on the device test's inputs (mild tables of 7 x 8, 1 x 120 and 513 x 136, and the sweep): float32
    expm1 of the float32 sum, rounded once, passes in both output formats.  Rejected: (a) ELU of the bf16-rounded sum, (b) a second
    rounding through 16 significand bits, (c) truncation, (d) -0 answered +0, (e) a negative denormal flushed, (f) -inf kept.
    (a) is caught even on the two smallest shapes and on more than 5 % of the large one's negative elements (a bf16 rounding of
    the sum moves it by up to 2^-9 of itself, the result by about as much, against a band a few 2^-24 wide); the band's ends
    coincide for more than 99.9 % of them, so there the reference alone fixes the bf16 result."""
    T = 2.0
    xs = _elu_inputs(cs, bf16)
    for x in xs:
        y, b = _honest(x)
        assert not net_ref.elu_wrong(x, y, T).any() and not net_ref.elu_wrong(x, b, T).any()
    big = xs[2]
    neg = ~net_ref.elu_fixed(big)
    assert ((big > -20) & (big < 0)).sum() >= 10000
    pinned = net_ref.bf16_between(_honest(big)[1], *net_ref.elu_bounds(big, T))[1]
    assert pinned[neg].mean() > 0.999
    union = np.concatenate([x.reshape(-1) for x in xs])
    tiny = np.finfo(np.float32).tiny
    assert np.isnan(union).any() and np.isposinf(union).any() and np.isneginf(union).any() and (np.signbit(union) & (union == 0)).any()
    assert ((union < 0) & (union > -tiny)).any() and ((union < -88) & np.isfinite(union)).any()
    for mutant in MUTANTS:
        caught32, caught16 = 0, []
        for x in xs:
            y, b = mutant(x)
            caught16.append(int(net_ref.elu_wrong(x, b, T).sum()))
            caught32 += 0 if y is None else int(net_ref.elu_wrong(x, y, T).sum())
        print(f"{cs} bf16 table {bf16} {mutant.__name__}: rejected bf16 elements per input {caught16}, float32 elements {caught32}")
        assert sum(caught16) > 0, mutant.__name__
        if mutant in MUTANTS[3:]:
            assert caught32 > 0, mutant.__name__
        if mutant is _elu_of_the_rounded_sum:
            assert caught16[0] >= 2 and caught16[1] >= 2 and caught16[2] > 0.05 * neg.sum(), caught16


def test_bf16_between_orders_the_bit_patterns_like_the_values():
    v = np.array([-np.inf, -3.0, -1.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, 3.0, np.inf], np.float32)
    bits = net_ref.bf16_bits(v)
    for i in range(len(v)):
        for j in range(i, len(v)):
            inside, pinned = net_ref.bf16_between(bits, np.full(len(v), v[i]), np.full(len(v), v[j]))
            assert (inside == ((np.arange(len(v)) >= i) & (np.arange(len(v)) <= j))).all() and (pinned == (i == j)).all()
    nan = np.full(1, np.nan, np.float32)
    inside, pinned = net_ref.bf16_between(net_ref.bf16_bits(nan), nan, nan)
    assert inside.all() and pinned.all()
    assert not net_ref.bf16_between(net_ref.bf16_bits(nan), -np.ones(1, np.float32), np.full(1, np.inf, np.float32))[0].any()
    assert not net_ref.bf16_between(net_ref.bf16_bits(np.ones(1, np.float32)), nan, nan)[0].any()


@pytest.mark.parametrize("cs", [3, 2])
def test_restated_row_sum_is_the_dense_first_layer(cs):
    """net_ref.first_layer (slot order, float32) against onehot @ W1.T + b1 in float64: within gamma_m * (|b| + sum |w|), m = SLOTS + 1
    terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4).  bf16 rounding restated with integers equals torch's."""
    import torch
    cube = beam_ref.Cube(cs)
    rng = np.random.default_rng(10 + cs)
    H = 72
    w1 = rng.standard_normal((H, cube.R * cube.C)).astype(np.float32)
    b1 = rng.standard_normal(H).astype(np.float32)
    st = net_ref.random_states(cube, 500, rng)
    codes, oh = cube.codes(st), cube.onehot(st).reshape(len(st), -1)
    got = net_ref.first_layer(cs, codes, np.ascontiguousarray(w1.T), b1)
    exact = oh.astype(np.float64) @ w1.T.astype(np.float64) + b1
    mag = oh.astype(np.float64) @ np.abs(w1.T).astype(np.float64) + np.abs(b1)
    u, m = 2.0 ** -24, cube.slots + 1
    gamma = (m - 1) * u / (1 - (m - 1) * u)
    assert (np.abs(got - exact) <= gamma * mag).all()
    x = np.concatenate([rng.standard_normal(5000).astype(np.float32) * 1e3, np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, 3.3895314e38], np.float32),
                        rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[~np.isnan(x)]
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (net_ref.bf16_bits(x) == want).all()
    assert (net_ref.bf16_to_f32(want) == torch.tensor(x).to(torch.bfloat16).float().numpy()).all()
    assert ((net_ref.bf16_bits(np.array([np.nan], np.float32)) & 0x7FFF) > 0x7F80).all()
