"""The cube group on the GPU (include/rubikhip.h "Cube group": cg_product, cg_inverse, cg_random, cg_invert_actions) and what is built on
it (ops.group_product / group_inverse / random_cubies / invert_actions, VecCubeEnv.compose / invert / reset_uniform, search.relative_to /
invert_actions / two_phase_solve_both / random_state_scramble).

  a. bytes: against the restatement (tests/cubegroup_ref.py) at every count that opens another path, both cube sizes, every ordered
     combination of three layouts for (x, y, out), every operand carved, guards and pad columns, in place, bad input, argument errors;
  b. the group laws on the device's own output;
  c. cg_random bit for bit, cut into chunks, legal, distinct, and uniform over the 2x2x2's distances;
  d. cg_invert_actions; e. the solver tie-ins; f. each launching export under capture and replay.
Every comparison is exact; the one statistical test has the cap of tests/test_cubegroup_host.py.  GPU only."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from rubiks_cube_solver_amd import _group_lib, _lib, ops
from tests import cubegroup_ref as R
from tests import cubie_ref as CR
from tests import layout_cases as LC
from tests.test_gpu_cubies import FILL, Arena, rows_arena
from tests.test_gpu_search import env_of, scrambles

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as C  # noqa: E402
import stream_driver as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
COUNTS = (1, 3, 513, 1029, 2565)
LAYOUTS = ("tight", "padded", "t512")
NMAX = max(COUNTS)
# two_phase_solve's budget in the solver tests: the settings of tests/test_gpu_twophase.py's end-to-end test, which takes about a
# second at 2565 cubes; here 513 cubes, two solves in two_phase_solve_both
TP = dict(candidates=4, phase1_limit=12, phase2_limit=16, max_steps=30000, steps_per_call=8192)


@pytest.fixture(scope="module")
def lib():
    _lib.init(torch.device(DEV, torch.cuda.current_device()))
    return _group_lib.group_lib()


def stream():
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def walked_env(cs, n, seed):
    from rubiks_cube_solver_amd import VecCubeEnv
    env = VecCubeEnv(n, DEV, cs, obs=None, seed=seed)
    env.reset(scramble_count=100)
    return env


def rows_of(t, n):
    return ops.to_aos(t, n).cpu().numpy()


class Pool:
    """2565 cubes x, y, z of one size from device walks of 100 moves, and the restatement's x o y and x^-1, computed once."""

    def __init__(self, cs):
        self.env = [walked_env(cs, NMAX, 11 * cs + k) for k in range(3)]
        self.x, self.y, self.z = (rows_of(e.cubies(), NMAX) for e in self.env)
        self.xy, self.inv = R.product(cs, self.x, self.y), R.inverse(cs, self.x)
        assert (R.product_bytes(cs, self.x, self.y)[0] == self.xy).all() and (R.inverse_bytes(cs, self.x)[0] == self.inv).all()
        for a in (self.x, self.y, self.z, self.xy, self.inv):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def pools():
    return {cs: Pool(cs) for cs in LC.CUBE_SIZES}


def flag_arena(offset):
    a = Arena(16, offset)
    a.host[a.start:a.start + 16] = 0
    return a.upload()


def run_product(lib, cs, n, X, Y, lays, carve, want, want_bad=0):
    SL = LC.SL_OF[cs]
    offs = LC.carve_offsets(4) if carve else [0] * 4
    x, y = rows_arena(X[:n], n, SL, lays[0], offs[0]).upload(), rows_arena(Y[:n], n, SL, lays[1], offs[1]).upload()
    out, bad = rows_arena(None, n, SL, lays[2], offs[2]).upload(), flag_arena(offs[3])
    rc = lib.cg_product(x.ptr(), x.pitch, y.ptr(), y.pitch, n, cs, out.ptr(), out.pitch, bad.ptr(), stream())
    assert rc == 0, _lib.lib().rc_last_error()
    out.expect_rows(want[:n], out.pitch)
    bad.expect(np.array([want_bad], np.uint8))
    for a, what in ((x, "x"), (y, "y"), (out, "out"), (bad, "bad")):
        a.check(f"cg_product {cs} {n} {lays} {what}")


def run_inverse(lib, cs, n, X, lays, carve, want, want_bad=0):
    SL = LC.SL_OF[cs]
    offs = LC.carve_offsets(3) if carve else [0] * 3
    x, out, bad = rows_arena(X[:n], n, SL, lays[0], offs[0]).upload(), rows_arena(None, n, SL, lays[1], offs[1]).upload(), flag_arena(offs[2])
    rc = lib.cg_inverse(x.ptr(), x.pitch, n, cs, out.ptr(), out.pitch, bad.ptr(), stream())
    assert rc == 0, _lib.lib().rc_last_error()
    out.expect_rows(want[:n], out.pitch)
    bad.expect(np.array([want_bad], np.uint8))
    for a, what in ((x, "x"), (out, "out"), (bad, "bad")):
        a.check(f"cg_inverse {cs} {n} {lays} {what}")


# ------------------------------------------------------------------------------------------------------------------ a. bytes
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_product_and_inverse_in_every_layout_carved(lib, pools, cs, n):
    P = pools[cs]
    for lays in itertools.product(LAYOUTS, repeat=3):
        if n in LC.SIZES:
            LC.check_premise(n, *lays)
        run_product(lib, cs, n, P.x, P.y, lays, True, P.xy)
    for lays in itertools.product(LAYOUTS, repeat=2):
        run_inverse(lib, cs, n, P.x, lays, True, P.inv)
    for lay in LAYOUTS:                                                     # and at the allocation's own alignment
        run_product(lib, cs, n, P.x, P.y, (lay,) * 3, False, P.xy)
        run_inverse(lib, cs, n, P.x, (lay,) * 2, False, P.inv)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_in_place(lib, pools, cs, n):
    P, SL = pools[cs], LC.SL_OF[cs]
    for lay, other in zip(LAYOUTS, LAYOUTS[1:] + LAYOUTS[:1]):
        offs = LC.carve_offsets(3)
        for which in ("x", "y", "inverse"):
            a = rows_arena((P.y if which == "y" else P.x)[:n], n, SL, lay, offs[0]).upload()
            b = rows_arena((P.x if which == "y" else P.y)[:n], n, SL, other, offs[1]).upload()
            bad = flag_arena(offs[2])
            if which == "x":
                rc = lib.cg_product(a.ptr(), a.pitch, b.ptr(), b.pitch, n, cs, a.ptr(), a.pitch, bad.ptr(), stream())
            elif which == "y":
                rc = lib.cg_product(b.ptr(), b.pitch, a.ptr(), a.pitch, n, cs, a.ptr(), a.pitch, bad.ptr(), stream())
            else:
                rc = lib.cg_inverse(a.ptr(), a.pitch, n, cs, a.ptr(), a.pitch, bad.ptr(), stream())
            assert rc == 0, _lib.lib().rc_last_error()
            a.expect_rows((P.inv if which == "inverse" else P.xy)[:n], a.pitch)
            for t in (a, b, bad):
                t.check(f"in place {which} {cs} {n} {lay}")


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_bad_input_gives_the_identity_and_the_flag(lib, pools, cs):
    P, nc, n = pools[cs], R.NC_OF[cs], 1029
    x, y = P.x[:n].copy(), P.y[:n].copy()
    x[5, 0], y[600, nc - 1], y[1028, 2] = 3 * nc, 255, 3 * nc + 2
    if cs == 3:
        x[7, nc + 3], y[520, nc + 11] = 24, 0x80
    y[9, 1] = y[9, 0]                                                       # a piece twice: the product is the gather as written
    y[10, :nc] = y[10, 0]
    want, bad = R.product_bytes(cs, x, y)
    assert bad.sum() == (5 if cs == 3 else 3) and (want[9] == R.product(cs, x[9:10], y[9:10])[0]).all()
    run_product(lib, cs, n, x, y, ("t512", "tight", "padded"), True, want, 1)
    run_product(lib, cs, n, P.x, P.y, ("t512", "tight", "padded"), True, P.xy, 0)
    want, bad = R.inverse_bytes(cs, y)
    assert bad.sum() == (5 if cs == 3 else 4) and bad[9] and bad[10]
    run_inverse(lib, cs, n, y, ("padded", "t512"), True, want, 1)
    # every corner byte and every edge byte value, one per cube, in slot 0 / slot NC: 3 * NC .. 255 and 24 .. 255 are flagged
    for slot, limit in ((0, 3 * nc),) + (((nc, 24),) if cs == 3 else ()):
        x = P.x[:256].copy()
        x[:, slot] = np.arange(256)
        want, bad = R.product_bytes(cs, x, P.y[:256])
        assert (bad == (np.arange(256) >= limit)).all()
        run_product(lib, cs, 256, x, P.y, ("tight", "tight", "tight"), False, want, 1)
        run_product(lib, cs, 256, P.y, x, ("tight", "tight", "tight"), False, R.product_bytes(cs, P.y[:256], x)[0], 1)
        run_inverse(lib, cs, 256, x, ("tight", "tight"), False, R.inverse_bytes(cs, x)[0], 1)


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_argument_errors_write_nothing(lib, pools, cs):
    P, SL, n = pools[cs], LC.SL_OF[cs], 513
    err = lambda: _lib.lib().rc_last_error().decode()
    mk = lambda rows, lay: rows_arena(rows, n, SL, lay, 16).upload()
    x, y, out, bad = mk(P.x[:n], "tight"), mk(P.y[:n], "padded"), mk(None, "t512"), flag_arena(16)
    big = rows_arena(P.x[:n], n, SL, "tight", 16)                           # x and a second buffer that starts inside it
    big.upload()
    inside = ctypes.c_void_p(big.view.data_ptr() + 32)
    off = lambda a: ctypes.c_void_p(a.view.data_ptr() + 8)
    s = stream()

    def product(**kw):
        a = dict(x=x.ptr(), x_pitch=x.pitch, y=y.ptr(), y_pitch=y.pitch, n=n, cs=cs, out=out.ptr(), out_pitch=out.pitch, bad=bad.ptr())
        a.update(kw)
        return lib.cg_product(a["x"], a["x_pitch"], a["y"], a["y_pitch"], a["n"], a["cs"], a["out"], a["out_pitch"], a["bad"], s)

    def inverse(**kw):
        a = dict(x=x.ptr(), x_pitch=x.pitch, n=n, cs=cs, out=out.ptr(), out_pitch=out.pitch, bad=bad.ptr())
        a.update(kw)
        return lib.cg_inverse(a["x"], a["x_pitch"], a["n"], a["cs"], a["out"], a["out_pitch"], a["bad"], s)

    def random(**kw):
        a = dict(first=0, n=n, cs=cs, out=out.ptr(), out_pitch=out.pitch)
        a.update(kw)
        return lib.cg_random(1, 2, a["first"], a["n"], a["cs"], a["out"], a["out_pitch"], s)

    cases = [(product, dict(x=None), "x is NULL"), (product, dict(x=off(x)), "x is NULL or not 16"), (product, dict(y=None), "y is NULL"),
             (product, dict(y=off(y)), "y is NULL or not 16"), (product, dict(out=None), "out is NULL"), (product, dict(out=off(out)), "out is NULL or not 16"),
             (product, dict(bad=None), "bad is NULL"), (product, dict(n=-1), "n is negative"), (product, dict(cs=4), "cube_size"),
             (product, dict(x_pitch=x.pitch + 8), "x_pitch"), (product, dict(x_pitch=496), "x_pitch"), (product, dict(y_pitch=0), "y_pitch"),
             (product, dict(out_pitch=400), "out_pitch"), (product, dict(out_pitch=256), "out_pitch"),
             (product, dict(out=x.ptr(), out_pitch=x.pitch + 16), "out overlaps x"), (product, dict(out=y.ptr(), out_pitch=y.pitch + 16), "out overlaps y"),
             (product, dict(x=big.ptr(), x_pitch=big.pitch, out=inside, out_pitch=big.pitch), "out overlaps x"),
             (product, dict(y=big.ptr(), y_pitch=big.pitch, out=inside, out_pitch=big.pitch), "out overlaps y"),
             (inverse, dict(x=None), "x is NULL"), (inverse, dict(x=off(x)), "x is NULL or not 16"), (inverse, dict(out=None), "out is NULL"),
             (inverse, dict(bad=None), "bad is NULL"), (inverse, dict(n=-1), "n is negative"), (inverse, dict(cs=1), "cube_size"),
             (inverse, dict(x_pitch=8), "x_pitch"), (inverse, dict(out_pitch=520), "out_pitch"),
             (inverse, dict(x=big.ptr(), x_pitch=big.pitch, out=inside, out_pitch=big.pitch), "out overlaps x"),
             (random, dict(out=None), "out is NULL"), (random, dict(out=off(out)), "out is NULL or not 16"), (random, dict(n=-1), "n is negative"),
             (random, dict(first=-1), "first"), (random, dict(first=2 ** 63 - 5), "first"), (random, dict(cs=0), "cube_size"),
             (random, dict(out_pitch=100), "out_pitch")]
    for fn, kw, text in cases:
        assert fn(**kw) == EINVAL and text in err() and fn.__name__ in err(), (fn.__name__, kw, err())
    # the action lists
    L, ap = 7, LC.ceil16(n)
    acts, aout = Arena(L * ap, 16).upload(), Arena(L * (ap + 16), 16).upload()

    def invert(**kw):
        a = dict(actions=acts.ptr(), rows=L, n=n, act_pitch=ap, cs=cs, out=aout.ptr(), out_pitch=ap + 16, bad=bad.ptr())
        a.update(kw)
        return lib.cg_invert_actions(a["actions"], a["rows"], a["n"], a["act_pitch"], a["cs"], a["out"], a["out_pitch"], a["bad"], s)

    for kw, text in ((dict(actions=None), "actions is NULL"), (dict(actions=off(acts)), "actions is NULL or not 16"), (dict(out=None), "out is NULL"),
                     (dict(out=off(aout)), "out is NULL or not 16"), (dict(bad=None), "bad is NULL"), (dict(rows=-1), "rows is negative"),
                     (dict(n=-1), "n is negative"), (dict(cs=5), "cube_size"), (dict(act_pitch=ap - 16), "act_pitch"), (dict(act_pitch=ap + 8), "act_pitch"),
                     (dict(out_pitch=n), "out_pitch"), (dict(out=acts.ptr(), out_pitch=ap + 16), "out overlaps actions"),
                     (dict(out=ctypes.c_void_p(acts.view.data_ptr() + 16), out_pitch=ap), "out overlaps actions")):
        assert invert(**kw) == EINVAL and text in err() and "cg_invert_actions" in err(), (kw, err())
    # n == 0 succeeds without a launch, whatever the pitches hold
    assert product(n=0) == 0 and inverse(n=0) == 0 and random(n=0) == 0 and invert(n=0) == 0 and invert(rows=0) == 0
    torch.cuda.synchronize()
    for a in (x, y, out, bad, big, acts, aout):
        a.check("an argument error wrote")


# ------------------------------------------------------------------------------------------------------------ b. group laws
def solved_states(cs, n):
    st = ops.alloc_states(n, cs, DEV)
    ops.fill_solved(st, n, cs)
    return st


def replay(st, cs, n, actions):
    """The actions [n, k] (A: no move) played on the sticker buffer st by the step kernel, in place."""
    for k in range(actions.shape[1]):
        ops.apply_moves(st, st, torch.as_tensor(np.ascontiguousarray(actions[:, k])).to(DEV), n, cs)
    return st


def same(a, b, n):
    return torch.equal(ops.to_aos(a, n), ops.to_aos(b, n))


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_group_laws_on_the_device(pools, cs):
    P, n = pools[cs], NMAX
    x, y, z = (e.cubies() for e in P.env)
    mul = lambda a, b: ops.group_product(a, b, n, cs)
    inv = lambda a: ops.group_inverse(a, n, cs)
    e = ops.from_aos(R.identity(cs, n), DEV)
    assert same(mul(mul(x, y), z), mul(x, mul(y, z)), n)
    assert same(mul(x, inv(x)), e, n) and same(mul(inv(x), x), e, n) and same(mul(x, e), x, n) and same(mul(e, x), x, n)
    assert same(inv(mul(x, y)), mul(inv(y), inv(x)), n) and same(inv(inv(x)), x, n)
    assert not same(mul(x, y), mul(y, x), n)
    # one move: rc_apply_moves by a = the product with the cube "solved then a"
    for a in range(LC.A_OF[cs]):
        col = torch.full((n,), a, dtype=torch.uint8, device=DEV)
        moved, move = torch.empty_like(P.env[0].stickers), solved_states(cs, n)
        ops.apply_moves(P.env[0].stickers, moved, col, n, cs)
        ops.apply_moves(move, move, col, n, cs)
        assert same(mul(x, ops.cubies(move, n, cs)["cubies"]), ops.cubies(moved, n, cs)["cubies"], n), a
    # a walked cube: x o y = rc_scramble_from(x, the actions of y)
    A, depth = LC.A_OF[cs], 100
    acts = torch.zeros((depth, _lib.pitch_for(n)), dtype=torch.uint8, device=DEV)
    walked = solved_states(cs, n)
    ops.scramble(walked, n, cs, depth, seed=5, stream_id=9, actions_out=acts)
    onto_x = torch.empty_like(P.env[0].stickers)
    ops.scramble(onto_x, n, cs, depth, actions_in=acts, src=P.env[0].stickers)
    assert same(mul(x, ops.cubies(walked, n, cs)["cubies"]), ops.cubies(onto_x, n, cs)["cubies"], n)


def test_the_order_of_r_u_is_105():
    n = 1
    st = replay(solved_states(3, n), 3, n, np.array([[4, 0]], np.uint8))    # R U
    g = ops.cubies(st, n, 3)["cubies"]
    e = ops.from_aos(R.identity(3, n), DEV)
    power, orders = g, []
    for k in range(1, 106):
        if same(power, e, n):
            orders.append(k)
        power = ops.group_product(power, g, n, 3)
    assert orders == [105]


def test_the_twelve_classes_multiply_as_their_bits_say(pools):
    """tests/test_cubies_host.py's (twist, flip, swap) classes: RCC_TWIST, RCC_FLIP, RCC_PARITY of a product follow from its factors."""
    P, n = pools[3], 64
    classes = CR.classes(3)
    status = lambda rows: CR.cubies(3, CR.from_cubies(3, rows)[0])[1]
    for (t1, f1, p1), (t2, f2, p2) in itertools.product(classes, repeat=2):
        a, b = CR.mutate(3, P.x[:n], t1, f1, p1), CR.mutate(3, P.y[:n], t2, f2, p2)
        assert (status(a) == CR.class_status(t1, f1, p1)).all() and (status(b) == CR.class_status(t2, f2, p2)).all()
        got = rows_of(ops.group_product(ops.from_aos(a, DEV), ops.from_aos(b, DEV), n, 3), n)
        assert (status(got) == CR.class_status((t1 + t2) % 3, f1 ^ f2, p1 ^ p2)).all(), ((t1, f1, p1), (t2, f2, p2))
        inv = rows_of(ops.group_inverse(ops.from_aos(a, DEV), n, 3), n)
        assert (status(inv) == CR.class_status(t1, f1, p1)).all()


@pytest.fixture(scope="module")
def table_222():
    from rubiks_cube_solver_amd import pattern
    return pattern.CornerTable.build(2, DEV)


def test_the_inverse_keeps_the_distance_of_all_222_cubes(table_222):
    """rcp_unrank -> cg_inverse -> rcc_from_cubies -> rcc_cubies index -> look-up, for all 3 674 160 indices."""
    N = table_222.table.numel()
    assert N == sum(R.SPHERES_222)
    idx = torch.arange(N, dtype=torch.int32, device=DEV)
    cub = table_222.cubies(idx)
    inv = ops.group_inverse(cub, N, 2)
    back = ops.cubies(ops.from_cubies(inv, N, 2), N, 2, cubies=False, index=True)
    assert not bool(back["status"].any())
    ci = back["corner_index"].long()
    assert bool((table_222.table[ci] == table_222.table).all())
    assert int((ci != idx.long()).sum()) > N // 2                           # and it is not the identity map
    assert torch.equal(torch.sort(ci).values, idx.long())                    # a bijection of the group


# ---------------------------------------------------------------------------------------------------------------- c. cg_random
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_random_equals_the_restatement(lib, cs):
    SL = LC.SL_OF[cs]
    for n, (seed, sid) in itertools.product(COUNTS, ((0, 0), (1, 7), (2 ** 64 - 1, 2 ** 40 + 3))):
        for lay in LAYOUTS if seed == 1 else ("t512",):
            out = rows_arena(None, n, SL, lay, 16).upload()
            assert lib.cg_random(seed, sid, 0, n, cs, out.ptr(), out.pitch, stream()) == 0, _lib.lib().rc_last_error()
            out.expect_rows(R.random_cubies(cs, seed, sid, 0, n), out.pitch)
            out.check(f"cg_random {cs} {n} {seed} {sid} {lay}")
    n = (1 << 18) + 5
    for seed, sid in ((0, 1), (1, 0), (2 ** 64 - 1, 5)):
        got = ops.random_cubies(n, cs, DEV, seed=seed, stream_id=sid)
        assert got.shape[0] > 1 and (rows_of(got, n) == R.random_cubies(cs, seed, sid, 0, n)).all()
        assert not bool(got.permute(0, 2, 1).reshape(-1, SL)[n:].any())      # pad columns keep their bytes


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_random_cut_into_chunks_and_legal(cs):
    whole = ops.random_cubies(2565, cs, DEV, seed=3, stream_id=4)
    a, b = ops.random_cubies(1029, cs, DEV, seed=3, stream_id=4), ops.random_cubies(1536, cs, DEV, seed=3, stream_id=4, first=1029)
    assert torch.equal(ops.to_aos(whole, 2565), torch.cat([ops.to_aos(a, 1029), ops.to_aos(b, 1536)]))
    n = 1 << 20
    cub = ops.random_cubies(n, cs, DEV, seed=8, stream_id=cs)
    out = ops.cubies(ops.from_cubies(cub, n, cs), n, cs, cubies=False, index=True)
    assert not bool(out["status"].any())
    if cs == 3:                                                              # 2^20 draws from 4.3e19 cubes: a repeat has probability 1e-8
        key = torch.stack([out["corner_index"].long(), out["edge_index"]], 1)
        assert len(torch.unique(key, dim=0)) == n


def test_random_222_distance_histogram(table_222):
    n = 1 << 22
    cub = ops.random_cubies(n, 2, DEV, seed=20261021, stream_id=1)
    dist = table_222.distance(ops.from_cubies(cub, n, 2), n)
    hist = torch.bincount(dist.long(), minlength=15).cpu().numpy()
    assert len(hist) == 15
    expected = R.merged_222(R.SPHERES_222) * (n / sum(R.SPHERES_222))
    chi = R.chi2(R.merged_222(hist), expected)
    print(f"2x2x2 distance histogram of 2^22 draws: chi2 {chi:.1f}, df 11, cap {11 + 6 * 22 ** 0.5:.1f}")
    assert chi <= 11 + 6 * 22 ** 0.5


# ------------------------------------------------------------------------------------------------------- d. cg_invert_actions
@pytest.mark.parametrize("rows", (1, 31, 87))
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_invert_actions_equals_the_restatement(lib, cs, rows):
    A = LC.A_OF[cs]
    for n in (1, 513, 1029):
        rng = np.random.default_rng(rows * 10000 + n + cs)
        acts = rng.integers(0, A, (rows, n)).astype(np.uint8)
        acts[rng.random((rows, n)) < 0.25] = A                               # no-ops anywhere
        acts[rows // 2:, ::3] = A                                            # at the end
        acts[:, 1::7] = A                                                    # everywhere
        if n > 4:
            acts[:, 2] = rng.integers(0, A, rows)                            # a column of full length
        want, bad = R.invert_actions(cs, acts)
        assert not bad
        ap, op = LC.ceil16(n), LC.ceil16(n) + 48
        for in_place in (False, True):
            src = Arena(rows * ap, 16)
            src.host[src.start + (np.arange(rows)[:, None] * ap + np.arange(n)[None, :])] = acts
            src.upload()
            dst = src if in_place else Arena(rows * op, 48).upload()
            flag = flag_arena(80)
            rc = lib.cg_invert_actions(src.ptr(), rows, n, ap, cs, dst.ptr(), ap if in_place else op, flag.ptr(), stream())
            assert rc == 0, _lib.lib().rc_last_error()
            dst.host[dst.start + (np.arange(rows)[:, None] * (ap if in_place else op) + np.arange(n)[None, :])] = want
            for a in (src, dst, flag):
                a.check(f"cg_invert_actions {cs} {rows} {n} in_place={in_place}")
        # an entry above A: skipped, and the flag
        acts[rows // 3, n // 2] = A + 1 + (n % 3)
        want, bad = R.invert_actions(cs, acts)
        assert bad
        buf = torch.full((rows, ap), FILL, dtype=torch.uint8, device=DEV)
        buf[:, :n] = torch.as_tensor(acts).to(DEV)
        flag = torch.zeros(16, dtype=torch.uint8, device=DEV)
        got = ops.invert_actions(buf, n, cs, bad=flag)
        assert (got[:, :n].cpu().numpy() == want).all() and flag.cpu().tolist() == [1] + [0] * 15
        with pytest.raises(IndexError):
            ops.invert_actions(buf, n, cs)


# --------------------------------------------------------------------------------------------------------------- e. solvers
@pytest.fixture(scope="module")
def tp():
    from rubiks_cube_solver_amd import pattern
    return pattern.TwoPhaseTables.build(DEV)


@pytest.fixture(scope="module")
def chain():
    from rubiks_cube_solver_amd import pattern
    return pattern.ChainTables.build(DEV)


def uniform_env(n, seed):
    from rubiks_cube_solver_amd import VecCubeEnv
    env = VecCubeEnv(n, DEV, 3, obs=None)
    env.reset_uniform(seed)
    return env


def states_of(env):
    return rows_of(env.stickers, env.num_envs)


def play(oracle, states, res):
    """The oracle's moves: res["actions"] on the states -> the states reached; every solved cube's column has exactly `length` moves."""
    acts, length = res["actions"].cpu().numpy(), res["length"].cpu().numpy()
    assert ((acts < 12).sum(axis=0) == np.maximum(length, 0)).all() and (acts <= 12).all()
    return R.walk_product(oracle, 3, states, acts.T)


def test_env_methods(oracle, pools):
    from rubiks_cube_solver_amd import VecCubeEnv
    for cs in LC.CUBE_SIZES:
        P, n = pools[cs], NMAX
        env = P.env[0].clone()
        env.compose(P.env[1])
        assert (rows_of(env.cubies(), n) == P.xy).all()
        env = P.env[0].clone()
        env.compose(P.env[1].cubies())
        assert (rows_of(env.cubies(), n) == P.xy).all()
        env = P.env[0].clone()
        env.invert()
        assert (rows_of(env.cubies(), n) == P.inv).all()
        env.compose(P.env[0])
        assert bool(env.is_solved().all())
        env.reset_uniform(12, stream_id=3, first=40)
        assert (rows_of(env.cubies(), n) == R.random_cubies(cs, 12, 3, 40, n)).all() and not bool(env.legality().any())
        # a bad byte raises and the env keeps its cubes
        before = env.stickers.clone()
        junk = env.cubies()
        junk[0, 0, 3] = 250
        with pytest.raises(ValueError):
            env.compose(junk)
        with pytest.raises(ValueError):
            env.compose(VecCubeEnv(n + 1, DEV, cs, obs=None))
        assert torch.equal(env.stickers, before)
        st = before.clone()
        st[0, 0, 2] = 7                                                      # no colour: a slot reads 0xFF
        env.stickers.copy_(st)
        with pytest.raises(ValueError):
            env.invert()
        assert torch.equal(env.stickers, st)


def test_relative_to_a_goal_by_chain_solve(oracle, chain):
    from rubiks_cube_solver_amd import search
    n = 513
    env, goal = uniform_env(n, 21), uniform_env(n, 22)
    x_before, g_before = env.stickers.clone(), goal.stickers.clone()
    rel = search.relative_to(env, goal)
    assert torch.equal(env.stickers, x_before) and torch.equal(goal.stickers, g_before)
    res = search.chain_solve(chain, rel)
    assert bool(res["solved"].all())
    assert (play(oracle, states_of(env), res) == states_of(goal)).all()
    same_goal = search.relative_to(env, goal.cubies())
    assert (states_of(same_goal) == states_of(rel)).all()                    # pad columns are nobody's
    assert bool(search.relative_to(env, env).is_solved().all())


def test_random_state_scramble(oracle, tp, chain):
    from rubiks_cube_solver_amd import search
    n = 513
    out = search.random_state_scramble(tp, chain, n, seed=31, **TP)
    drawn = rows_of(out["cubies"], n)
    assert (drawn == R.random_cubies(3, 31, 0, 0, n)).all()
    length = out["length"].cpu().numpy()
    assert (length >= 0).all()
    reached = play(oracle, oracle.solved(3, n), out)
    assert (CR.cubies(3, reached)[0] == drawn).all()
    print(f"random_state_scramble of {n} cubes: mean length {length.mean():.2f}, max {length.max()}")


def test_two_phase_solve_both(oracle, tp, chain):
    from rubiks_cube_solver_amd import search
    n = 513
    env = uniform_env(n, 41)
    before = env.stickers.clone()
    plain = search.two_phase_solve(tp, chain, env, **TP)
    both = search.two_phase_solve_both(tp, chain, env, **TP)
    assert torch.equal(env.stickers, before) and set(both) == set(plain) | {"side"}
    assert bool(both["solved"].all()) and oracle.is_solved(3, play(oracle, states_of(env), both)).all()
    lb, lp, side = both["length"].cpu().numpy(), plain["length"].cpu().numpy(), both["side"].cpu().numpy()
    assert (lb <= lp).all() and (side[lb == lp] == 0).all() and (side[lb < lp] == 1).all() and both["side"].dtype == torch.uint8
    assert torch.equal(both["actions"][:, both["side"] == 0], search._rows_to(plain["actions"], both["actions"].shape[0])[:, both["side"] == 0])
    print(f"two_phase_solve_both of {n} uniform cubes: mean {lb.mean():.2f} against {lp.mean():.2f}, the inverse side won {side.mean():.3f}")
    assert side.any()


# ------------------------------------------------------------------------------------------------------ f. capture and replay
def _s_cubes(ctx, cs, which):
    key = ("cg_cubes", cs, which)
    if key not in ctx.cache:
        seed = 5 if which == "A" else 6
        x, y = R.random_cubies(cs, seed, 1, 0, C.N), R.random_cubies(cs, seed, 2, 0, C.N)
        y[3 if which == "A" else 700, 0] = 255                               # one bad byte: the flag is written
        ctx.cache[key] = (x, y)
    return ctx.cache[key]


def _s_product(ctx, cs, variant, arena):
    n, SL = C.N, LC.SL_OF[cs]
    x, y = arena.input((C.tiles_of(n), SL, C.pitch_of(n))), arena.input((C.tiles_of(n), SL, C.pitch_of(n)))
    host = {w: [C.tiled(ctx, r, n) for r in _s_cubes(ctx, cs, w)] for w in C.SETS}
    out, bad = arena.output((C.tiles_of(n), SL, C.pitch_of(n))), arena.state((16,))

    def fill(w):
        x.copy_(host[w][0])
        y.copy_(host[w][1])
        bad.zero_()

    def check(w):
        C.same(ctx, out, n, R.product_bytes(cs, *_s_cubes(ctx, cs, w))[0], "out")
        assert bad.cpu().tolist() == [1] + [0] * 15
    return C.built(lambda: ops.group_product(x, y, n, cs, out=out, bad=bad), [fill], check)


def _s_inverse(ctx, cs, variant, arena):
    n, SL = C.N, LC.SL_OF[cs]
    x = arena.input((C.tiles_of(n), SL, C.pitch_of(n)))
    host = {w: C.tiled(ctx, _s_cubes(ctx, cs, w)[1], n) for w in C.SETS}
    out, bad = arena.output((C.tiles_of(n), SL, C.pitch_of(n))), arena.state((16,))

    def fill(w):
        x.copy_(host[w])
        bad.zero_()

    def check(w):
        C.same(ctx, out, n, R.inverse_bytes(cs, _s_cubes(ctx, cs, w)[1])[0], "out")
        assert bad.cpu().tolist() == [1] + [0] * 15
    return C.built(lambda: ops.group_inverse(x, n, cs, out=out, bad=bad), [fill], check)


def _s_random(ctx, cs, variant, arena):
    """The seed is a scalar argument, so both sets draw the same cubes: what a replay must reproduce."""
    n, SL = C.N, LC.SL_OF[cs]
    out = arena.output((C.tiles_of(n), SL, C.pitch_of(n)))
    return C.built(lambda: ops.random_cubies(n, cs, ctx.dev, seed=17, stream_id=2, first=1000, out=out), [],
                   lambda w: C.same(ctx, out, n, R.random_cubies(cs, 17, 2, 1000, n), "out"))


def _s_invert_actions(ctx, cs, variant, arena):
    n, L, A = C.N, 23, LC.A_OF[cs]
    pitch = LC.ceil16(n)
    acts = {}
    for w in C.SETS:
        rng = np.random.default_rng(90 + cs + (w == "B"))
        a = rng.integers(0, A + 1, (L, n)).astype(np.uint8)
        a[4, 11 if w == "A" else 300] = A + 2
        acts[w] = a
    src = arena.input((L, pitch))
    out, bad = arena.output((L, pitch)), arena.state((16,))

    def fill(w):
        src.fill_(A)
        src[:, :n] = ctx.torch.as_tensor(acts[w]).to(src.device)
        bad.zero_()

    def check(w):
        assert (out[:, :n].cpu().numpy() == R.invert_actions(cs, acts[w])[0]).all(), "out"
        assert bad.cpu().tolist() == [1] + [0] * 15
    return C.built(lambda: ops.invert_actions(src, n, cs, out=out, bad=bad), [fill], check)


# the form of tests/stream_cases.py ROWS, kept here: that table is pinned to the signature tables it lists
GROUP_ROWS = [C.Row("cg_product", _s_product), C.Row("cg_inverse", _s_inverse), C.Row("cg_random", _s_random),
              C.Row("cg_invert_actions", _s_invert_actions)]
GROUP_CASES = [(f"{r.label}-{cs}", r, cs) for r in GROUP_ROWS for cs in r.cube_sizes]


def test_every_launching_export_has_a_stream_row():
    assert {r.export for r in GROUP_ROWS} == set(_group_lib.GROUP_SIGNATURES)
    assert not {r.export for r in GROUP_ROWS} & {r.export for r in C.ROWS}


@pytest.fixture(scope="module")
def ctx(oracle):
    return C.Ctx(oracle, "cuda")


@pytest.mark.parametrize("row,cs", [c[1:] for c in GROUP_CASES], ids=[c[0] for c in GROUP_CASES])
def test_one_call_under_capture_and_replay(ctx, row, cs):
    from tests.test_gpu_stream_order import GraphBackend
    try:
        with torch.no_grad():
            D.run(GraphBackend(ctx.ops, ctx.L), lambda arena: row.build(ctx, cs, 0, arena))
    except Exception as e:  # noqa: BLE001
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")) and "capture" not in str(e).lower():
            pytest.exit(f"a GPU fault in this case: nothing more is started on the device -- {e}", returncode=3)
        raise
