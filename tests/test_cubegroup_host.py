"""The cg_* section of librubikhip.so and its restatement (tests/cubegroup_ref.py) without a GPU: header <-> exports <->
GROUP_SIGNATURES with every other prefix's set unchanged; THE RULE's byte formulas against sticker permutations and the oracle's
moves; the group laws; the restated generator's legality and uniformity under one fixed seed; the inverted action lists."""
import numpy as np
import pytest

from rubiks_cube_solver_amd import (_chain_lib, _cubie_lib, _edge_lib, _episode_lib, _group_lib, _ida_lib, _lib, _native,
                                    _twophase_lib)
from tests import cubegroup_ref as R
from tests import cubie_ref as C
from tests import group_ref as G
from tests.test_cubies_host import exported, prototypes

ARITY = {"cg_product": 10, "cg_inverse": 8, "cg_random": 8, "cg_invert_actions": 9}
SEED = 20261021          # the one seed of the uniformity tests; a correct generator fails a 6 sigma cap about once in 10^9
DRAWS = 1 << 20


def cap(df):
    return 6.0 * (2.0 * df) ** 0.5


def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "cg_")
    assert protos == ARITY
    L = _group_lib.group_lib()                                              # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("cg_")} == set(protos) == set(_group_lib.GROUP_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_group_lib.GROUP_SIGNATURES[fn])[0]) == n_params, fn
    others = {"rc_": ("rubikhip.h", _lib.SIGNATURES), "rcc_": ("rubikhip.h", _cubie_lib.CUBIE_SIGNATURES),
              "rce_": ("rubikhip.h", _edge_lib.EDGE_SIGNATURES), "rct_": ("rubikhip.h", _chain_lib.CHAIN_SIGNATURES),
              "ida_": ("rubikhip.h", _ida_lib.IDA_SIGNATURES), "tp_": ("rubikhip.h", _twophase_lib.TWOPHASE_SIGNATURES),
              "rcx_": ("rubikepisode.h", _episode_lib.EPISODE_SIGNATURES)}
    for prefix, (header, table) in others.items():
        assert {e for e in names if e.startswith(prefix)} == set(prototypes(header, prefix)) == set(table), prefix
        assert not set(table) & set(_group_lib.GROUP_SIGNATURES)
    assert len(prototypes("rubikhip.h", "rc_")) == 38
    assert all(e.startswith(("rc_", "rcc_", "rce_", "rcx_", "rct_")) for e in names if e.startswith("rc"))


@pytest.fixture(scope="module")
def walked(oracle):
    """{cs: (actions [2, 64, 30], cubies x [64, SLOTS], cubies y, sticker rows of x)}: two sets of 64 walks of 30 oracle moves."""
    out = {}
    for cs in (3, 2):
        rng = np.random.default_rng(70 + cs)
        acts = rng.integers(0, R.A_OF[cs], (2, 64, 30)).astype(np.uint8)
        st = [R.walk_product(oracle, cs, oracle.solved(cs, 64), a) for a in acts]
        cub = [C.cubies(cs, s)[0] for s in st]
        out[cs] = (acts, cub[0], cub[1], st[0])
    return out


@pytest.mark.parametrize("cs", (3, 2))
def test_byte_rule_equals_the_sticker_restatement(oracle, walked, cs):
    acts, x, y, x_st = walked[cs]
    by_moves = C.cubies(cs, R.walk_product(oracle, cs, x_st, acts[1]))[0]    # the oracle's moves applied to x's stickers
    by_bytes, bad = R.product_bytes(cs, x, y)
    assert not bad.any() and (by_bytes == by_moves).all() and (R.product(cs, x, y) == by_moves).all()
    inv, bad = R.inverse_bytes(cs, x)
    assert not bad.any() and (inv == R.inverse(cs, x)).all()
    assert (C.from_cubies(cs, by_bytes)[0] == R.walk_product(oracle, cs, x_st, acts[1])).all()
    # one move: the product with the cube "solved then a" is the oracle's move
    for a in range(R.A_OF[cs]):
        col = np.full(64, a, np.uint8)
        move = C.cubies(cs, oracle.step(cs, oracle.solved(cs, 64), col)[0])[0]
        assert (R.product_bytes(cs, x, move)[0] == C.cubies(cs, oracle.step(cs, x_st, col)[0])[0]).all()


@pytest.mark.parametrize("cs", (3, 2))
def test_group_laws_on_the_restatement(walked, cs):
    acts, x, y, _ = walked[cs]
    z = np.roll(x, 7, axis=0)
    P = lambda a, b: R.product_bytes(cs, a, b)[0]
    I = lambda a: R.inverse_bytes(cs, a)[0]
    e = R.identity(cs, 64)
    assert (P(P(x, y), z) == P(x, P(y, z))).all()
    assert (P(x, I(x)) == e).all() and (P(I(x), x) == e).all() and (P(x, e) == x).all() and (P(e, x) == x).all()
    assert (I(P(x, y)) == P(I(y), I(x))).all() and (I(I(x)) == x).all()
    assert not (P(x, y) == P(y, x)).all()                                   # the group is not abelian: the order of the factors shows


def test_bad_input_of_the_restatement():
    for cs in (3, 2):
        nc = R.NC_OF[cs]
        x = R.random_cubies(cs, 5, 0, 0, 8)
        y = x.copy()
        y[1, 0] = 3 * nc                                                    # no corner
        y[2, 1] = y[2, 0]                                                   # a piece twice
        if cs == 3:
            y[3, nc + 2] = 24                                               # no edge
        out, bad = R.product_bytes(cs, x, y)
        assert bad.tolist() == [False, True, False, cs == 3] + [False] * 4 and (out[bad] == R.identity(cs, 1)).all()
        assert (out[2] == R.product(cs, x[2:3], y[2:3])[0]).all()           # no permutation: the gather as written
        out, bad = R.inverse_bytes(cs, y)
        assert bad.tolist() == [False, True, True, cs == 3] + [False] * 4 and (out[bad] == R.identity(cs, 1)).all()


@pytest.fixture(scope="module")
def drawn():
    return {cs: R.random_parts(cs, SEED, 3, 0, DRAWS) for cs in (3, 2)}


@pytest.mark.parametrize("cs", (3, 2))
def test_restated_generator_draws_legal_cubes(drawn, cs):
    cp, co, ep, eo = drawn[cs]
    nc, ne = R.NC_OF[cs], R.NE_OF[cs]
    assert (np.sort(cp, axis=1) == np.arange(nc)).all() and (co.sum(axis=1) % 3 == 0).all() and ((co >= 0) & (co < 3)).all()
    if ne:
        assert (np.sort(ep, axis=1) == np.arange(ne)).all() and (eo.sum(axis=1) % 2 == 0).all()
        assert (R.perm_parity(cp) == R.perm_parity(ep)).all()
    cub = R.random_cubies(cs, SEED, 3, 0, 4096)
    assert (C.cubies(cs, C.from_cubies(cs, cub)[0])[1] == 0).all()          # status 0 by the cubie rule's own restatement
    # cube i depends on (seed, stream, first + i) alone
    assert (R.random_cubies(cs, SEED, 3, 1000, 96) == cub[1000:1096]).all()
    assert not (R.random_cubies(cs, SEED, 4, 0, 96) == cub[:96]).all() and not (R.random_cubies(cs, SEED + 1, 3, 0, 96) == cub[:96]).all()


def test_restated_generator_is_uniform_on_the_333(drawn):
    cp, co, ep, eo = drawn[3]
    n = DRAWS

    def check(index, bins, what):
        counts = np.bincount(index, minlength=bins)
        assert len(counts) == bins
        chi, df = R.chi2(counts, np.full(bins, n / bins)), bins - 1
        print(f"{what}: chi2 {chi:.1f}, df {df}, |chi2 - df| {abs(chi - df):.1f}, cap {cap(df):.1f}")
        assert abs(chi - df) <= cap(df), what

    check(R.perm_rank(cp), 40320, "corner permutation rank")
    check((co[:, :7] * 3 ** np.arange(7)).sum(axis=1), 2187, "twist word")
    check((eo[:, :11] * 2 ** np.arange(11)).sum(axis=1), 2048, "flip word")
    place = np.argsort(ep, axis=1)[:, :4]                                   # the slots that hold edge pieces 0..3
    index = np.zeros(n, np.int64)
    for k in range(4):
        index = index * (12 - k) + (place[:, k] - (place[:, :k] < place[:, k:k + 1]).sum(axis=1))
    check(index, 11880, "places of edge pieces 0..3")


@pytest.fixture(scope="module")
def distance_222(oracle):
    """int8 [3 674 160]: the 2x2x2's distance by corner_index, from the breadth-first search of tests/group_ref.py."""
    levels = G.oracle_bfs(oracle, 2, None)
    assert tuple(len(lv.states) for lv in levels) == R.SPHERES_222
    dist = np.full(sum(R.SPHERES_222), -1, np.int8)
    for lv in levels:
        _, status, cidx, _ = C.cubies(2, lv.states)
        assert (status == 0).all()
        dist[cidx] = lv.depth
    assert (dist >= 0).all()
    return dist


def test_restated_generator_is_uniform_on_the_222(drawn, distance_222):
    cp, co, _, _ = drawn[2]
    hist = np.bincount(distance_222[R.corner_index(2, cp, co)], minlength=15)
    expected = R.merged_222(R.SPHERES_222) * (DRAWS / sum(R.SPHERES_222))
    chi = R.chi2(R.merged_222(hist), expected)
    print(f"2x2x2 distance histogram: chi2 {chi:.1f}, df 11, cap {11 + cap(11):.1f}")
    assert chi <= 11 + cap(11)


@pytest.mark.parametrize("cs", (3, 2))
def test_invert_actions(oracle, cs):
    A = R.A_OF[cs]
    rng = np.random.default_rng(9)
    L, n = 13, 40
    acts = rng.integers(0, A, (L, n)).astype(np.uint8)
    acts[9:, :8] = A                                                        # no-ops at the end
    acts[3:7, 8:16] = A                                                     # in the middle
    acts[:, 16:20] = A                                                      # everywhere
    # columns 20..29 are of full length
    acts[:, 30:] = np.where(rng.random((L, 10)) < 0.4, A, acts[:, 30:])     # scattered
    inv, bad = R.invert_actions(cs, acts)
    assert not bad
    for c in range(n):
        kept = [int(a) for a in acts[:, c] if a < A]
        assert inv[:len(kept), c].tolist() == [a ^ 1 for a in reversed(kept)] and (inv[len(kept):, c] == A).all()
    assert (R.invert_actions(cs, inv)[0][:, 20:30] == acts[:, 20:30]).all()  # an involution on full columns
    # the actions, then their inverse: every cube is back where it started
    start = C.walks(oracle, cs, n, 20, 3)
    assert (R.walk_product(oracle, cs, R.walk_product(oracle, cs, start, acts.T), inv.T) == start).all()
    acts[2, 5] = A + 1
    inv2, bad = R.invert_actions(cs, acts)
    assert bad and (inv2[:, 6:] == inv[:, 6:]).all()
