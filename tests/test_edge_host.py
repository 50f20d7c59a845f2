"""The rce_* section of librubikhip.so and its restatement without a GPU: header <-> exports <-> EDGE_SIGNATURES, the move tables
derived three ways, the move rule against the oracle, rank / unrank, the level counts of the small tables, and the Python layer's
argument errors."""
import os

import numpy as np
import pytest

from rubiks_cube_solver_amd import _edge_lib, _lib, _native, tables
from tests import edge_ref as R
from tests.test_cubies_host import exported, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"rce_table_bytes": 1, "rce_home_index": 1, "rce_tables": 2, "rce_build_begin": 4, "rce_build_level": 6, "rce_unrank": 7,
         "rce_lookup": 8, "rce_score_codes": 10}


def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "rce_")
    assert protos == ARITY
    L = _edge_lib.edge_lib()                                                # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rce_")} == set(protos) == set(_edge_lib.EDGE_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_edge_lib.EDGE_SIGNATURES[fn])[0]) == n_params, fn
    from rubiks_cube_solver_amd import _cubie_lib
    assert not set(_edge_lib.EDGE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_cubie_lib.CUBIE_SIGNATURES))


def test_move_tables_three_ways():
    """tables.get_edge_moves (what the header is generated from), rce_tables (what the library was compiled with) and the
    restatement's derivation from where each move carries each edge sticker."""
    mine, theirs, ref = tables.get_edge_moves(), _edge_lib.tables(), R.edge_moves(tables.get_tables(3).perm)
    for a, b, c in zip(mine, theirs, ref):
        assert a.shape == (12, 12) and (a == b).all() and (a == c).all()
    src = open(os.path.join(ROOT, "rubiks-cube-solver_amd", "csrc", "rc_tables.h")).read()
    assert "emove_src[12][12]" in src and "emove_flip[12][12]" in src
    esrc, eflip = ref
    for a in range(12):                                                     # a permutation of the slots; a quarter turn and its inverse undo each other
        assert sorted(esrc[a]) == list(range(12))
        assert (esrc[a][esrc[a ^ 1]] == np.arange(12)).all() and ((eflip[a][esrc[a ^ 1]] ^ eflip[a ^ 1]) == 0).all()


def test_sizes_and_home_indices():
    for mask in R.SMALL_MASKS + (R.LOW6, R.HIGH6, 0x0FE, 0xAA5):
        k = len(R.pieces(mask))
        assert _edge_lib.table_bytes(mask) == R.size(k) and _edge_lib.home_index(mask) == R.home_index(mask)
        assert _edge_lib.edge_mask(R.pieces(mask)) == mask
    assert R.home_index(0x001) == 0 and R.home_index(R.HIGH6) != 0          # home is not index 0 in general
    L = _edge_lib.edge_lib()
    for bad in (0, 0x0FF, 0x1000, 0x1001, -1):                              # no piece, k = 8, bits above 11
        assert L.rce_table_bytes(bad) == -1 and L.rce_home_index(bad) == -1
        with pytest.raises(ValueError):
            _edge_lib.edge_mask(bad)
    for bad in ([], [12], [0, 0], [-1], range(8)):
        with pytest.raises(ValueError):
            _edge_lib.edge_mask(bad)


def test_move_rule_equals_the_oracle_on_walks(oracle):
    """30-move walks: the pattern moved by THE RULE = the pattern read from the oracle's stickers, for every mask, at every step."""
    esrc, eflip = tables.get_edge_moves()
    rng = np.random.default_rng(17)
    n = 24
    st = oracle.solved(3, n)
    masks = R.SMALL_MASKS + (R.LOW6, R.HIGH6, 0x0FE)
    state = {m: [R.unrank(len(R.pieces(m)), R.home_index(m)) for _ in range(n)] for m in masks}
    for _ in range(30):
        acts = rng.integers(0, 12, n).astype(np.uint8)
        st = oracle.step(3, st, acts)[0]
        for m in masks:
            state[m] = [R.move(esrc, eflip, int(a), *s) for a, s in zip(acts, state[m])]
            assert [R.rank(*s) for s in state[m]] == R.index_of_states(m, st).tolist()


@pytest.mark.parametrize("mask", R.SMALL_MASKS)
def test_rank_unrank_and_cubies_at_every_index(mask):
    """rank(unrank(i)) == i at every index; the unranked cube is reachable (cubie_ref status 0) and reads back as i."""
    from tests import cubie_ref
    k = len(R.pieces(mask))
    N = R.size(k)
    for i in range(N):
        pos, ori = R.unrank(k, i)
        assert len(set(pos)) == k and R.rank(pos, ori) == i
    idx = np.arange(N) if N <= 10560 else np.arange(3, N, 37)
    cub, bad = R.unrank_cubies(mask, idx)
    assert not bad.any() and (R.index_of_bytes(mask, cub[:, 8:]) == idx).all()
    st, flagged = cubie_ref.from_cubies(3, cub)
    assert not flagged.any() and not cubie_ref.cubies(3, st)[1].any()
    assert (R.index_of_states(mask, st) == idx).all()
    solved, bad = R.unrank_cubies(mask, [N, R.home_index(mask)])
    assert bad.tolist() == [True, False] and (solved == np.array([3 * q for q in range(8)] + [2 * q for q in range(12)])).all()


@pytest.mark.parametrize("mask", R.SMALL_MASKS)
def test_level_counts_of_the_small_tables(mask):
    table, levels = R.small(mask)
    N = R.size(len(R.pieces(mask)))
    assert len(table) == N and sum(levels) == N and levels[0] == 1 and table[R.home_index(mask)] == 0
    assert tuple(np.bincount(table)) == levels and (table == 0).sum() == 1


def test_illegal_rows_of_the_restatement():
    home = np.array([[2 * q for q in range(12)]], np.uint8)
    for mask in (0x001, 0x801, R.LOW6):
        assert R.index_of_bytes(mask, home)[0] == R.home_index(mask)
        e = home.copy(); e[0, 11] = 24                                      # a byte >= 24, in a slot that holds no tracked piece of 0x001
        assert R.index_of_bytes(mask, e)[0] == 0xFFFFFFFF
        e = home.copy(); e[0, 5] = 0                                        # piece 0 twice (piece 5 absent)
        assert R.index_of_bytes(mask, e)[0] == 0xFFFFFFFF
        e = home.copy(); e[0, 0] = 2 * 9                                    # piece 0 absent (piece 9 twice, untracked in all three)
        assert R.index_of_bytes(mask, e)[0] == 0xFFFFFFFF
    e = home.copy(); e[0, 9] = 2 * 10                                       # an untracked piece twice, another absent: not looked at
    assert R.index_of_bytes(R.LOW6, e)[0] == R.home_index(R.LOW6)


def test_python_argument_errors_come_before_any_device_use():
    import torch
    from rubiks_cube_solver_amd import pattern
    import rubiks_cube_solver_amd as rc
    assert rc.EdgeTable is pattern.EdgeTable and rc.MaxTable is pattern.MaxTable
    with pytest.raises(ValueError):
        pattern.EdgeTable.build([0, 1], "cuda", cube_size=2)                # the 2x2x2 has no edges
    with pytest.raises(ValueError):
        pattern.EdgeTable(torch.zeros(24, dtype=torch.uint8), [0], cube_size=2)
    for edges in ([], range(8), [12], 0, 0x1000):
        with pytest.raises(ValueError):
            pattern.EdgeTable.build(edges, "cuda")
    for t in (torch.zeros(23, dtype=torch.uint8), torch.zeros(24, dtype=torch.int8), torch.zeros((24, 1), dtype=torch.uint8), [0] * 24,
              torch.zeros(24, dtype=torch.uint8)):                          # the last: right size, but no HIP device
        with pytest.raises(ValueError):
            pattern.EdgeTable(t, [0])
    for members in ((None,), ("x",), (None, "x"), (torch.zeros(3),)):
        with pytest.raises(ValueError):
            pattern.MaxTable(*members)
    from rubiks_cube_solver_amd import search
    with pytest.raises(ValueError):
        search._check_table("x", 3)
