"""The rct_* section of librubikhip.so and its restatement without a GPU: header <-> exports <-> CHAIN_SIGNATURES with the other
prefixes' sets unchanged, the generated data three ways, the level counts of all four stages by the restated search, the committed
tables of stages 0, 1 and 3 (tests/golden/chain_tables.npz, what the GPU tests compare the built tables with), rank o unrank, the
plain-loop descent on 200 oracle walks, and the Python layer's argument errors."""
import os

import numpy as np
import pytest

from rubiks_cube_solver_amd import _chain_lib, _cubie_lib, _edge_lib, _episode_lib, _lib, _native, tables
from tests import chain_ref as R
from tests.test_cubies_host import exported, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"rct_table_bytes": 1, "rct_generators": 3, "rct_corner_cosets": 1, "rct_build_begin": 4, "rct_build_level": 6, "rct_index": 6,
         "rct_unrank": 7, "rct_descend": 13}


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "chain_tables.npz"))


def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "rct_")
    assert protos == ARITY
    L = _chain_lib.chain_lib()                                              # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rct_")} == set(protos) == set(_chain_lib.CHAIN_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_chain_lib.CHAIN_SIGNATURES[fn])[0]) == n_params, fn
    # the other prefixes of the library: what their own signature tables list, no more and no less
    others = {"rc_": ("rubikhip.h", _lib.SIGNATURES), "rcc_": ("rubikhip.h", _cubie_lib.CUBIE_SIGNATURES),
              "rce_": ("rubikhip.h", _edge_lib.EDGE_SIGNATURES), "rcx_": ("rubikepisode.h", _episode_lib.EPISODE_SIGNATURES)}
    for prefix, (header, table) in others.items():
        assert {e for e in names if e.startswith(prefix)} == set(prototypes(header, prefix)) == set(table), prefix
        assert not set(table) & set(_chain_lib.CHAIN_SIGNATURES)
    assert len(prototypes("rubikhip.h", "rc_")) == 38
    assert all(e.startswith(("rc_", "rcc_", "rce_", "rcx_", "rct_")) for e in names if e.startswith("rc"))


def test_generated_data_three_ways():
    """tables.get_chain (what the header is generated from), rct_generators / rct_corner_cosets (what the library was compiled with)
    and the restatement's lists and its closure under the oracle's half turns."""
    ch = tables.get_chain()
    h = R.corner_cosets()[0]
    assert len(h) == 96 and h[0] == 0 and (np.diff(h) > 0).all()
    assert (ch.corner_cosets == h).all() and (_chain_lib.corner_cosets() == h).all() and ch.corner_cosets.dtype == np.uint16
    for stage in range(4):
        want = np.array([(g[0], g[1] if len(g) == 2 else 0xFF) for g in R.GENERATORS[stage]], np.uint8)
        assert (ch.generators[stage] == want).all() and (_chain_lib.generators(stage) == want).all(), stage
        assert _chain_lib.table_bytes(stage) == R.SIZE[stage] == ch.sizes[stage]
        codes = ch.gen_codes[stage]
        assert (codes[:len(want)] == want[:, 0] + 16 * (want[:, 1] != 0xFF)).all() and (codes[len(want):] == 0xFF).all()
    L = _chain_lib.chain_lib()
    assert L.rct_table_bytes(-1) == -1 and L.rct_table_bytes(4) == -1 and L.rct_generators(4, None, None) == -1
    assert b"stage" in L.rc_last_error()
    assert (_chain_lib.MAX_GENERATORS, _chain_lib.MAX_LENGTH) == (R.MAX_GENERATORS, R.MAX_LENGTH) == (47, 87)


def test_which_moves_change_an_orientation():
    """The facts the chain rests on, from the oracle: only F, F', B, B' change an edge ori bit; every quarter turn but U, U', D, D'
    changes a corner ori."""
    solved = tables.get_tables(3).solved[None, :]
    for a in range(12):
        _, co, _, eo, _ = R.coords(R.move(solved, (a,)))
        assert bool(eo.any()) == (a in (R.F, R.F_, R.B, R.B_)) and bool(co.any()) == (a not in (R.U, R.U_, R.D, R.D_)), a


@pytest.mark.parametrize("stage", (0, 3, 1, 2))
def test_restated_search_reproduces_the_level_counts(stage):
    """Breadth-first on sticker arrays under the stage's generators (stage 1: 45 s, stage 2: 90 s of numpy).  Stages 0, 1 and 3: the
    committed tables are this search's, byte for byte."""
    dist, levels = R.bfs(stage)
    assert levels == R.LEVELS[stage] and len(dist) == R.SIZE[stage]
    assert tuple(np.bincount(dist[dist != R.NONE])) == levels
    assert (np.flatnonzero(dist == 0) == R.goal_indices(stage)).all() and len(R.goal_indices(stage)) == levels[0]
    assert (dist == R.NONE).sum() == (R.SIZE[3] // 2 if stage == 3 else 0)
    if stage != 2:
        assert (golden()[f"stage{stage}"] == dist).all()


def test_goal_entries():
    assert R.goal_indices(0).tolist() == [0] and R.goal_indices(1).tolist() == [494 * 2187] and R.goal_indices(3).tolist() == [0]
    assert (R.goal_indices(2) == R.corner_cosets()[0] + 40320 * R.E_HOME).all()


@pytest.mark.parametrize("stage", range(4))
def test_rank_unrank(stage):
    """index(unrank(i)) == i at every index of stages 0 and 3 and on a stride of stages 1 and 2; the unranked cube is reachable
    (status 0 of the cubie rule); a stage-3 index is flagged exactly where the committed table holds 0xFF."""
    cb = tables.get_cubies(3)
    N = R.SIZE[stage]
    idx = np.arange(N) if stage in (0, 3) else np.concatenate([np.arange(0, N, 61), [N - 1]])
    rows, bad = R.unrank(stage, idx)
    if stage == 3:
        assert (bad == (golden()["stage3"] == R.NONE)).all() and bad.sum() == N // 2
    else:
        assert not bad.any()
    st = cb.from_cubies(rows)[0]
    assert (cb.cubies(st)[1] == 0).all()
    back = R.index_rows(stage, rows).astype(np.int64)
    assert (back[~bad] == idx[~bad]).all() and (back[bad] == (0 if stage != 1 else 494 * 2187)).all()
    rows, bad = R.unrank(stage, np.array([N, -1, N + 5]))
    assert bad.all() and (rows == R.HOME_ROWS).all()


def test_index_outside_the_domains():
    """One flipped edge, one twisted pair, a slice edge out of its slice, a corner permutation outside H, a byte >= 24, a piece twice."""
    home = R.HOME_ROWS
    def rows(**kw):
        r = home.copy()
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r
    flipped = rows(s8=1, s9=3)                                               # edges 0 and 1 flipped: legal, outside stages 1..3
    twisted = rows(s0=1, s1=3 + 2)                                           # corner 0 twisted +1, corner 1 twisted -1
    sliced = rows(s8=2 * 8, s16=0)                                           # slice piece 8 in slot 0, piece 0 in slot 8
    quarter = tables.get_cubies(3).cubies(R.move(tables.get_tables(3).solved[None, :], (R.U,)))[0][0]   # U: in stage 2's domain, outside H
    big, twice = rows(s12=24), rows(s9=0)
    signed = lambda v: -1 if int(v) == 0xFFFFFFFF else int(v)
    got = {name: [signed(R.index_rows(s, r[None, :])[0]) for s in range(4)]
           for name, r in dict(flipped=flipped, twisted=twisted, sliced=sliced, quarter=quarter, big=big, twice=twice).items()}
    assert got["flipped"] == [3, -1, -1, -1]
    assert got["twisted"][0] == 0 and got["twisted"][1] == 494 * 2187 + 1 + 2 * 3 and got["twisted"][2:] == [-1, -1]
    assert got["sliced"][0] == 0 and got["sliced"][1] >= 0 and got["sliced"][1] != 494 * 2187 and got["sliced"][2:] == [-1, -1]
    assert got["quarter"][:2] == [0, 494 * 2187] and got["quarter"][2] >= 0 and got["quarter"][3] == -1
    assert got["big"] == [-1] * 4 and got["twice"] == [-1] * 4


def test_plain_loop_descent_solves_200_walks():
    """200 oracle walks of 100 moves through the committed tables (stage 2's from the restated search, which the level test also runs):
    every cube solved at exactly `length`, each stage's output in the next stage's domain, the bounds of the depths hold."""
    g = golden()
    tabs = [g["stage0"], g["stage1"], R.bfs(2)[0], g["stage3"]]
    states, _ = R.scramble(200, 100, 7)
    length, actions, moves, status = R.solve(tabs, states)
    assert not status.any() and (moves != R.NONE).all()
    assert (moves <= np.array(R.DEPTH)[:, None]).all() and (moves.astype(int).sum(0) <= R.MAX_GENERATORS).all()
    assert (length <= R.MAX_LENGTH).all() and (length >= moves.astype(int).sum(0)).all() and (length <= moves[0] + 2 * moves[1:].astype(int).sum(0)).all()
    solved = tables.get_tables(3).solved
    assert (R.replay(states, actions) == solved).all()
    for c in range(0, 200, 23):                                              # exactly at `length`: one move earlier the cube is not solved
        assert (actions[length[c]:, c] == R.NOOP).all() and (actions[:length[c], c] < 12).all()
        assert length[c] == 0 or (R.replay(states[c:c + 1], actions[:length[c] - 1, c:c + 1]) != solved).any()
    # stage by stage: the rows one descent leaves are in the next one's domain, and at its goal
    rows = tables.get_cubies(3).cubies(states[:16])[0]
    acts, ln = np.full((R.MAX_LENGTH, 16), R.NOOP, np.uint8), np.zeros(16, np.int32)
    for stage in range(4):
        rows, acts, ln, mv, st = R.descend(stage, tabs[stage], rows, acts, ln, R.MAX_LENGTH)
        assert not st.any() and (R.table_at(tabs[stage], R.index_rows(stage, rows).astype(np.int64)) == 0).all()
        if stage < 3:
            assert (R.index_rows(stage + 1, rows) != 0xFFFFFFFF).all()
    assert (rows == R.HOME_ROWS).all()
    # the status bytes
    rows = tables.get_cubies(3).cubies(states[:4])[0]
    rows[1, 3] = 24
    rows[2, 9] = rows[2, 8]
    out = R.descend(0, tabs[0], rows, acts, np.array([0, 0, 0, 85], np.int32), R.MAX_LENGTH)
    assert out[4].tolist() == [0, R.ILLEGAL, R.ILLEGAL, R.NO_ROOM if out[3][3] > 1 else 0] and out[3][1] == out[3][2] == R.NONE
    assert R.descend(1, tabs[1], rows[:1], acts, ln[:1], R.MAX_LENGTH)[4].tolist() == [R.OUTSIDE]
    stuck = R.descend(0, tabs[2], rows[:1], acts, np.zeros(1, np.int32), R.MAX_LENGTH)   # a foreign table: ends, says so
    assert stuck[4][0] in (R.STUCK, R.OUTSIDE, 0)


def test_python_argument_errors_come_before_any_device_use():
    import torch
    import rubiks_cube_solver_amd as rc
    from rubiks_cube_solver_amd import pattern, search
    assert rc.ChainTables is pattern.ChainTables and rc.chain_solve is search.chain_solve
    with pytest.raises(ValueError):
        pattern.ChainTables.build("cuda", cube_size=2)
    good = [torch.zeros(n, dtype=torch.uint8) for n in R.SIZE]              # right sizes, but no HIP device
    for tabs in (good, good[:3], [t.to(torch.int8) for t in good], [good[0], good[1], good[2], torch.zeros(5, dtype=torch.uint8)], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            pattern.ChainTables(tabs)
    with pytest.raises(ValueError):
        pattern.ChainTables(good, cube_size=2)
    for stage in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError):
            _chain_lib.check_stage(stage)

    class Env2:
        cube_size, stickers, num_envs = 2, torch.zeros(1), 1
    for tabs in ("x", None):
        with pytest.raises(ValueError):
            search.chain_solve(tabs, Env2())
    chain = pattern.ChainTables.__new__(pattern.ChainTables)                # no device needed to be refused
    chain.device = torch.device("cpu")
    with pytest.raises(ValueError):
        search.chain_solve(chain, Env2())
    with pytest.raises(ValueError):
        chain.index(Env2(), 0)
    with pytest.raises(ValueError):
        search.chain_solve(chain, "x")
