"""The corner pattern database without a GPU: the three-way ABI check of the rcp_* entry points (header <-> exports <->
PATTERN_SIGNATURES), the host-only rcp_table_bytes / rcp_tables, the move rule against the sticker moves on oracle walks, the numpy
restatement (tests/pattern_ref.py) against the level counts, and the argument errors of the Python layer."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import group_ref
from tests import pattern_ref as R
from tests.cubie_ref import walks
from tests.test_symmetry_host import exported, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"rcp_table_bytes": 1, "rcp_tables": 3, "rcp_build_begin": 4, "rcp_build_level": 6, "rcp_unrank": 7, "rcp_lookup": 8,
          "rcp_score_keys": 9, "rcp_relax": 22}
# what the library exported under the older prefixes before the rcp_* section existed
RC = {"rc_search_build_id", "rc_search_last_error", "rc_search_workspace_bytes", "rc_search_init", "rc_search_expand", "rc_search_select",
      "rc_search_advance", "rc_search_backtrack"}
RCA = {"rca_workspace_bytes", "rca_init", "rca_pop", "rca_merge", "rca_backtrack"}
RCS = {"rcs_sym_count", "rcs_sym_tables", "rcs_sym_apply", "rcs_sym_canonical"}


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_exports_and_signature_table_agree():
    from rubiks_cube_solver_amd import _astar_lib, _native, _pattern_lib, _search_lib, _sym_lib
    protos = prototypes("rubiksearch.h", "rcp_")
    assert protos == PARAMS
    L = _pattern_lib.pattern_lib()                                           # loads without a GPU
    assert L is _search_lib.search_lib()                                     # the same loaded library, not a second one
    names = exported(_search_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rcp_")} == set(protos) == set(_pattern_lib.PATTERN_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_pattern_lib.PATTERN_SIGNATURES[fn])[0]) == n_params, fn
    assert not set(_pattern_lib.PATTERN_SIGNATURES) & (set(_search_lib.SIGNATURES) | set(_sym_lib.SYM_SIGNATURES) | set(_astar_lib.ASTAR_SIGNATURES))
    # the older sets are what they were
    assert {e for e in names if e.startswith("rc_")} == RC == set(prototypes("rubiksearch.h", "rc_"))
    assert {e for e in names if e.startswith("rca_")} == RCA == set(prototypes("rubiksearch.h", "rca_"))
    assert {e for e in names if e.startswith("rcs_")} == RCS == set(prototypes("rubiksym.h", "rcs_"))
    assert {e for e in names if e.startswith("rc")} == RC | RCA | RCS | set(PARAMS)


def test_generated_header_is_current():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"]).returncode == 0


def test_table_bytes():
    from rubiks_cube_solver_amd import _pattern_lib
    assert _pattern_lib.table_bytes(3) == 88179840 == 40320 * 3 ** 7 == R.SIZE[3]
    assert _pattern_lib.table_bytes(2) == 3674160 == 5040 * 3 ** 6 == R.SIZE[2] == group_ref.GROUP_222
    L = _pattern_lib.pattern_lib()
    for cs in (0, 1, 4, -3):
        assert L.rcp_table_bytes(cs) == -1
        with pytest.raises(NotImplementedError):
            _pattern_lib.table_bytes(cs)


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("cs", (2, 3))
def test_move_tables_three_ways(cs):
    """rcp_tables (what the kernels were compiled with) = tables.get_corner_moves (what the header is generated from) = the
    restatement's derivation from sticker positions; each row is a permutation whose twists sum to 0 mod 3."""
    from rubiks_cube_solver_amd import _pattern_lib, _search_lib
    from rubiks_cube_solver_amd.tables import get_corner_moves
    lib, gen, ref = _pattern_lib.tables(cs), get_corner_moves(cs), R.corner_moves(cs)
    A, NC = (12, 8) if cs == 3 else (6, 7)
    for got in (lib, gen):
        for x, y in zip(got, ref):
            assert x.shape == (A, NC) and x.dtype == np.uint8 and (x == y).all()
    src, twist = ref
    assert (np.sort(src, 1) == np.arange(NC)).all() and (twist.sum(1) % 3 == 0).all() and twist.max() <= 2
    for a in range(A):                                                       # a ^ 1 undoes a
        assert (src[a][src[a ^ 1]] == np.arange(NC)).all() and ((twist[a][src[a ^ 1]] + twist[a ^ 1]) % 3 == 0).all()
    L = _pattern_lib.pattern_lib()
    assert L.rcp_tables(cs, None, None) == 0                                 # either pointer may be NULL
    assert L.rcp_tables(4, None, None) == -1 and b"cube_size" in L.rc_search_last_error()
    with pytest.raises(NotImplementedError):
        _pattern_lib.tables(5)
    assert _search_lib.search_lib() is L


@pytest.mark.parametrize("cs", (2, 3))
def test_move_rule_equals_the_sticker_moves(oracle, cs):
    """THE RULE's move on (piece, ori) = the oracle's move on stickers, read back through the cubie rule: every move, from states 30
    oracle moves deep (and from the solved cube), and the index of the result is the index of the moved coordinates."""
    src, twist = R.corner_moves(cs)
    A = 12 if cs == 3 else 6
    st = np.concatenate([oracle.solved(cs, 1), walks(oracle, cs, 300, 30, seed=cs)])
    piece, ori, idx = R.coords(cs, st)
    assert (R.rank(piece, ori) == idx).all() and (idx < R.SIZE[cs]).all()
    for a in range(A):
        child = oracle.step(cs, st, np.full(len(st), a, np.uint8))[0]
        cp, co, cidx = R.coords(cs, child)
        mp, mo = R.move_coords(piece, ori, src, twist, a)
        assert (mp == cp).all() and (mo == co).all() and (R.rank(mp, mo) == cidx).all(), a


def test_restatement_reproduces_the_level_counts():
    """The sticker search: the 3x3x3 corner projection to depth 6 gives the first seven committed counts.  (The whole 2x2x2 group is
    searched by the GPU suite's session fixture, where its table is compared entry by entry.)"""
    dist, levels = R.bfs(3, 6)
    assert levels == R.LEVELS_333[:7]
    assert tuple(np.bincount(dist[dist != R.ILLEGAL], minlength=7)) == R.LEVELS_333[:7] and dist[0] == 0
    assert len(R.LEVELS_333) == 15 and len(group_ref.SPHERES_222) == 15


def test_corner_index_of_the_restatement(oracle):
    """pattern_ref.corner_index, the reference of rcp_lookup / rcp_score_keys: the cubie rule's corner_index on legal cubes; on the
    3x3x3 edge trouble does not matter, corner trouble does."""
    from rubiks_cube_solver_amd.tables import get_cubies
    for cs in (2, 3):
        st = walks(oracle, cs, 64, 20, seed=7)
        want = get_cubies(cs).cubies(st)[2]
        assert (R.corner_index(cs, st) == want).all()
        cb = get_cubies(cs)
        bad = st.copy()
        bad[0, cb.corner_cw[0][0]] = 6                                       # no colour
        bad[1, cb.corner_cw[1]] = bad[1, np.roll(cb.corner_cw[1], 1)]        # a twisted corner
        bad[2, cb.corner_cw[2]] = bad[2, cb.corner_cw[3]]                    # a repeated piece
        got = R.corner_index(cs, bad)
        assert (got[:3] == 0xFFFFFFFF).all() and (got[3:] == want[3:]).all()
        if cs == 3:
            e = st.copy()
            e[:, cb.edge_facelets[0]] = e[:, cb.edge_facelets[0][::-1]]      # a flipped edge: RCC_FLIP for the cube, nothing for the corners
            e[1, 4] = 7                                                      # a centre that is no colour
            assert (cb.cubies(e)[1] != 0).all() and (R.corner_index(3, e) == want).all()


# ------------------------------------------------------------------------------------------------------------ the relax scenario
def scenario_roots(case):
    from tests import beam_ref
    from tests.test_gpu_search import scrambles
    return beam_ref.Cube(case.cs).scramble(scrambles(case.cs, R.scenario_depths(case.P), seed=R.SEEDS[case.cs]))


@pytest.mark.parametrize("case", R.scenario_cases(max_P=5), ids=R.case_id)
def test_relax_scenario_reaches_its_cases(case):
    """"Flood, lift, re-open" (tests/pattern_ref.py) on the restatement alone, at every point of tests/test_gpu_relax.py with P <= 5:
    the case each point exists for occurs -- contested nodes, ties on g, winners that are not the lowest c, offers from different
    strides, winners at c >= 256, dropped NEW candidates and their duplicates, a priority an fma would round otherwise."""
    st = R.run_scenario(case, scenario_roots(case))
    R.check_reached(case, st)
    if (case.P, case.B, case.weight, case.C) == (3, 64, 1.0, 1 + 64 * (11 if case.cs == 3 else 5) * 8):
        # one problem of three is deep here; with three deep roots the counters are three times these
        want = {(3, True): (533, 63, 28, 36, 18, 7, 354, 0), (3, False): (626, 88, 88, 0, 0, 11, 412, 0),
                (2, True): (248, 19, 0, 19, 11, 1, 78, 0), (2, False): (293, 28, 28, 0, 0, 1, 97, 0)}[case.cs, case.jitter]
        assert tuple(st.counters().values()) == want


def test_relaxed_step_is_merge_then_relax():
    """The split restatement: relaxed_step (merge, then relax as a stage of its own) leaves what the inherited rule leaves wherever
    nothing is relaxed, and a node it lowers holds the least g, then the least c, of its offers."""
    from tests import astar_ref, beam_ref
    case = R.Case(3, 3, 4, 1 + 4 * 11 * 8, 1.0, None, True)
    cube, roots = beam_ref.Cube(3), scenario_roots(case)
    st, plain = R.relaxed_class()(cube, roots, 4, case.C), astar_ref.AStar(cube, roots, 4, case.C)
    for _ in range(6):
        R.relaxed_step(st, lambda states: np.zeros(len(states), np.float32))
        plain.pop(), plain.expand()
        plain.merge(R.zero_scores(plain))
    assert st.relaxed == 0
    for name in ("g", "parent", "action", "prio", "state", "count", "pop_node", "live", "active"):
        assert (getattr(st, name) == getattr(plain, name)).all(), name
    R.doctor(st)
    before = st.g.copy()
    R.relaxed_step(st, lambda states: np.zeros(len(states), np.float32))
    low = np.flatnonzero(st.g < before)
    assert len(low) == st.relaxed > 0
    p = 2                                                                    # the deep root
    par = st.pop_node[p * 4 + st.cand[p]["i"]]
    for gid in low:
        n = gid - p * case.C
        offers = sorted((int(st.g[p * case.C + par[c]]) + 1, int(c)) for c in range(len(par))
                        if st.cand[p]["valid"][c] and st.known[p][st.cand[p]["keys"][:, c].tobytes()] == n)
        g, c = offers[0]
        assert (st.g[gid], st.parent[gid], st.action[gid]) == (g, par[c], st.cand[p]["a"][c]) and st.prio[gid] == np.float32(-g)


# ------------------------------------------------------------------------------------------------------------ python errors
def test_argument_errors_come_before_any_device_use():
    """front="table" and the CornerTable constructor: every ValueError with a device name torch does not know, an env without stickers,
    or host tensors -- nothing can have touched a device."""
    import torch
    from rubiks_cube_solver_amd import CornerTable, pattern, search
    assert CornerTable is pattern.CornerTable
    n2 = R.SIZE[2]
    for table, cs in ((torch.zeros(n2, dtype=torch.uint8), 2),               # a host tensor
                      (torch.zeros(n2, dtype=torch.int8), 2), (torch.zeros(n2 - 1, dtype=torch.uint8), 2), (torch.zeros(n2, dtype=torch.uint8), 3),
                      (torch.zeros((1, n2), dtype=torch.uint8), 2), (torch.zeros(2 * n2, dtype=torch.uint8)[::2], 2), (np.zeros(n2, np.uint8), 2),
                      (torch.zeros(n2, dtype=torch.uint8), 4)):
        with pytest.raises(ValueError):
            CornerTable(table, cs)
    dev = "no-such-device"
    with pytest.raises(ValueError, match="'table'"):                         # the message names the third front
        search.BeamPlan(2, 2, 4, 3, dev, front="tables")
    with pytest.raises(ValueError):
        search.AStarPlan(2, 2, 4, 10, dev, front="tables")
    env = types.SimpleNamespace(num_envs=3, cube_size=2)                     # no stickers, no device: reading either would raise
    fake = object.__new__(CornerTable)                                       # a table of the OTHER cube size, never on a device
    fake.cube_size, fake.device = 3, torch.device("cuda", 0)
    for model in (object(), torch.nn.Linear(2, 1), None, fake):
        with pytest.raises(ValueError):
            search.beam_search(model, env, 4, 3, front="table")
        with pytest.raises(ValueError):
            search.astar_search(model, env, 4, 3, front="table")
        with pytest.raises(ValueError):
            search.beam_search_symmetric(model, env, 4, 3, symmetries=[0], front="table")
        with pytest.raises(ValueError):
            search.beam_solve_percentage(model, 2, 2, 2, 4, 3, device=dev, front="table")
        with pytest.raises(ValueError):
            search.astar_solve_percentage(model, 2, 2, 2, 4, 3, device=dev, front="table")
    fake.cube_size = 2                                                       # the right size on another device
    env = types.SimpleNamespace(num_envs=3, cube_size=2, stickers=types.SimpleNamespace(device=torch.device("cuda", 1)))
    with pytest.raises(ValueError, match="cuda:0"):
        search.astar_search(fake, env, 4, 3, front="table")
    with pytest.raises(ValueError, match="cuda:0"):
        search.beam_search(fake, env, 4, 3, front="table")
    with pytest.raises(ValueError):
        fake.distance(types.SimpleNamespace(stickers=None, cube_size=3, num_envs=1))
    with pytest.raises(ValueError):                                          # the existing fronts still refuse what they refused
        search.beam_search(object(), env, 4, 3, front="sparse")
