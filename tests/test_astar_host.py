"""Batch-weighted A* without a GPU: the three-way ABI check of the rca_* entry points (header <-> exports <-> ASTAR_SIGNATURES), the
host-only rca_workspace_bytes, the argument errors of the Python layer, and the numpy restatement (tests/astar_ref.py) against the
2x2x2 group's own distances.  Every comparison is exact."""
import types

import numpy as np
import pytest

from tests import astar_ref as R
from tests import group_ref as G
from tests.beam_ref import Cube
from tests.test_symmetry_host import exported, prototypes

PARAMS = {"rca_workspace_bytes": 3, "rca_init": 24, "rca_pop": 19, "rca_merge": 32, "rca_backtrack": 10}


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_exports_and_signature_table_agree():
    from rubiks_cube_solver_amd import _astar_lib, _native, _search_lib, _sym_lib
    protos = prototypes("rubiksearch.h", "rca_")
    assert protos == PARAMS
    L = _astar_lib.astar_lib()                                               # loads without a GPU
    assert L is _search_lib.search_lib() and L is _sym_lib.sym_lib()         # the same loaded library, not a second one
    names = exported(_search_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rca_")} == set(protos) == set(_astar_lib.ASTAR_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_astar_lib.ASTAR_SIGNATURES[fn])[0]) == n_params, fn
    assert not set(_astar_lib.ASTAR_SIGNATURES) & (set(_search_lib.SIGNATURES) | set(_sym_lib.SYM_SIGNATURES))
    assert (_astar_lib.OPEN, _astar_lib.CLOSED, _astar_lib.NEW) == (R.OPEN, R.CLOSED, R.NEW)


def test_an_extension_names_what_the_library_lacks():
    """_native.extension, the loader behind astar_lib / sym_lib / episode_lib: a signature table with a function the library does
    not export raises, naming that function (and no other) and the library's path; the real loaders all hand out ONE object."""
    from rubiks_cube_solver_amd import _astar_lib, _native, _search_lib, _sym_lib
    loader = _native.extension(_search_lib.search_lib, {**_astar_lib.ASTAR_SIGNATURES, "rca_no_such_function": []}, "search")
    for _ in range(2):                                                       # a failed call leaves nothing behind
        with pytest.raises(_native.RubikHipError) as e:
            loader()
        assert "rca_no_such_function" in str(e.value) and _search_lib.LIB_PATH in str(e.value) and "rca_init" not in str(e.value)
    L = _search_lib.search_lib()
    assert _astar_lib.astar_lib() is L and _sym_lib.sym_lib() is L and _astar_lib.astar_lib() is _astar_lib.astar_lib()


def test_workspace_bytes():
    from rubiks_cube_solver_amd import _astar_lib
    wb = _astar_lib.workspace_bytes
    for cs in (2, 3):
        assert wb(cs, 1, 1) == 1024 * 8                                      # the smallest table
        assert wb(cs, 1, 512) == 1024 * 8 and wb(cs, 1, 513) == 2048 * 8     # a power of two of slots >= 2 * P * C
        assert wb(cs, 40, 5000) == (1 << 19) * 8 and wb(cs, 1000, 100000) == (1 << 28) * 8
        for P, C in ((3, 7), (1, 1 << 20), (1 << 10, 1 << 10), (7, 300000000)):
            slots = wb(cs, P, C) // 8
            assert slots & (slots - 1) == 0 and 2 * P * C <= slots < max(4 * P * C, 2048)
        assert wb(cs, 1, (1 << 31) - 1) == (1 << 32) * 8
        for P, C in ((0, 1), (1, 0), (-1, 5), (1, 1 << 31), (1 << 31, 1), (1 << 16, 1 << 15), (2, 1 << 30)):
            assert wb(cs, P, C) == -1, (P, C)
    assert wb(4, 1, 1) == -1 and wb(0, 1, 1) == -1


def test_argument_errors_come_before_any_device_use():
    """Every ValueError is raised with a device name torch does not know and an env without stickers: nothing can have touched a device."""
    from rubiks_cube_solver_amd import search
    dev = "no-such-device"                                                   # torch.device(dev) itself would raise RuntimeError
    ok = dict(n_problems=2, cube_size=3, batch=4, capacity=10, device=dev)
    for bad in (dict(batch=0), dict(batch=65537), dict(n_problems=0), dict(capacity=0), dict(n_problems=1 << 16, capacity=1 << 15),
                dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-0.5), dict(cube_size=4), dict(front="sparse"),
                dict(front="codes"), dict(front="codes", hidden=64, dtype=__import__("torch").float16)):
        with pytest.raises(ValueError):
            search.AStarPlan(**{**ok, **bad})
    env = types.SimpleNamespace(num_envs=3, cube_size=2)                     # no stickers, no device: reading either would raise
    model = object()
    for bad in (dict(batch=0), dict(batch=1 << 17), dict(max_iterations=-1), dict(sync_every=0), dict(weight=float("nan")),
                dict(weight=-1.0), dict(weight=float("inf")), dict(front="onehot"), dict(capacity=0), dict(capacity=1 << 30)):
        kw = {**dict(batch=4, max_iterations=3), **bad}
        with pytest.raises(ValueError):
            search.astar_search(model, env, kw.pop("batch"), kw.pop("max_iterations"), **kw)


def test_default_capacity():
    from rubiks_cube_solver_amd import search
    assert search.astar_capacity(10, 3, 16, 5) == 1 + 16 * 11 * 5 and search.astar_capacity(10, 2, 1, 3) == 1 + 5 * 3
    assert search.astar_capacity(10, 3, 16, 0) == 1
    per = search.pool_node_bytes(3)
    assert per == 54 + 24 + 18 + 32 and search.pool_node_bytes(2) == 24 + 16 + 18 + 32
    c = search.astar_capacity(1000, 3, 1024, 100)                            # capped by the byte budget
    assert c == search.POOL_BUDGET_BYTES // (per * 1000) and c * 1000 * per <= search.POOL_BUDGET_BYTES
    assert search.astar_capacity(5, 3, 1024, 10 ** 6, budget_bytes=1 << 60) == ((1 << 31) - 1) // 5
    assert search.astar_capacity(1 << 20, 3, 4, 4, budget_bytes=1) == 1


# ---------------------------------------------------------------------------------------------------------- restatement
RADIUS = 6


@pytest.fixture(scope="module")
def ball(oracle):
    """The 2x2x2 ball of RADIUS by the oracle's moves: ({sticker bytes: distance}, states [n, 24], dist [n])."""
    levels = G.oracle_bfs(oracle, 2, RADIUS)
    assert tuple(len(lv.states) for lv in levels) == G.SPHERES_222[:RADIUS + 1]
    states = np.concatenate([lv.states for lv in levels])
    dist = np.concatenate([np.full(len(lv.states), lv.depth) for lv in levels])
    return {s.tobytes(): int(d) for s, d in zip(states, dist)}, states, dist


def heuristic(table):
    return lambda st: np.array([-min(table.get(s.tobytes(), RADIUS + 1), RADIUS + 1) for s in st], np.float32)


def test_priority_arithmetic_and_order():
    assert R.prio_of(np.float32(1.0), 0.1, 3).dtype == np.float32
    s, w, g = np.array([1052320509, 1058753659], np.uint32).view(np.float32)[0], np.array([1058753659], np.uint32).view(np.float32)[0], 29
    assert R.prio_of(s, float(w), g) == np.float32(s - np.float32(w * np.float32(g)))                     # two roundings
    assert R.prio_of(s, float(w), g) != np.float32(np.float64(s) - np.float64(w) * np.float64(g))         # and not the fused result
    prio = np.array([1.0, np.nan, 1.0, -0.0, 0.0, np.inf, -np.inf], np.float32)
    nodes = np.arange(7)
    assert R.best_open(prio, nodes, 7).tolist() == list(range(7))
    assert [R.best_open(prio, nodes, k).tolist() for k in (1, 2, 3, 4, 5, 6)] == [[5], [2, 5], [0, 2, 5], [0, 2, 4, 5], [0, 2, 3, 4, 5],
                                                                                 [0, 2, 3, 4, 5, 6]]
    assert R.best_open(prio, nodes, 2, tie="lower").tolist() == [0, 5] and R.best_open(prio, nodes, 4, tie="lower").tolist() == [0, 2, 3, 5]


def test_exact_heuristic_walks_one_geodesic(ball):
    """B = 1, weight = 1, h = -min(dist, R + 1), every root within R - 2: length == dist, iterations == dist, the moves replay to
    solved.  With the tie rule flipped to "lower node index wins" some root needs more iterations: the rule is observable."""
    table, states, dist = ball
    cube = Cube(2)
    keep = dist <= RADIUS - 2
    roots, d = states[keep], dist[keep]
    res = R.astar_search(cube, roots, 1, RADIUS, heuristic(table), weight=1.0)
    assert (res["length"] == d).all() and (res["iterations"] == d).all() and res["solved"].all() and not res["overflow"].any()
    solved = R.replay(cube, roots, res["actions"])
    assert res["actions"].shape == (max(1, d.max()), len(roots))
    for p in range(len(roots)):
        assert solved[d[p], p] and not solved[:d[p], p].any()
        assert (res["actions"][d[p]:, p] == cube.A).all() and (res["actions"][:d[p], p] < cube.A).all()
    assert (res["nodes"] <= 1 + 5 * np.maximum(d, 0) + (d > 0)).all()        # one node popped per iteration: at most A children each
    far = np.flatnonzero(d == RADIUS - 2)[:80]
    flipped = R.astar_search(cube, roots[far], 1, 400, heuristic(table), weight=1.0, tie="lower")
    assert (flipped["length"] == d[far]).all()                               # still optimal (consistent heuristic) ...
    assert (flipped["iterations"] >= d[far]).all() and (flipped["iterations"] > d[far]).any()   # ... but it floods the ties


def test_wider_batches_capacity_and_exhaustion(ball):
    table, states, dist = ball
    cube = Cube(2)
    roots, d = states[dist == 4][:60], 4
    res = R.astar_search(cube, roots, 4, 12, heuristic(table), weight=0.5)
    assert res["solved"].all() and (res["length"] >= d).all() and ((res["length"] - d) % 2 == 0).all()
    solved = R.replay(cube, roots, res["actions"])
    assert all(solved[res["length"][p], p] and not solved[:res["length"][p], p].any() for p in range(len(roots)))
    # a full pool at init: everything is dropped, the next pop finds no open node
    tiny = R.astar_search(cube, roots[:3], 4, 5, heuristic(table), capacity=1)
    assert (tiny["length"] == -1).all() and tiny["overflow"].all() and (tiny["nodes"] == 1).all() and (tiny["iterations"] == 2).all()
    # capacity 5: the first merge overflows mid-list (6 children, 4 fit)
    small = R.astar_search(cube, roots[:3], 4, 9, heuristic(table), capacity=5)
    assert small["overflow"].all() and (small["nodes"] == 5).all() and (small["length"] == -1).all()
    st = small["state"]
    assert (st.state.reshape(3, 5) == R.CLOSED).all() and (st.active == 0).all() and (small["iterations"] == 3).all()
    # a solved root and a depth-1 root
    one = states[dist <= 1]
    r1 = R.astar_search(cube, one, 2, 3, heuristic(table))
    assert r1["length"].tolist() == [0] + [1] * 6 and r1["iterations"].tolist() == [0] + [1] * 6 and r1["nodes"].tolist() == [1] * 7
