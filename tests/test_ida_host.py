"""The ida_* section of librubikhip.so and its restatement without a GPU: header <-> exports <-> IDA_SIGNATURES, the canonical-move
mask three ways, the counts of canonical sequences, what canonical sequences reach, the restated search without a table against
breadth-first distances, and the Python layer's argument errors."""
import os

import numpy as np
import pytest

from rubiks_cube_solver_amd import _ida_lib, _lib, _native, tables
from tests import cubie_ref, ida_ref as R, pattern_ref
from tests.test_cubies_host import exported, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"ida_max_steps": 0, "ida_canonical": 1, "ida_init": 22, "ida_search": 24}


def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "ida_")
    assert protos == ARITY
    L = _ida_lib.ida_lib()                                                  # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("ida_")} == set(protos) == set(_ida_lib.IDA_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_ida_lib.IDA_SIGNATURES[fn])[0]) == n_params, fn
    assert not any(fn.startswith("rc") for fn in _ida_lib.IDA_SIGNATURES)   # the closed lists of the rc* sections stay closed
    header = open(os.path.join(ROOT, "include", "rubikhip.h")).read()
    for name, bit in (("IDA_SOLVED", 1), ("IDA_EXHAUSTED", 2), ("IDA_ILLEGAL", 4), ("IDA_BAD_FRAME", 8)):
        assert f"#define {name} {bit}u" in header and getattr(_ida_lib, name[4:]) == bit == getattr(R, name[4:])
    assert 1 <= _ida_lib.max_steps() < 2 ** 31 and (_ida_lib.MAX_DEPTH, _ida_lib.NOOP, _ida_lib.INF) == (R.MAX_DEPTH, R.NOOP, R.INF)


def test_the_canonical_mask_three_ways():
    """ida_canonical (what the kernel was compiled with) = the restated rule; and the rule's one claim about the cube: faces f and
    f + 3 commute on the package's own permutations, no other pair of distinct faces does."""
    got = _ida_lib.canonical()
    assert got.shape == (13, 13, 12) and (got == R.allowed_mask()).all()
    assert got[12, 12].all() and got[:, 12].all()                           # after no move everything goes
    perm = tables.get_tables(3).perm.astype(np.int64)
    for a in range(12):
        assert (perm[a][perm[a ^ 1]] == np.arange(54)).all()                # a ^ 1 undoes a
        for b in range(12):
            commute = (perm[a][perm[b]] == perm[b][perm[a]]).all()
            assert commute == (a >> 1 == b >> 1 or abs((a >> 1) - (b >> 1)) == 3), (a, b)
    assert [len(p) for p in map(_ida_lib.prefixes, range(4))] == [1, 12, 114, 1068]
    assert [tuple(r) for r in _ida_lib.prefixes(2)] == list(R.sequences(2))


def test_the_counts_of_canonical_sequences():
    assert tuple(R.count(k) for k in range(1, 8)) == R.COUNTS
    assert tuple(sum(1 for _ in R.sequences(k)) for k in range(1, 5)) == R.COUNTS[:4]


def test_the_movers_are_the_oracles(oracle):
    """The 48-entry movers against the oracle on 64 walks of 30 moves, and corner_index against pattern_ref's."""
    rng = np.random.default_rng(5)
    st = oracle.solved(3, 64)
    xs = [R.HOME] * 64
    for _ in range(30):
        acts = rng.integers(0, 12, 64).astype(np.uint8)
        st = oracle.step(3, st, acts)[0]
        xs = [R.movers()[a](x) for a, x in zip(acts, xs)]
        cub = cubie_ref.cubies(3, st)[0]
        assert (np.array([R.to_bytes(x) for x in xs]) == cub).all()
    assert all(R.from_bytes(R.to_bytes(x)) == x for x in xs)
    c = cub[:, :8].astype(np.int64)
    assert (np.array([R.corner_index(x) for x in xs]) == pattern_ref.rank(c // 3, c % 3)).all()
    assert (np.array([R.corner_index(x) for x in xs]) == cubie_ref.cubies(3, st)[2]).all()
    for a in range(12):
        assert R.movers()[a ^ 1](R.movers()[a](xs[0])) == xs[0]


def test_canonical_sequences_reach_each_sphere_once():
    """Canonical sequences of length k, moved by the oracle's movers, reach exactly the states at distance k, each once, for k <= 5
    (the spheres of the quarter-turn metric: 12, 114, 1068, 10 011, 93 840)."""
    dist, levels = R.spheres(5)
    assert tuple(len(lv) for lv in levels[1:]) == R.COUNTS[:5]
    mv = R.movers()

    def walk(x, p2, p1, k, out):
        if k == 0:
            out.append(x)
            return
        for m in R.ALLOWED[p2][p1]:
            walk(mv[m](x), p1, m, k - 1, out)
    for k in range(1, 6):
        out = []
        walk(R.HOME, R.NOOP, R.NOOP, k, out)
        assert len(out) == R.COUNTS[k - 1] == len(set(out)) and all(dist[x] == k for x in out), k


def test_a_full_iteration_without_a_table_generates_every_canonical_child():
    """At bound b, h = 0, from a cube more than b + 1 moves from solved: c_1 + ... + c_{b+1} children, then next = b + 1."""
    far = R.to_bytes(next(iter(R.spheres(5)[1][5])))
    for b in range(4):
        f = R.Frame(far, R.Heuristic(), limit=b, max_depth=8)
        assert f.status == 0 and f.bound == 0
        f.run()
        assert f.status == R.EXHAUSTED and f.next == b + 1 and f.nodes == sum(sum(R.COUNTS[:i + 1]) for i in range(b + 1))
        # one iteration alone: from bound b's start to its exhaustion
        g = R.Frame(far, R.Heuristic(), limit=b, max_depth=8)
        g.bound = b
        g.run()
        assert g.nodes == sum(R.COUNTS[:b + 1]) and g.next == b + 1


def test_without_a_table_the_restatement_returns_the_distance():
    dist, levels = R.spheres(3)
    h = R.Heuristic()
    for d, level in enumerate(levels):
        for x in level:                                                      # all 1 + 12 + 114 + 1068
            f = R.solve(R.to_bytes(x), h, limit=5)
            assert f.status == R.SOLVED and f.length == d == dist[x] and f.lower_bound == d
            assert R.replay_bytes(R.to_bytes(x), f.path) == R.to_bytes(R.HOME)
            assert f.nodes >= sum(sum(R.COUNTS[:i + 1]) for i in range(d)) + (d > 0)
    # limits and frames
    x = R.to_bytes(levels[3][5])
    f = R.solve(x, h, limit=2)
    assert f.status == R.EXHAUSTED and f.next == 3 == f.lower_bound and f.length == -1
    assert R.Frame(x, h, 5, 8, prefix=(0, 12)).status == R.BAD_FRAME and R.Frame(x, h, 5, 8, floor_given=9).status == R.BAD_FRAME
    bad = list(x)
    bad[9] = bad[8]
    assert R.Frame(bad, h, 5, 8).status == R.ILLEGAL and R.Frame([24] + x[1:], h, 5, 8).status == R.ILLEGAL
    # a budget cut anywhere leaves the same frames
    whole = R.solve(x, h, limit=5)
    cut = R.Frame(x, h, 5, 5)
    for k in range(1, whole.passes + 1):
        cut.run(max_passes=k)
    assert (cut.trail, cut.nodes, cut.bound, cut.next, cut.status) == (whole.trail, whole.nodes, whole.bound, whole.next, whole.status)


def test_python_argument_errors_come_before_any_device_use():
    import torch
    import rubiks_cube_solver_amd as rc
    from rubiks_cube_solver_amd import pattern, search
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    assert rc.ida_search is search.ida_search and "ida_search" in rc.__all__ and hasattr(VecCubeEnv, "ida_search")

    class Env3:
        cube_size, stickers, num_envs = 3, torch.zeros((1, 54, 16), dtype=torch.uint8), 1

    class Env2:
        cube_size, stickers, num_envs = 2, torch.zeros(1), 1
    for table in ("x", 3, [None]):
        with pytest.raises(ValueError, match="table is a"):
            search.ida_search(table, Env3())
    for env in (Env2(), "x"):
        with pytest.raises(ValueError, match="3x3x3 VecCubeEnv"):
            search.ida_search(None, env)
    for kw in (dict(limit=33), dict(limit=-1), dict(limit=2.0), dict(split=4), dict(split=-1), dict(split=True), dict(max_steps=0),
               dict(steps_per_call=0), dict(steps_per_call=_ida_lib.max_steps() + 1), dict(steps_per_call=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            search.ida_search(None, Env3(), **kw)
    corner2 = pattern.CornerTable.__new__(pattern.CornerTable)              # no device needed to be refused
    corner2.cube_size, corner2.device = 2, torch.device("cpu")
    with pytest.raises(ValueError, match="3x3x3's"):
        search.ida_search(corner2, Env3())
    many = pattern.MaxTable.__new__(pattern.MaxTable)
    many.corner, many.device = None, torch.device("cpu")
    many.edge_tables = tuple(pattern.EdgeTable.__new__(pattern.EdgeTable) for _ in range(5))
    with pytest.raises(ValueError, match="at most 4"):
        search.ida_search(many, Env3())
    many.edge_tables = many.edge_tables[:1]
    with pytest.raises(ValueError, match="the tables are on"):            # a host env against a table said to be elsewhere
        many.device = torch.device("cuda", 0)
        search.ida_search(many, Env3())
    # the library refuses before any launch too: no device is initialised here, and RC_EINVAL needs none for these
    L = _ida_lib.ida_lib()
    assert L.ida_canonical(None) == -1 and L.rc_last_error().startswith(b"ida_canonical")


# ------------------------------------------------------------------------------------------------------------------ deep sets
def test_the_deep_cases_end_within_the_pass_cap_and_reach_word_1_of_the_trail():
    """tests/deep_cases.py, h = 0: every case ends in the status its construction predicts within PASS_CAP restated passes (printed);
    a SOLVED case's prefix and solution rows bring the root home; and the set covers what it is there for -- word 1 of the trail
    nonzero in every case that can reach nibble 16 (f + d > 16, d >= 1), a write at nibbles 15, 16 and 31, a node at g = 32."""
    from tests import deep_cases as D
    h, written, deepest = R.Heuristic(), set(), 0
    cases = D.ida_cases() + D.ida_cases(20)
    assert [(c.f, c.d) for c in cases] == [(13, 3), (14, 3), (15, 3), (16, 3), (17, 3), (28, 3), (29, 3), (30, 2), (31, 1), (32, 0), (29, 4),
                                          (30, 3), (17, 3)] and cases[-1].max_depth == 20 and cases[3].column[16:] == [R.NOOP] * 16
    for c in cases:
        f = c.frame(h)
        assert f.floor == f.depth == c.f and f.bound == c.f
        f.run(max_passes=D.PASS_CAP + 1, max_nodes=10 ** 9)
        print(f"deep IDA* {c.name}: {f.passes} passes, {f.nodes} nodes, status {f.status}, depth {f.depth}, next {f.next}")
        assert f.passes <= D.PASS_CAP and f.status == c.want, c.name
        if c.want == R.SOLVED:
            assert f.depth == c.f + c.d and f.nib[:c.f] == c.W[:c.f] and R.replay_bytes(c.root, f.path) == R.to_bytes(R.HOME), c.name
        else:
            assert f.depth == c.f and f.next == c.f + c.d == 33, c.name
        if c.d >= 1:
            assert f.word1 == (c.f + c.d > 16), c.name
            assert f.written == set(range(c.f, min(c.f + c.d, c.max_depth))), c.name
        written |= f.written
        deepest = max(deepest, f.deepest)
    assert {15, 16, 31} <= written and deepest == 32


def test_resume_refuses_what_the_header_refuses_and_continues_what_a_run_left():
    """Frame.resume on a frame the caller wrote: each invalid frame of the header's list gets IDA_BAD_FRAME and keeps every field;
    depth > bound is taken; the frame an uninterrupted run leaves after p passes, written back, continues to the same end."""
    from tests import deep_cases as D
    h = R.Heuristic()
    c = D.IdaCase(17, 3)
    whole = c.frame(h).run(max_nodes=10 ** 9)
    good = dict(floor=17, trail=c.W[:18], depth=18, bound=20, next=R.INF, cursor=3, nodes=5)
    assert R.Frame.resume(c.root, h, 32, 32, **good).status == 0
    bad = [dict(floor=-1), dict(floor=33), dict(depth=16), dict(depth=33, bound=32), dict(cursor=13), dict(bound=33), dict(trail=c.W[:17] + [12]),
           dict(trail=[15] + c.W[1:18])]
    for kw in bad:
        f = R.Frame.resume(c.root, h, 32, 32, **{**good, **kw})
        assert f.status == R.BAD_FRAME, kw
        w = {**good, **kw}
        assert (f.floor, f.nib, f.depth, f.bound, f.next, f.cursor, f.nodes) == \
               (w["floor"], (w["trail"] + [0] * 32)[:32], w["depth"], w["bound"], w["next"], w["cursor"], w["nodes"]), kw
        assert f.run().passes == 0                                           # a frame with a status is not touched
    assert R.Frame.resume(c.root, h, 20, 32, **{**good, "bound": 21}).status == R.BAD_FRAME       # the cap is min(limit, max_depth)
    assert R.Frame.resume(c.root, h, 32, 20, **{**good, "bound": 21}).status == R.BAD_FRAME
    assert R.Frame.resume(c.root, h, 32, 32, **{**good, "trail": c.W[:18] + [13]}).status == 0   # a stale nibble at or above depth
    assert R.Frame.resume([24] + c.root[1:], h, 32, 32, **good).status == R.ILLEGAL
    deep = R.Frame.resume(c.root, h, 32, 32, **{**good, "bound": 17})        # depth 18 > bound 17: taken; every child is dropped
    assert deep.status == 0
    while deep.depth == 18:
        deep.step()
    assert deep.depth == 17 and deep.next == 19 and deep.nodes - 5 == deep.passes - 1 > 0 and not deep.written
    for p in (0, 1, 5, 700, whole.passes - 1):
        cut = c.frame(h).run(max_passes=p, max_nodes=10 ** 9)
        again = R.Frame.resume(c.root, h, 32, 32, **cut.written_frame())
        assert again.status == 0 and again.x == cut.x
        again.run(max_nodes=10 ** 9)
        assert again.passes == whole.passes - p
        assert (again.status, again.trail, again.depth, again.bound, again.next, again.cursor, again.nodes, again.words) == \
               (whole.status, whole.trail, whole.depth, whole.bound, whole.next, whole.cursor, whole.nodes, whole.words), p
