"""The tp_* section of librubikhip.so and its restatement without a GPU: header <-> exports <-> TWOPHASE_SIGNATURES, the host-only
entry points, the four restated searches against the level counts of the rule, the goal sets, the indices along oracle walks, the
restated state machines on small spheres, the restated two_phase_solve against the chain, and the Python layer's argument errors."""
import functools
import os
from ctypes import byref, c_int

import numpy as np
import pytest

from rubiks_cube_solver_amd import _chain_lib, _cubie_lib, _edge_lib, _episode_lib, _ida_lib, _lib, _native, _twophase_lib as T
from tests import chain_ref, cubie_ref, ida_ref, twophase_ref as R
from tests.test_cubies_host import exported, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"tp_table_bytes": 1, "tp_generators": 4, "tp_max_steps": 0, "tp_build_begin": 4, "tp_build_level": 6, "tp_index": 6,
         "tp_phase1_init": 25, "tp_phase1_search": 27, "tp_phase2_init": 20, "tp_phase2_search": 22}


@functools.lru_cache(maxsize=None)
def tabs():
    return [R.bfs(w)[0] for w in range(4)]


@functools.lru_cache(maxsize=None)
def chain_tabs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "chain_tables.npz"))
    return [g["stage0"], g["stage1"], chain_ref.bfs(2)[0], g["stage3"]]


def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "tp_")
    assert protos == ARITY
    L = T.twophase_lib()                                                    # loads without a GPU
    assert L is _lib.lib()
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("tp_")} == set(protos) == set(T.TWOPHASE_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(T.TWOPHASE_SIGNATURES[fn])[0]) == n_params, fn
    assert not any(fn.startswith("rc") for fn in T.TWOPHASE_SIGNATURES)
    # the other sections of the library are what they were
    for prefix, table, header in (("rct_", _chain_lib.CHAIN_SIGNATURES, "rubikhip.h"), ("rce_", _edge_lib.EDGE_SIGNATURES, "rubikhip.h"),
                                  ("ida_", _ida_lib.IDA_SIGNATURES, "rubikhip.h"), ("rcc_", _cubie_lib.CUBIE_SIGNATURES, "rubikhip.h"),
                                  ("rcx_", _episode_lib.EPISODE_SIGNATURES, "rubikepisode.h"), ("rc_", _lib.SIGNATURES, "rubikhip.h")):
        assert {e for e in names if e.startswith(prefix)} == set(prototypes(header, prefix)) == set(table), prefix
    header = open(os.path.join(ROOT, "include", "rubikhip.h")).read()
    for name, bit in (("TP_SOLVED", 1), ("TP_FULL", 1), ("TP_EXHAUSTED", 2), ("TP_ILLEGAL", 4), ("TP_BAD_FRAME", 8), ("TP_OUTSIDE", 16)):
        assert f"#define {name} {bit}u" in header and getattr(T, name[3:]) == bit == getattr(R, name[3:])
    assert (T.MAX_DEPTH, T.MAX_TRAIL, T.NOOP, T.INF) == (R.MAX_DEPTH, R.MAX_TRAIL, R.NOOP, R.INF)


def test_host_only_entry_points_and_their_argument_errors():
    L = T.twophase_lib()
    assert [T.table_bytes(w) for w in range(4)] == list(R.SIZE) == [1082565, 1013760, 967680, 967680]
    assert L.tp_table_bytes(-1) == -1 and L.tp_table_bytes(4) == -1
    assert 1 <= T.max_steps() < 2 ** 31
    for phase in (1, 2):
        gens, cost = T.generators(phase)
        want = R.GENERATORS[phase]
        assert len(gens) == len(want) and list(cost) == list(R.COST[phase])
        assert [tuple(a for a in row if a != 0xFF) for row in gens.tolist()] == list(want)
        full, fcost, count = np.zeros((12, 2), np.uint8), np.full(12, 9, np.uint8), c_int(0)
        assert L.tp_generators(phase, full.ctypes.data, fcost.ctypes.data, byref(count)) == 0 and count.value == len(want)
        assert (full[len(want):] == 0xFF).all() and (fcost[len(want):] == 0).all()
        assert L.tp_generators(phase, None, None, None) == 0
    for phase in (0, 3, -1):
        assert L.tp_generators(phase, None, None, None) == -1 and L.rc_last_error().startswith(b"tp_generators: phase")
    for bad in (-1, 4, True, 1.0, "0"):
        with pytest.raises(ValueError, match="which"):
            T.table_bytes(bad)
    with pytest.raises(ValueError, match="phase"):
        T.generators(3)


@pytest.mark.parametrize("which", range(4))
def test_restated_search_reproduces_the_level_counts(which):
    dist, levels = R.bfs(which)
    assert levels == R.LEVELS[which] and (dist != R.NONE).all() and dist[R.GOAL[which]] == 0 and (dist == 0).sum() == 1


def test_g1_spheres_and_generators_keep_g1():
    levels = R.g1_spheres(8)
    assert tuple(len(lv) for lv in levels) == R.G1_SPHERES
    rows = np.array([ida_ref.to_bytes(x) for lv in levels[:6] for x in lv])
    assert R.in_g1(rows).all()
    for g in R.GENERATORS[2]:
        assert R.in_g1(R.move_rows(rows, g)).all()
    for a in (2, 3, 4, 5, 8, 9, 10, 11):                                     # a quarter turn of F, R, B, L leaves G1
        assert not R.in_g1(R.move_rows(rows[:1], (a,))).any()
    # h of phase 2 is admissible and exact at the goal alone
    h2 = np.maximum(tabs()[2][R.index_legal(2, rows)], tabs()[3][R.index_legal(3, rows)])
    d = np.array([k for k, lv in enumerate(levels[:6]) for _ in lv])
    assert (h2 <= d).all() and ((h2 == 0) == (d == 0)).all()


def test_phase1_goal_set_is_the_domain_of_chain_stage_2(oracle):
    """Tables 0 and 1 both read 0 <=> the cube is in G1 = the domain of the chain's stage 2, on walks that stay near it."""
    rng = np.random.default_rng(11)
    st = oracle.solved(3, 600)
    for step in range(12):
        acts = rng.choice([0, 1, 6, 7, 0, 1, 6, 7, 2, 4, 8, 10], 600).astype(np.uint8)      # mostly U, D: F, R, B, L leave and return
        st = oracle.step(3, st, acts)[0]
        rows = cubie_ref.cubies(3, st)[0]
        both = (tabs()[0][R.index_legal(0, rows)] == 0) & (tabs()[1][R.index_legal(1, rows)] == 0)
        assert (both == (chain_ref.index(2, st) >= 0)).all() and (both == R.in_g1(rows)).all()
    assert both.any() and not both.all()


def test_indices_follow_the_coordinates_along_oracle_walks(oracle):
    """Along 30-move oracle walks the index of the sticker state's cubie rows = the index of the rows moved by the restated rule; and
    along walks of phase-2 generators tables 2 and 3 keep their domain."""
    rng = np.random.default_rng(12)
    st, rows = oracle.solved(3, 64), np.tile(R.HOME_ROWS, (64, 1))
    for _ in range(30):
        acts = rng.integers(0, 12, 64).astype(np.uint8)
        st = oracle.step(3, st, acts)[0]
        rows = np.stack([R.move_rows(rows[i:i + 1], (int(a),))[0] for i, a in enumerate(acts)])
        assert (rows == cubie_ref.cubies(3, st)[0]).all()
        for w in range(4):
            got = R.index_rows(w, rows)
            assert (got == np.where(R.index_legal(w, rows) >= 0, R.index_legal(w, rows), 0xFFFFFFFF)).all()
            assert (got[got != 0xFFFFFFFF] < R.SIZE[w]).all()
            assert [R.scalar_index(w, ida_ref.from_bytes(r)) for r in rows[:8]] == R.index_legal(w, rows[:8]).tolist()
    st, rows = oracle.solved(3, 64), np.tile(R.HOME_ROWS, (64, 1))
    for _ in range(30):
        gi = rng.integers(0, 8, 64)
        for i, j in enumerate(gi):
            for a in R.GENERATORS[2][j]:
                st[i:i + 1] = oracle.step(3, st[i:i + 1], np.array([a], np.uint8))[0]
        rows = np.stack([R.move_rows(rows[i:i + 1], R.GENERATORS[2][j])[0] for i, j in enumerate(gi)])
        assert (rows == cubie_ref.cubies(3, st)[0]).all() and R.in_g1(rows).all()
        assert (R.index_rows(2, rows) < R.SIZE[2]).all() and (R.index_rows(3, rows) < R.SIZE[3]).all()
        for w in (2, 3):
            assert [R.scalar_index(w, ida_ref.from_bytes(r)) for r in rows[:8]] == R.index_legal(w, rows[:8]).tolist()
    bad = rows.copy()
    bad[0, 9], bad[1, 0] = bad[0, 8], 24
    assert (R.index_rows(0, bad)[:2] == 0xFFFFFFFF).all() and R.index_rows(0, bad)[2] != 0xFFFFFFFF


def test_restated_phase2_returns_the_weighted_distance():
    """On every G1 state within weighted distance 5 phase 2 returns exactly that distance and a path that solves."""
    h2 = R.Heuristic(2, tabs())
    levels = R.g1_spheres(5)
    assert sum(len(lv) for lv in levels) == 1 + 4 + 10 + 36 + 123 + 368
    for d, level in enumerate(levels):
        for x in level:
            f = R.Phase2(ida_ref.to_bytes(x), h2, limit=20).run()
            assert f.status == R.SOLVED and f.depth == d and len(f.solution) == d
            assert R.apply(x, f.solution) == ida_ref.HOME
    x = levels[5][7]
    f = R.Phase2(ida_ref.to_bytes(x), h2, limit=4).run()
    assert f.status == R.EXHAUSTED and f.next >= 5
    whole = R.Phase2(ida_ref.to_bytes(x), h2, limit=20).run()
    cut = R.Phase2(ida_ref.to_bytes(x), h2, limit=20)
    for k in range(1, whole.passes + 1):
        cut.run(max_passes=k)
    assert cut.fields() == whole.fields()
    # the canonical rule reads the prefix: after U no U' first, after F F no F2, after U U no third U
    far = ida_ref.to_bytes(levels[5][0])
    open_after = lambda prefix: R.Phase2(far, h2, limit=40, prefix=prefix).open()
    assert open_after(()) == list(range(8))
    assert open_after((0,)) == [0, 2, 3, 4, 5, 6, 7]                         # U U is a half turn; U' would undo
    assert open_after((2, 2)) == [0, 1, 3, 4, 5, 6, 7]                       # F F F
    assert open_after((0, 0)) == [2, 3, 4, 5, 6, 7]
    assert open_after((6,)) == [2, 3, 4, 6, 6 + 1][:0] + [2, 3, 4, 6, 7]     # after D: no U, U' (the lower face goes first), no D'


def test_restated_phase1_candidates():
    """Candidates of 50 walks of 6 moves: distinct, nondecreasing in length, each ends in G1, none ends in a U or D turn."""
    h1 = R.Heuristic(1, tabs())
    rng = np.random.default_rng(13)
    seen_any = 0
    for _ in range(50):
        x = R.apply(ida_ref.HOME, rng.integers(0, 12, 6).tolist())
        f = R.Phase1(ida_ref.to_bytes(x), h1, K=6, limit=7).run(cap=200000)
        assert f.status in (R.FULL, R.EXHAUSTED)
        paths = [c[0] for c in f.cands]
        assert len(set(paths)) == len(paths) and [len(p) for p in paths] == sorted(len(p) for p in paths)
        for path, rows in f.cands:
            assert R.in_g1(np.array([rows]))[0] and ida_ref.to_bytes(R.apply(x, path)) == rows
            assert not path or path[-1] >> 1 not in (0, 3)
        assert paths and len(paths[0]) == h1(x) or h1(x) == 0 or len(paths[0]) >= h1(x)
        seen_any += len(paths)
    assert seen_any >= 150
    g = R.Phase1(R.HOME_ROWS.tolist(), h1, K=2, limit=4)                      # a cube in G1: candidate 0 of length 0, searched all the same
    assert g.found == 1 and g.cands[0][0] == () and g.status == 0
    assert R.Phase1(R.HOME_ROWS.tolist(), h1, K=1, limit=4).status == R.FULL


def test_restated_two_phase_solve_beats_the_chain(oracle):
    """20 random cubes: every answer replays to solved on the oracle at its length, is no longer than the chain's and has its parity."""
    st, _ = chain_ref.scramble(20, 40, seed=14)
    rows = cubie_ref.cubies(3, st)[0]
    sources = []
    for c in range(20):
        out = R.solve(tabs(), chain_tabs(), rows[c].tolist(), K=3, phase1_limit=12, phase2_limit=14, max_steps=3000)
        acts = np.array(out["actions"], np.int64).reshape(-1, 1)
        assert len(acts) == out["length"] and (chain_ref.replay(st[c:c + 1], acts) == oracle.solved(3, 1)).all()
        assert out["length"] <= out["chain_length"] and (out["length"] - out["chain_length"]) % 2 == 0
        sources.append(out["source"])
    assert any(s != 0 for s in sources)


def test_python_argument_errors_come_before_any_device_use():
    import torch
    import rubiks_cube_solver_amd as rc
    from rubiks_cube_solver_amd import pattern, search
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    assert rc.two_phase_solve is search.two_phase_solve and "two_phase_solve" in rc.__all__ and hasattr(VecCubeEnv, "two_phase_solve")
    assert rc.TwoPhaseTables is pattern.TwoPhaseTables and "TwoPhaseTables" in rc.__all__

    class Env3:
        cube_size, stickers, num_envs = 3, torch.zeros((1, 54, 16), dtype=torch.uint8), 1

    class Env2:
        cube_size, stickers, num_envs = 2, torch.zeros(1), 1
    tp = pattern.TwoPhaseTables.__new__(pattern.TwoPhaseTables)              # no device needed to be refused
    ch = pattern.ChainTables.__new__(pattern.ChainTables)
    tp.device = ch.device = torch.device("cuda", 0)
    for bad in ("x", None, ch):
        with pytest.raises(ValueError, match="tables is a pattern.TwoPhaseTables"):
            search.two_phase_solve(bad, ch, Env3())
    for bad in ("x", None, tp):
        with pytest.raises(ValueError, match="chain is a pattern.ChainTables"):
            search.two_phase_solve(tp, bad, Env3())
    for env in (Env2(), "x"):
        with pytest.raises(ValueError, match="3x3x3 VecCubeEnv"):
            search.two_phase_solve(tp, ch, env)
    for kw in (dict(candidates=0), dict(candidates=4097), dict(candidates=2.0), dict(phase1_limit=33), dict(phase1_limit=-1),
               dict(phase2_limit=33), dict(phase2_limit=True), dict(max_steps=0), dict(steps_per_call=0),
               dict(steps_per_call=T.max_steps() + 1), dict(steps_per_call=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            search.two_phase_solve(tp, ch, Env3(), **kw)
    with pytest.raises(ValueError, match="the tables are on"):              # a host env against tables said to be elsewhere
        search.two_phase_solve(tp, ch, Env3())
    ch.device = torch.device("cpu")
    with pytest.raises(ValueError, match="the chain's on"):
        search.two_phase_solve(tp, ch, Env3())
    with pytest.raises(ValueError, match="3x3x3 only"):
        pattern.TwoPhaseTables.build("cuda", cube_size=2)
    with pytest.raises(ValueError, match="4 tables"):
        pattern.TwoPhaseTables([torch.zeros(4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="table 0 is a contiguous uint8 tensor"):
        pattern.TwoPhaseTables([torch.zeros(4, dtype=torch.uint8)] * 4)
    with pytest.raises(ValueError, match="HIP device"):
        pattern.TwoPhaseTables([torch.zeros(n, dtype=torch.uint8) for n in R.SIZE])


# ------------------------------------------------------------------------------------------------------------------ deep sets
def test_the_deep_phase2_cases_end_within_the_pass_cap_and_reach_the_upper_rows():
    """tests/deep_cases.py: every written phase-2 frame is taken, ends in a status its construction predicts within PASS_CAP restated
    passes (printed), and a SOLVED column's rows floor..depth-1 bring its root home; the set covers k0 = 15, 16, 17, k >= 24, f >= 16,
    f + cost(W) = 48 = max_depth, floor + 32 as the cap and max_depth below the limit; word 1 of the trail is nonzero in every case
    whose trail reaches nibble 16, and a half turn lies across rows 15/16 or 31/32 of a SOLVED path."""
    from tests import deep_cases as D
    h2 = R.Heuristic(2, tabs())
    cases = D.phase2_cases() + D.phase2_cases(24)
    assert {c.k0 for c in cases} >= {15, 16, 17} and any(c.k >= 24 for c in cases) and any(c.f >= 16 for c in cases)
    assert any(c.total == 48 == c.max_depth == c.lim for c in cases) and any(c.lim == c.f + 32 < min(c.total, c.limit, c.max_depth) for c in cases)
    assert any(c.lim == c.max_depth < min(c.total, c.limit, c.f + 32) for c in cases)
    written, straddles = set(), 0
    for c in cases:
        f = c.frame(h2)
        assert f.status == 0 and f.k == c.k0 and f.depth <= f.bound == min(c.total, c.lim), c.name
        f.run(max_passes=D.PASS_CAP + 1)
        print(f"deep phase 2 {c.name} ({c.why}): {f.passes} passes, {f.nodes} nodes, status {f.status}, depth {f.depth}, {f.k} generators")
        assert f.passes <= D.PASS_CAP and f.status in c.want, c.name
        if f.status == R.SOLVED:
            assert f.depth <= f.bound and c.f + len(f.solution) == f.depth, c.name
            assert R.apply(ida_ref.from_bytes(c.root), f.solution) == ida_ref.HOME, c.name
            col = list(c.prefix) + f.solution
            straddles += sum(1 for r in (15, 31) if r + 1 < len(col) and r >= c.f and col[r] == col[r + 1] and _one_half_turn(c.f, f, r))
        else:
            assert f.next > c.lim, c.name
        assert f.word1 == (max(f.written | {c.k0 - 1}) >= 16 and any(f.nib[16:])), c.name
        if max(f.written | {c.k0 - 1}) >= 16:
            assert f.word1, c.name
        written |= f.written
    assert max(written) >= 16 and {15, 16, 17} <= written and straddles >= 1


def _one_half_turn(floor, f, r):
    """rows r, r + 1 of a SOLVED column are the two actions of ONE generator"""
    row = floor
    for j in f.nib[:f.k]:
        if R.COST[2][j] == 2 and row == r:
            return True
        row += R.COST[2][j]
    return False


def test_the_deep_phase1_cases_end_within_the_pass_cap_and_emit_at_length_32():
    """Every written phase-1 frame is taken and ends FULL within PASS_CAP restated passes (printed); every candidate ends in G1, has
    the iteration's length and no U or D turn at its end; over the set an emission has length 32 (path row 31)."""
    from tests import deep_cases as D
    h1 = R.Heuristic(1, tabs())
    cases = D.phase1_cases()
    assert [(c.L, c.d0, c.K) for c in cases] == [(L, d0, K) for K in (1, 8) for L, d0 in ((18, 15), (20, 17), (32, 29), (32, 30))]
    longest = 0
    for c in cases:
        f = c.frame(h1)
        assert f.status == 0 and f.depth == c.d0 and f.bound == c.L == f.lim, c.name
        f.run(max_passes=D.PASS_CAP + 1)
        print(f"deep phase 1 {c.name}: {f.passes} passes, {f.nodes} nodes, status {f.status}, found {f.found}")
        assert f.passes <= D.PASS_CAP and f.status == R.FULL and f.found == c.K, c.name
        for path, rows in f.cands:
            assert len(path) == c.L and path[-1] >> 1 not in (0, 3) and R.in_g1(np.array([rows]))[0], c.name
            assert ida_ref.to_bytes(R.apply(ida_ref.from_bytes(c.root), path)) == rows, c.name
        assert f.cands[0][0] == tuple(c.W) or c.K > 1 or len(f.cands[0][0]) == c.L
        assert f.word1 and max(f.written) >= 16, c.name
        longest = max(longest, max(len(p) for p, _ in f.cands))
    assert longest == 32


def test_resume_refuses_what_the_header_refuses_and_continues_what_a_run_left():
    """Phase1.resume and Phase2.resume on frames the caller wrote: each invalid frame of the header's list gets TP_BAD_FRAME and keeps
    its fields; the frame an uninterrupted run leaves after p passes, written back, continues to the same end."""
    from tests import deep_cases as D
    h1, h2 = R.Heuristic(1, tabs()), R.Heuristic(2, tabs())
    c = D.Phase1Case(20, 17, 8)
    good = dict(c.written, next=R.INF, nodes=0)
    assert R.Phase1.resume(c.root, h1, 8, 20, **good).status == 0
    for kw in (dict(depth=-1), dict(depth=32, bound=32), dict(depth=21), dict(cursor=13), dict(bound=21), dict(found=-1), dict(found=8),
               dict(trail=c.W[:16] + [12]), dict(trail=[14] + c.W[1:17])):
        f = R.Phase1.resume(c.root, h1, 8, 32 if kw.get("bound") == 32 else 20, **{**good, **kw})
        assert f.status == R.BAD_FRAME, kw
        assert f.fields() == dict(trail=f.words, cursor=kw.get("cursor", 0), depth=kw.get("depth", 17), bound=kw.get("bound", 20), next=R.INF,
                                  nodes=0, status=R.BAD_FRAME) and f.found == kw.get("found", 0) and f.run().passes == 0, kw
    assert R.Phase1.resume(c.root, h1, 8, 20, max_depth=19, **good).status == R.BAD_FRAME      # the cap is min(limit, max_depth, 32)
    assert R.Phase1.resume(c.root, h1, 8, 40, **{**good, "bound": 33}).status == R.BAD_FRAME
    whole = c.frame(h1).run()
    for p in (1, 40, whole.passes // 2, whole.passes - 1):
        cut = c.frame(h1).run(max_passes=p)
        again = R.Phase1.resume(c.root, h1, 8, 20, **cut.written_frame()).run()
        assert again.status == R.FULL and again.passes == whole.passes - p and again.fields() == whole.fields() and again.cands == whole.cands, p
    c = D.Phase2Case(16, 18, 15, cost=28)
    good = dict(c.written, next=R.INF, nodes=0)
    make = lambda limit=48, prefix=tuple(c.prefix), max_depth=48, floor_given=None, **kw: R.Phase2.resume(
        c.root, h2, limit, prefix=prefix, max_depth=max_depth, floor_given=floor_given, **{**good, **kw})
    assert make().status == 0 and make().k == 15
    g, b = good["depth"], good["bound"]
    for kw in (dict(floor_given=-1), dict(floor_given=49), dict(prefix=tuple(c.prefix[:15]) + (12,)), dict(prefix=tuple(c.prefix[:14]) + (200, 0)),
               dict(depth=15), dict(depth=49, bound=49), dict(max_depth=g - 1), dict(depth=b + 1, trail=c.W[:16]), dict(cursor=9), dict(bound=49),
               dict(limit=b - 1), dict(max_depth=b - 1), dict(trail=c.W[:14] + [8]), dict(depth=g + 1, trail=c.W[:15] + [2])):   # F2: the costs step over g + 1
        f = make(**kw)
        assert f.status == R.BAD_FRAME, kw
        assert (f.depth, f.bound, f.cursor, f.next, f.nodes) == (kw.get("depth", g), kw.get("bound", b), kw.get("cursor", 0), R.INF, 0), kw
        assert f.words == [sum(v << (4 * i) for i, v in enumerate((kw.get("trail", c.W[:15]) + [0] * 32)[16 * w:16 * w + 16])) for w in range(2)], kw
    assert make(limit=60, max_depth=48, bound=48).status == 0 and R.Phase2.resume(c.root, h2, 60, max_depth=48, **{**good, "depth": g - 16, "bound": 33}).status == R.BAD_FRAME
    outside = R.Phase2.resume(ida_ref.to_bytes(R.apply(ida_ref.HOME, (2,))), h2, 48, **dict(good, depth=0, bound=10, trail=[]))
    assert outside.status == R.OUTSIDE
    c = D.phase2_cases()[-1]                                                 # the longest run of the set
    whole = c.frame(h2).run()
    assert whole.status == R.SOLVED and whole.passes > 1000
    for p in (1, 100, whole.passes // 2, whole.passes - 1):
        cut = c.frame(h2).run(max_passes=p)
        again = R.Phase2.resume(c.root, h2, 48, prefix=tuple(c.prefix), **cut.written_frame()).run()
        assert again.passes == whole.passes - p and again.fields() == whole.fields() and again.solution == whole.solution, p
