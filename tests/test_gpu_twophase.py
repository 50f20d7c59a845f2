"""Two-phase on the GPU (pattern.TwoPhaseTables, search.two_phase_solve, the tp_* entry points of librubikhip.so): the built tables
against the restatement (tests/twophase_ref.py) at every index and level by level, tp_index in every layout with carved operands,
both search kernels frame for frame against the restated state machines and under every cut of the budget, two_phase_solve against
the oracle, the chain and the restated selection, every argument error, each launching export under capture and replay.  All
comparisons are exact.  GPU only."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from tests import chain_ref, ida_ref
from tests import layout_cases as LC
from tests import twophase_ref as R
from tests.test_gpu_cubies import FILL, Arena, rows_arena
from tests.test_gpu_search import env_of, scrambles

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as C  # noqa: E402
import stream_driver as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
COUNTS = (1, 3, 513, 1029)
LAYOUTS = ("tight", "padded", "t512")


def mods():
    from rubiks_cube_solver_amd import _lib, _twophase_lib, ops, pattern, search
    return _lib, _twophase_lib, ops, pattern, search


def stream():
    from rubiks_cube_solver_amd import _lib
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def ceil16(n):
    return -(-n // 16) * 16


@pytest.fixture(scope="module")
def tp():
    return mods()[3].TwoPhaseTables.build(DEV)


@pytest.fixture(scope="module")
def chain():
    return mods()[3].ChainTables.build(DEV)


@pytest.fixture(scope="module")
def ref():
    """The restated tables, once per module, and the two heuristics on them (their caches are shared by every test)."""
    tabs = [R.bfs(w)[0] for w in range(4)]
    return dict(tabs=tabs, h1=R.Heuristic(1, tabs), h2=R.Heuristic(2, tabs))


def rows_of(env):
    from rubiks_cube_solver_amd.tables import get_cubies
    states = mods()[2].to_aos(env.stickers, env.num_envs).cpu().numpy()
    return states, get_cubies(3).cubies(states)[0]


def g1_walks(n, moves, seed):
    """n G1 cubes, cube i after moves[i] random phase-2 generators: cubie rows [n, 20]."""
    rng = np.random.default_rng(seed)
    rows = np.tile(R.HOME_ROWS, (n, 1)).astype(np.int64)
    for i in range(n):
        for j in rng.integers(0, 8, moves[i]):
            rows[i:i + 1] = R.move_rows(rows[i:i + 1], R.GENERATORS[2][j])
    return rows.astype(np.uint8)


def cubie_buffer(rows):
    """[n, 20] -> a one-tile device buffer [20, pitch] and its pitch; pad columns hold FILL."""
    n = len(rows)
    buf = torch.full((20, ceil16(n)), FILL, dtype=torch.uint8, device=DEV)
    buf[:, :n] = torch.as_tensor(np.ascontiguousarray(np.asarray(rows, np.uint8).T)).to(DEV)
    return buf, buf.shape[1]


# ---------------------------------------------------------------------------------------------------------------- 1. tables
def test_tables_equal_the_restatement_at_every_index(tp, ref):
    _, _, _, pattern, _ = mods()
    assert tp.levels == R.LEVELS and tp.depth == tuple(len(lv) - 1 for lv in R.LEVELS)
    for w in range(4):
        t = tp.tables[w].cpu().numpy()
        assert t.dtype == np.uint8 and len(t) == R.SIZE[w] and (t == ref["tabs"][w]).all(), w
        assert tuple(np.bincount(t)) == R.LEVELS[w]
    wrapped = pattern.TwoPhaseTables([t.clone() for t in tp.tables])
    assert wrapped.levels is None and wrapped.depth is None
    with pytest.raises(ValueError):
        pattern.TwoPhaseTables([t[1:] for t in tp.tables])


@pytest.mark.parametrize("which", (1, 3))
def test_a_build_level_by_level(tp, ref, which):
    """One phase-1 and one phase-2 (weighted) table: the count per level, the table after each level = the restatement's entries up to
    it, so no entry changes once set; past the last level nothing is set."""
    _, T, _, _, _ = mods()
    L, n, want = T.twophase_lib(), R.SIZE[which], torch.as_tensor(ref["tabs"][which].copy()).to(DEV)
    table = torch.full((n + 32,), FILL, dtype=torch.uint8, device=DEV)
    count = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.tp_build_begin(p(table), n, which, stream()) == 0
    levels = R.LEVELS[which]
    for depth in range(len(levels) + 1):
        assert torch.equal(table[:n], torch.where(want <= depth, want, torch.full_like(want, 0xFF))), depth
        assert L.tp_build_level(p(table), n, which, depth, p(count), stream()) == 0
        assert int(count[0]) == (levels[depth + 1] if depth + 1 < len(levels) else 0), depth
    assert torch.equal(table[:n], want) and bool((table[n:] == FILL).all())


# ---------------------------------------------------------------------------------------------------------------- 2. tp_index
def outside_rows():
    """A flipped edge pair, a twisted pair, a slice edge out of its slice (all outside G1), then a byte >= 24, a piece twice, 0xFF."""
    out = np.tile(R.HOME_ROWS, (6, 1))
    out[0, [8, 9]] = 1, 3
    out[1, [0, 1]] = 1, 5
    out[2, [8, 16]] = 16, 0
    out[3, 12] = 24
    out[4, 9] = 0
    out[5, 3] = 0xFF
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_index_in_every_layout_carved(n):
    _, T, _, _, _ = mods()
    L = T.twophase_lib()
    _, scrambled = rows_of(env_of(3, scrambles(3, [100] * n, seed=20 + n)))
    inside = g1_walks(n, [100] * n, seed=30 + n) if n <= 3 else np.concatenate([g1_walks(40, [100] * 40, seed=30 + n)] * (n // 40 + 1))[:n]
    for which in range(4):
        rows = (scrambled if which < 2 else inside).copy()
        if n >= 6:
            rows[-6:] = outside_rows()
        want = R.index_rows(which, rows)
        assert (want[:max(1, n - 6)] != 0xFFFFFFFF).all()
        if n >= 6:
            assert (want[-3:] == 0xFFFFFFFF).all() and ((want[-6:-3] == 0xFFFFFFFF).all() == (which >= 2))
        for lay in LAYOUTS:
            offs = LC.carve_offsets(2)
            cub = rows_arena(rows, n, 20, lay, offs[0]).upload()
            out = Arena(4 * n, offs[1]).upload()
            assert L.tp_index(cub.ptr(), n, cub.pitch, which, out.ptr(), stream()) == 0, L.rc_last_error()
            out.expect(want)
            cub.check(f"table {which} n={n} {lay}: cubies")
            out.check(f"table {which} n={n} {lay}: index")


def test_index_and_distance_of_an_env(tp, ref):
    env = env_of(3, scrambles(3, [100] * 37, seed=3))
    _, rows = rows_of(env)
    for which in range(4):
        want = R.index_legal(which, rows)
        assert (tp.index(which, env).cpu().numpy() == want).all()
        d = np.where(want >= 0, ref["tabs"][which][np.maximum(want, 0)], 0xFF)
        assert (tp.distance(which, env).cpu().numpy() == d).all()


# ---------------------------------------------------------------------------------------------------------------- 3. phase 1
def phase1_frame(tp, rows, K, limit):
    S = mods()[4]
    cub, pitch = cubie_buffer(rows)
    fr = S.TwoPhase1Frame(tp, cub, len(rows), pitch, K, torch.as_tensor(np.asarray(limit, np.int32)).to(DEV))
    fr.init()
    return fr


def phase1_state(fr):
    """Every byte of the frame, host side."""
    return {k: getattr(fr, k).cpu().numpy().copy() for k in ("trail", "cursor", "depth", "bound", "next", "nodes", "found", "status", "path",
                                                              "cand_length", "cand_cubies")}


def same_frames(a, b, what):
    for k in a:
        assert (a[k] == b[k]).all(), (what, k)


def check_phase1(state, frames, K, stride, what):
    """The device frame against the restated frames, field by field; slots not emitted keep the caller's prefill."""
    n = len(frames)
    for c, f in enumerate(frames):
        got = dict(trail=[int(v) & (2 ** 64 - 1) for v in state["trail"][c]], cursor=int(state["cursor"][c]), depth=int(state["depth"][c]),
                   bound=int(state["bound"][c]), next=int(state["next"][c]), nodes=int(state["nodes"][c]), status=int(state["status"][c]))
        assert got == f.fields(), (what, c, got, f.fields())
        assert int(state["found"][c]) == f.found, (what, c)
        for j in range(K):
            col = j * stride + c
            path, rows = f.cands[j] if j < len(f.cands) else ((), R.HOME_ROWS.tolist())   # a refused frame's found may be any number
            assert state["path"][:, col].tolist() == list(path) + [R.NOOP] * (R.MAX_DEPTH - len(path)), (what, c, j)
            assert int(state["cand_length"][col]) == len(path) and state["cand_cubies"][:, col].tolist() == list(rows), (what, c, j)
    pad = np.ones(stride, bool)
    pad[:n] = False
    assert not state["status"][pad].any() and not state["found"][pad].any() and (state["path"].reshape(-1, K, stride)[:, :, pad] == R.NOOP).all(), what


def phase1_cubes():
    """Walks of 1..8 moves and 8 random cubes: cubie rows [16, 20]."""
    return rows_of(env_of(3, scrambles(3, list(range(1, 9)) + [100] * 8, seed=41)))[1]


@pytest.mark.parametrize("K", (1, 3, 8))
def test_phase1_frame_for_frame(tp, ref, K):
    """4096 passes cut four ways leave byte-equal frames, equal to the restatement's after 4096 passes; then on to 20 000."""
    rows, n, limit = phase1_cubes(), 16, 12
    frames = [R.Phase1(r.tolist(), ref["h1"], K, limit) for r in rows]
    fr = phase1_frame(tp, rows, K, [limit] * n)
    check_phase1(phase1_state(fr), frames, K, fr.stride, f"K={K} at init")
    first = None
    for cut in ([4096], [64] * 64, [7] * 585 + [1], [1] * 4096):
        fr = phase1_frame(tp, rows, K, [limit] * n)
        for k in cut:
            fr.search(k)
        state = phase1_state(fr)
        if first is None:
            first = state
            for f in frames:
                f.run(max_passes=4096)
            check_phase1(state, frames, K, fr.stride, f"K={K} after 4096 passes")
        else:
            same_frames(first, state, f"K={K} cut {cut[0]}")
    fr.search(15904)
    for f in frames:
        f.run(max_passes=20000)
    check_phase1(phase1_state(fr), frames, K, fr.stride, f"K={K} after 20 000 passes")
    running = int(fr.running[0])
    assert running == sum(1 for f in frames if not f.status)
    assert any(f.status == R.FULL for f in frames) and all(f.found >= 1 for f in frames[:8])
    before = phase1_state(fr)
    fr.search(64)                                                            # a cube with a status is not touched again
    after = phase1_state(fr)
    done = before["status"][:n] != 0
    for k in ("trail", "cursor", "depth", "bound", "next", "nodes", "found", "status"):
        assert (before[k][:n][done] == after[k][:n][done]).all(), k


def test_phase1_limits_g1_roots_and_illegal_rows(tp, ref):
    rows = phase1_cubes()
    rows = np.concatenate([rows[8:12], g1_walks(3, [0, 3, 9], seed=5), outside_rows()[3:]])
    n = len(rows)
    limit = [3, 0, -1, 32, 5, 5, 0, 5, 5, 5]
    for K in (1, 2):
        frames = [R.Phase1(r.tolist(), ref["h1"], K, lim) for r, lim in zip(rows, limit)]
        assert [f.status for f in frames[:3]] == [R.EXHAUSTED] * 3 and all(f.next == ref["h1"](ida_ref.from_bytes(r.tolist())) for f, r in zip(frames, rows[:3]))
        assert all(f.found == 1 and f.cands[0][0] == () for f in frames[4:7]) and [f.status for f in frames[7:]] == [R.ILLEGAL] * 3
        assert [f.status for f in frames[4:7]] == ([R.FULL] * 3 if K == 1 else [0, 0, 0])
        fr = phase1_frame(tp, rows, K, limit)
        check_phase1(phase1_state(fr), frames, K, fr.stride, f"K={K} init")
        fr.search(3000)
        for f in frames:
            f.run(max_passes=3000)
        check_phase1(phase1_state(fr), frames, K, fr.stride, f"K={K} after 3000 passes")


# ---------------------------------------------------------------------------------------------------------------- 4. phase 2
def phase2_frame(tp, rows, prefixes, limit, max_depth=R.MAX_DEPTH):
    S = mods()[4]
    n = len(rows)
    cub, pitch = cubie_buffer(rows)
    path = torch.full((max_depth, pitch), R.NOOP, dtype=torch.uint8, device=DEV)
    floor = torch.zeros(pitch, dtype=torch.int32, device=DEV)
    for c, pre in enumerate(prefixes):
        floor[c] = len(pre)
        if len(pre):
            path[:len(pre), c] = torch.as_tensor(list(pre), dtype=torch.uint8)
    lim = torch.full((pitch,), -1, dtype=torch.int32, device=DEV)
    lim[:n] = torch.as_tensor(np.asarray(limit, np.int32))
    fr = S.TwoPhase2Frame(tp, cub, n, pitch, path, floor, lim)
    fr.init()
    return fr


def phase2_state(fr):
    return {k: getattr(fr, k).cpu().numpy().copy() for k in ("trail", "cursor", "depth", "bound", "next", "nodes", "status", "path")}


def check_phase2(state, frames, prefixes, what):
    n = len(frames)
    for c, (f, pre) in enumerate(zip(frames, prefixes)):
        got = dict(trail=[int(v) & (2 ** 64 - 1) for v in state["trail"][c]], cursor=int(state["cursor"][c]), depth=int(state["depth"][c]),
                   bound=int(state["bound"][c]), next=int(state["next"][c]), nodes=int(state["nodes"][c]), status=int(state["status"][c]))
        assert got == f.fields(), (what, c, got, f.fields())
        col = list(pre) + (f.solution if f.status == R.SOLVED else [])
        assert state["path"][:, c].tolist() == col + [R.NOOP] * (state["path"].shape[0] - len(col)), (what, c)
    assert (state["path"][:, n:] == R.NOOP).all() and not state["status"][n:].any(), what


def test_phase2_frame_for_frame(tp, ref):
    """Roots 1..10 generators into G1, with and without a prefix, cut four ways; prefixes that end in U, in F F and in U U."""
    rows = g1_walks(20, list(range(1, 11)) * 2, seed=42)
    prefixes = [()] * 10 + [(0,), (2, 2), (0, 0), (3, 0), (6,), (4, 7), (1, 1), (8, 8), (5,), (2, 11, 6, 6)]
    n, limit = 20, [30] * 20
    make = lambda: [R.Phase2(r.tolist(), ref["h2"], lim, prefix=pre) for r, lim, pre in zip(rows, limit, prefixes)]
    frames = make()
    fr = phase2_frame(tp, rows, prefixes, limit)
    check_phase2(phase2_state(fr), frames, prefixes, "init")
    first = None
    for cut in ([4096], [64] * 64, [7] * 585 + [1], [1] * 4096):
        fr = phase2_frame(tp, rows, prefixes, limit)
        for k in cut:
            fr.search(k)
        state = phase2_state(fr)
        if first is None:
            first = state
            for f in frames:
                f.run(max_passes=4096)
            check_phase2(state, frames, prefixes, "after 4096 passes")
        else:
            same_frames(first, state, f"cut {cut[0]}")
    fr.search(15904)
    for f in frames:
        f.run(max_passes=20000)
    check_phase2(phase2_state(fr), frames, prefixes, "after 20 000 passes")
    assert sum(f.status == R.SOLVED for f in frames) >= 12
    for f, r, pre in zip(frames, rows, prefixes):
        if f.status == R.SOLVED:
            assert ida_ref.to_bytes(R.apply(ida_ref.from_bytes(r.tolist()), f.solution)) == R.HOME_ROWS.tolist() and f.depth == len(pre) + len(f.solution)
    # the canonical rule at the root reads the prefix
    roots = make()
    assert roots[10].open() == [0, 2, 3, 4, 5, 6, 7] and roots[11].open() == [0, 1, 3, 4, 5, 6, 7] and roots[12].open() == [2, 3, 4, 5, 6, 7]


def test_phase2_outside_limits_and_bad_frames(tp, ref):
    rows = np.concatenate([g1_walks(4, [6, 6, 0, 0], seed=43), phase1_cubes()[10:11], outside_rows()[:3], outside_rows()[3:], g1_walks(3, [5, 5, 5], seed=44)])
    prefixes = [(), (4, 4), (), (9,)] + [()] * 7 + [(12,), (0, 13), (3, 2)]
    n = len(rows)
    h = [ref["h2"](ida_ref.from_bytes(r.tolist())) for r in rows[:4]]
    limit = [h[0] - 1, 2 + h[1] - 1, -1, 1] + [30] * 10
    frames = [R.Phase2(r.tolist(), ref["h2"], lim, prefix=pre) for r, lim, pre in zip(rows, limit, prefixes)]
    assert [f.status for f in frames] == [R.EXHAUSTED] * 3 + [R.SOLVED] + [R.OUTSIDE] * 4 + [R.ILLEGAL] * 3 + [R.BAD_FRAME] * 2 + [0]
    assert frames[0].next == h[0] and frames[1].next == 2 + h[1] and frames[3].depth == 1
    fr = phase2_frame(tp, rows, prefixes, limit)
    check_phase2(phase2_state(fr), frames, prefixes, "init")                 # nothing is written to a path at init
    fr.search(5000)
    frames[-1].run(max_passes=5000)
    check_phase2(phase2_state(fr), frames, prefixes, "after the search")
    assert frames[-1].status == R.SOLVED and int(fr.running[0]) == 0
    fl = fr.floor.clone()
    fr.floor[13] = 49                                                        # a floor above max_depth
    fr.init()
    assert int(fr.status[13]) == R.BAD_FRAME
    fr.floor.copy_(fl)
    short = phase2_frame(tp, rows[13:14], [(3, 2)], [30], max_depth=6)       # min(limit, max_depth): the answer needs 2 + 5 rows
    short.search(5000)
    assert int(short.status[0]) == R.EXHAUSTED and (short.path[2:, 0] == R.NOOP).all()


def test_phase2_solves_every_g1_state_within_6_at_its_distance(tp):
    levels = R.g1_spheres(6)
    rows = np.array([ida_ref.to_bytes(x) for lv in levels for x in lv], np.uint8)
    d = np.array([k for k, lv in enumerate(levels) for _ in lv])
    n = len(rows)
    assert n == 1734
    fr = phase2_frame(tp, rows, [()] * n, [20] * n)
    fr.run(1 << 16, 1 << 12)
    assert int(fr.running[0]) == 0 and bool((fr.status[:n] == R.SOLVED).all())
    assert (fr.depth[:n].cpu().numpy() == d).all()
    path = fr.path[:, :n].cpu().numpy()
    assert ((path != R.NOOP).sum(0) == d).all()
    home = np.tile(R.HOME_ROWS, (n, 1))
    for c in range(0, n, 7):
        assert (R.move_rows(rows[c:c + 1], path[:d[c], c].tolist())[0] == home[0]).all(), c


# ------------------------------------------------------------------------------------------- 4b. deep sets: written frames
from tests import deep_cases as DC  # noqa: E402

FIELDS = ("cursor", "depth", "bound", "next", "nodes", "status")


def write_frames(fr, frames, phase):
    """The restated frames' fields into the device frame, as a caller writes them (phase 1: found and the candidates too)."""
    n = len(frames)
    fr.trail[:n] = torch.as_tensor(np.array([f.words for f in frames], np.uint64).view(np.int64)).to(DEV)
    for k in FIELDS:
        t = getattr(fr, k)
        t[:n] = torch.as_tensor(np.array([getattr(f, k) for f in frames], np.int64)).to(DEV).to(t.dtype)
    if phase == 1:
        fr.found[:n] = torch.as_tensor(np.array([f.found for f in frames], np.int64)).to(DEV).to(torch.int32)
        for c, f in enumerate(frames):
            for j, (path, rows) in enumerate(f.cands):
                col = j * fr.stride + c
                fr.path[:len(path), col] = torch.as_tensor(list(path), dtype=torch.uint8)
                fr.cand_length[col] = len(path)
                fr.cand_cubies[:, col] = torch.as_tensor(list(rows), dtype=torch.uint8)


def deep2(tp, ref, max_depth):
    """(cases, a fresh device frame with the written frames in it, the restated frames)"""
    cases = DC.phase2_cases(max_depth)
    fr = phase2_frame(tp, np.array([c.root for c in cases], np.uint8), [c.prefix for c in cases], [c.limit for c in cases], max_depth)
    frames = [c.frame(ref["h2"]) for c in cases]
    assert all(f.status == 0 for f in frames)
    write_frames(fr, frames, 2)
    return cases, fr, frames


@pytest.mark.parametrize("max_depth", (48, 24))
def test_deep_phase2_written_frames(tp, ref, max_depth):
    """The written frames of tests/deep_cases.py (trails of 15..21 generators, floors to 20, answers to row 47): after 64 passes and
    at the end every field, both trail words, every row of path and the running counter are the restatement's; launches of 1 and 7
    leave the same bytes as one launch; a frame stored after p passes and copied into a fresh frame over a fresh path continues to
    the same end."""
    cases, fr, frames = deep2(tp, ref, max_depth)
    prefixes = [c.prefix for c in cases]
    fr.search(64)
    for f in frames:
        f.run(max_passes=64)
    check_phase2(phase2_state(fr), frames, prefixes, "after 64 passes")
    assert int(fr.running[0]) == sum(1 for f in frames if not f.status)
    stored = {k: getattr(fr, k).clone() for k in ("trail",) + FIELDS}
    fr.search(DC.PASS_CAP)
    for c, f in zip(cases, frames):
        f.run(max_passes=DC.PASS_CAP + 64)
        assert f.status in c.want and f.passes <= DC.PASS_CAP, c.name
    whole = phase2_state(fr)
    check_phase2(whole, frames, prefixes, "at the end")
    assert int(fr.running[0]) == 0 and (max_depth != 48 or any(f.status == R.SOLVED and f.depth == 48 for f in frames))
    total = max(f.passes for f in frames)
    for per_call in (1, 7):
        _, cut, _ = deep2(tp, ref, max_depth)
        for spent in range(0, total, per_call):
            cut.search(min(per_call, total - spent))
        same_frames(whole, phase2_state(cut), f"launches of {per_call}")
    _, again, _ = deep2(tp, ref, max_depth)                                  # a fresh path: the prefixes alone
    for k, v in stored.items():
        getattr(again, k).copy_(v)
    again.search(DC.PASS_CAP)
    want = {k: v.copy() for k, v in whole.items()}
    early = np.flatnonzero(stored["status"].cpu().numpy()[:len(cases)])      # ended before the copy: not touched, so no rows are written
    for c in early:
        want["path"][len(prefixes[c]):, c] = R.NOOP
    same_frames(want, phase2_state(again), "resumed after 64 passes")
    assert len(early) < len(cases)


def deep1(tp, ref, K):
    cases = [c for c in DC.phase1_cases() if c.K == K]
    fr = phase1_frame(tp, np.array([c.root for c in cases], np.uint8), K, [c.limit for c in cases])
    frames = [c.frame(ref["h1"]) for c in cases]
    assert all(f.status == 0 for f in frames)
    write_frames(fr, frames, 1)
    return cases, fr, frames


@pytest.mark.parametrize("K", (1, 8))
def test_deep_phase1_written_frames(tp, ref, K):
    """The written phase-1 frames (trails of 15..30 actions, bound to 32): after 64 passes and at the end every field, every candidate
    column row by row (a candidate of length 32 fills rows 0..31), cand_length, cand_cubies and the running counter are the
    restatement's; launches of 1 and 7 leave the same bytes; a frame stored after 64 passes, copied with the candidates emitted so
    far, continues to the same end."""
    cases, fr, frames = deep1(tp, ref, K)
    fr.search(64)
    for f in frames:
        f.run(max_passes=64)
    check_phase1(phase1_state(fr), frames, K, fr.stride, "after 64 passes")
    assert int(fr.running[0]) == sum(1 for f in frames if not f.status)
    stored = phase1_state(fr)
    fr.search(DC.PASS_CAP)
    for c, f in zip(cases, frames):
        f.run(max_passes=DC.PASS_CAP + 64)
        assert f.status == R.FULL and f.passes <= DC.PASS_CAP, c.name
    whole = phase1_state(fr)
    check_phase1(whole, frames, K, fr.stride, "at the end")
    assert int(fr.running[0]) == 0 and any(len(p) == 32 for f in frames for p, _ in f.cands)
    total = max(f.passes for f in frames)
    for per_call in (7, 1) if K == 1 else (7,):
        _, cut, _ = deep1(tp, ref, K)
        for spent in range(0, total, per_call):
            cut.search(min(per_call, total - spent))
        same_frames(whole, phase1_state(cut), f"launches of {per_call}")
    _, again, _ = deep1(tp, ref, K)
    for k, v in stored.items():
        getattr(again, k).copy_(torch.as_tensor(v).to(DEV))
    again.search(DC.PASS_CAP)
    same_frames(whole, phase1_state(again), "resumed after 64 passes")


def test_phase1_launches_of_one_pass_on_the_deep_set(tp, ref):
    """K = 8 in launches of ONE pass, 8192 of them: byte-equal to one launch of 8192 (the set's longer runs are cut at 7 above)."""
    _, one, _ = deep1(tp, ref, 8)
    _, cut, _ = deep1(tp, ref, 8)
    one.search(8192)
    for _ in range(8192):
        cut.search(1)
    same_frames(phase1_state(one), phase1_state(cut), "launches of 1")
    assert int(one.running[0]) >= 1 and (one.status[:4] != 0).any()


def test_written_frames_that_are_invalid_get_bad_frame_and_keep_every_byte(tp, ref):
    """tp_phase1_search and tp_phase2_search on frames the caller wrote, one column per invalid frame of the header's list (odd
    columns) beside valid neighbours: the invalid column gets TP_BAD_FRAME and keeps every other byte of its frame, of its path
    column and (phase 1) of its candidate slots; running does not count it; a second call leaves it alone; the neighbours finish as
    the restatement says."""
    c = DC.Phase1Case(20, 17, 8)
    good = dict(c.written, next=R.INF, nodes=0)
    bad = [dict(depth=-1), dict(depth=32, bound=32, limit=32), dict(depth=21), dict(cursor=13), dict(bound=21), dict(found=-1), dict(found=8),
           dict(trail=c.W[:16] + [12]), dict(trail=[14] + c.W[1:17])]
    kws = [{**good, **(bad[i // 2] if i % 2 else {})} for i in range(2 * len(bad) + 1)]
    limit = [kw.pop("limit", 20) for kw in kws]
    n = len(kws)
    frames = [R.Phase1.resume(c.root, ref["h1"], 8, lim, **kw) for kw, lim in zip(kws, limit)]
    assert [f.status for f in frames] == [R.BAD_FRAME if i % 2 else 0 for i in range(n)]
    fr = phase1_frame(tp, np.array([c.root] * n, np.uint8), 8, limit)
    write_frames(fr, frames, 1)
    fr.status[:n] = 0
    for f in frames:
        f.run(max_passes=DC.PASS_CAP)
    assert all(f.status == R.FULL for f in frames[::2])
    fr.search(DC.PASS_CAP)
    state = phase1_state(fr)
    check_phase1(state, frames, 8, fr.stride, "phase 1 written frames")
    assert int(fr.running[0]) == 0
    fr.search(64)
    same_frames(state, phase1_state(fr), "phase 1, a second call")

    c = DC.Phase2Case(16, 18, 15, cost=28)
    good = dict(c.written, next=R.INF, nodes=0)
    g, b, pre = good["depth"], good["bound"], tuple(c.prefix)
    bad = [dict(floor_given=-1, prefix=()), dict(floor_given=49, prefix=()), dict(prefix=pre[:15] + (12,)), dict(prefix=pre[:14] + (200, 0)), dict(depth=15),
           dict(depth=49, bound=49), dict(depth=b + 1, trail=c.W[:16]), dict(cursor=9), dict(bound=49), dict(limit=b - 1), dict(trail=c.W[:14] + [8]),
           dict(depth=g + 1, trail=c.W[:15] + [2])]
    kws = [{**good, **(bad[i // 2] if i % 2 else {})} for i in range(2 * len(bad) + 1)]
    n = len(kws)
    limit, prefixes, floors = [kw.pop("limit", 48) for kw in kws], [kw.pop("prefix", pre) for kw in kws], [kw.pop("floor_given", None) for kw in kws]
    frames = [R.Phase2.resume(c.root, ref["h2"], lim, prefix=p_, floor_given=fl, **kw) for kw, lim, p_, fl in zip(kws, limit, prefixes, floors)]
    assert [f.status for f in frames] == [R.BAD_FRAME if i % 2 else 0 for i in range(n)]
    fr = phase2_frame(tp, np.array([c.root] * n, np.uint8), prefixes, limit)
    for i, fl in enumerate(floors):
        if fl is not None:
            fr.floor[i] = fl
    write_frames(fr, frames, 2)
    fr.status[:n] = 0
    for f in frames:
        f.run(max_passes=DC.PASS_CAP)
    assert all(f.status == R.SOLVED and f.depth == b for f in frames[::2])
    fr.search(DC.PASS_CAP)
    state = phase2_state(fr)
    check_phase2(state, frames, prefixes, "phase 2 written frames")
    assert int(fr.running[0]) == 0
    fr.search(64)
    same_frames(state, phase2_state(fr), "phase 2, a second call")


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def check_result(states, res, n, legal=None):
    from rubiks_cube_solver_amd.tables import get_tables
    legal = np.ones(n, bool) if legal is None else legal
    length, actions = res["length"].cpu().numpy(), res["actions"].cpu().numpy()
    chain_length = res["chain_length"].cpu().numpy()
    assert (res["solved"].cpu().numpy() == legal).all() and (length[legal] >= 0).all() and (length[~legal] == -1).all()
    assert actions.shape == (max(1, int(length.max())), n) and actions.dtype == np.uint8
    r = np.arange(actions.shape[0])[:, None]
    assert (actions[r >= length[None, :]] == R.NOOP).all() and (actions[r < length[None, :]] < 12).all()
    assert (chain_ref.replay(states, actions)[legal] == get_tables(3).solved).all()
    assert (length[legal] <= chain_length[legal]).all() and ((chain_length - length)[legal] % 2 == 0).all()
    return length, actions


@pytest.mark.parametrize("n", COUNTS)
def test_two_phase_solve_end_to_end(tp, chain, n):
    _, T, _, _, S = mods()
    env = env_of(3, scrambles(3, [100] * n, seed=50 + n))
    states, _ = rows_of(env)
    before = env.stickers.clone()
    K = 4
    res, fr = S.two_phase_frames(tp, chain, env, candidates=K, phase1_limit=12, phase2_limit=16, max_steps=30000, steps_per_call=8192)
    assert torch.equal(env.stickers, before)
    length, actions = check_result(states, res, n)
    one, two = fr["one"], fr["two"]
    view = lambda t: t.view(K, one.stride)[:, :n].cpu().numpy()
    found = one.found[:n].cpu().numpy()
    cl = res["chain_length"].cpu().numpy()
    cand, total, source = R.select(K, cl, view(one.cand_length), found, fr["descent"].cpu().numpy(), view(two.status), view(two.depth))
    assert (res["candidate"].cpu().numpy() == cand).all() and (length == total).all() and (res["source"].cpu().numpy() == source).all()
    lim = fr["limit2"].cpu().numpy()
    sure = np.where(np.arange(K)[:, None] < found[None, :], view(one.cand_length) + fr["descent"].cpu().numpy(), R.INF)
    G = np.minimum(sure.min(0), cl)
    assert (lim == np.where(np.arange(K)[:, None] < found[None, :], np.minimum(np.minimum(view(one.cand_length) + 16, G - 1), 48), -1)).all()
    assert (res["nodes"].cpu().numpy() == np.stack([one.nodes[:n].cpu().numpy(), view(two.nodes).sum(0)])).all()
    p1 = res["phase1_length"].cpu().numpy()
    assert (p1[source == 0] == -1).all() and (p1[source != 0] == view(one.cand_length)[cand[source != 0], np.flatnonzero(source != 0)]).all()
    print(f"two_phase_solve of {n} cubes, K={K}, 30 000 passes: mean {length.mean():.1f} (chain {cl.mean():.1f}), sources {np.bincount(source, minlength=3).tolist()}")
    if n >= 513:
        assert (source != 0).any() and length.mean() < cl.mean()
    same = env.two_phase_solve(tp, chain, candidates=K, phase1_limit=12, phase2_limit=16, max_steps=30000, steps_per_call=8192)
    for k in res:
        assert torch.equal(same[k], res[k]), k
    # with one pass nothing is found: chain_solve's bytes
    one_pass = S.two_phase_solve(tp, chain, env, candidates=K, max_steps=1)
    ch = S.chain_solve(chain, env)
    assert torch.equal(one_pass["actions"], ch["actions"]) and torch.equal(one_pass["length"], ch["length"]) and not bool(one_pass["source"].any())
    assert bool((one_pass["candidate"] == K).all()) and bool((one_pass["phase1_length"] == -1).all())


def test_illegal_cubes_are_not_searched(tp, chain):
    _, T, _, _, S = mods()
    from rubiks_cube_solver_amd import VecCubeEnv
    from rubiks_cube_solver_amd.tables import get_cubies
    cb, n = get_cubies(3), 24
    states, rows = rows_of(env_of(3, scrambles(3, [100] * n, seed=60)))
    rows = rows.copy()
    rows[3, 0] = rows[3, 0] // 3 * 3 + (rows[3, 0] + 1) % 3
    rows[7, 8] ^= 1
    rows[11, [8, 9]] = rows[11, [9, 8]]
    states[[3, 7, 11]] = cb.from_cubies(rows[[3, 7, 11]])[0]
    env = VecCubeEnv(n, DEV, 3, obs=None)
    env.set_sim_cube(states, check=False)
    bad = np.zeros(n, bool)
    bad[[3, 7, 11]] = True
    res = S.two_phase_solve(tp, chain, env, candidates=3, phase1_limit=12, max_steps=20000)
    check_result(states, res, n, ~bad)
    assert (res["status"].cpu().numpy()[bad] == R.ILLEGAL).all() and (res["candidate"].cpu().numpy()[bad] == -1).all()
    assert (res["actions"].cpu().numpy()[:, bad] == R.NOOP).all() and not res["nodes"].cpu().numpy()[:, bad].any()


def test_the_127_cubes_within_two_moves_get_their_optimal_length(tp, chain):
    _, _, ops, _, S = mods()
    seqs = [()] + [(a,) for a in range(12)] + list(itertools.product(range(12), repeat=2))
    scr = np.full((len(seqs), 2), 12, np.uint8)
    for i, q in enumerate(seqs):
        scr[i, :len(q)] = q
    env = env_of(3, scr)
    states, _ = rows_of(env)
    dist = {x: d for d, lv in enumerate(ida_ref.spheres(2)[1]) for x in lv}
    want = np.array([dist[R.apply(ida_ref.HOME, q)] for q in seqs])
    assert len(dist) == 127
    res = S.two_phase_solve(tp, chain, env, candidates=4, phase1_limit=6, max_steps=4000)
    length, _ = check_result(states, res, len(seqs))
    assert (length == want).all()


def test_the_222_and_wrong_tables_raise(tp, chain):
    _, _, _, pattern, S = mods()
    env2, env3 = env_of(2, scrambles(2, [3, 3], seed=1)), env_of(3, scrambles(3, [3], seed=1))
    for call in (lambda: S.two_phase_solve(tp, chain, env2), lambda: env2.two_phase_solve(tp, chain), lambda: tp.index(0, env2),
                 lambda: tp.distance(1, env2), lambda: S.two_phase_solve(chain, tp, env3), lambda: tp.index(4, env3),
                 lambda: pattern.TwoPhaseTables(tp.tables, cube_size=2)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------------- 6. argument errors
def test_argument_errors_write_nothing(tp):
    _, T, _, _, _ = mods()
    L, n, sp = T.twophase_lib(), 513, stream()
    K, stride = 2, 528
    cols = K * stride
    tabs = [t.clone() for t in tp.tables]
    N = [t.numel() for t in tabs]
    rows = rows_arena(np.tile(R.HOME_ROWS, (n, 1)), n, 20, "tight", 0).upload()
    out = Arena(4 * n + 16, 0).upload()
    bufs = dict(limit=Arena(4 * stride, 0), path=Arena(48 * cols, 0), cand_length=Arena(4 * cols, 0), cand=Arena(20 * cols, 0), trail=Arena(16 * cols, 0),
                cursor=Arena(cols, 0), depth=Arena(4 * cols, 0), bound=Arena(4 * cols, 0), next=Arena(4 * cols, 0), nodes=Arena(8 * cols, 0),
                found=Arena(4 * stride, 0), status=Arena(cols, 0), floor=Arena(4 * cols, 0), running=Arena(16, 0))
    for a in bufs.values():
        a.upload()
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    refused = []
    for w in (-1, 4, 255):
        refused += [L.tp_build_begin(p(tabs[0]), 1 << 22, w, sp), L.tp_build_level(p(tabs[0]), 1 << 22, w, 0, p(cnt), sp),
                    L.tp_index(rows.ptr(), n, rows.pitch, w, out.ptr(), sp)]
        assert b"which" in L.rc_last_error()
    refused += [L.tp_build_begin(None, N[0], 0, sp), L.tp_build_begin(p(tabs[0], 8), N[0], 0, sp), L.tp_build_begin(p(tabs[1]), N[0] - 1, 0, sp),
                L.tp_build_begin(p(tabs[0]), -1, 0, sp), L.tp_build_level(p(tabs[2]), N[2] - 1, 2, 0, p(cnt), sp),
                L.tp_build_level(p(tabs[2]), N[2], 2, -1, p(cnt), sp), L.tp_build_level(p(tabs[2]), N[2], 2, 254, p(cnt), sp),
                L.tp_build_level(p(tabs[2]), N[2], 2, 0, None, sp), L.tp_build_level(p(tabs[2]), N[2], 2, 0, p(cnt, 4), sp),
                L.tp_build_level(None, N[2], 2, 0, p(cnt), sp)]
    assert all(rc == EINVAL for rc in refused), refused
    good = dict(cubies=rows.ptr(), n=n, pitch=rows.pitch, which=0, index=out.ptr())
    call = lambda **kw: (lambda a: L.tp_index(a["cubies"], a["n"], a["pitch"], a["which"], a["index"], sp))({**good, **kw})
    for word, kw in [("cubies", dict(cubies=None)), ("cubies", dict(cubies=p(rows.view, 8))), ("n is", dict(n=-1)), ("pitch", dict(pitch=rows.pitch - 8)),
                     ("pitch", dict(pitch=256)), ("index", dict(index=None)), ("index", dict(index=p(out.view, 4))), ("which", dict(which=4))]:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in L.rc_last_error().decode(), (word, L.rc_last_error())
    P = {k: a.ptr() for k, a in bufs.items()}
    good1 = dict(cubies=rows.ptr(), n=n, pitch=rows.pitch, ta=p(tabs[0]), ba=N[0], tb=p(tabs[1]), bb=N[1], limit=P["limit"], K=K, stride=stride,
                 path=P["path"], md=48, pp=cols, cand_length=P["cand_length"], cand=P["cand"], cp=cols, trail=P["trail"], cursor=P["cursor"],
                 depth=P["depth"], bound=P["bound"], next=P["next"], nodes=P["nodes"], found=P["found"], status=P["status"], steps=64,
                 running=P["running"])
    order1 = ("cubies", "n", "pitch", "ta", "ba", "tb", "bb", "limit", "K", "stride", "path", "md", "pp", "cand_length", "cand", "cp", "trail", "cursor",
              "depth", "bound", "next", "nodes", "found", "status")
    good2 = dict(good1, ta=p(tabs[2]), ba=N[2], tb=p(tabs[3]), bb=N[3], floor=P["floor"], pp=528)
    order2 = ("cubies", "n", "pitch", "ta", "ba", "tb", "bb", "path", "md", "pp", "floor", "limit", "trail", "cursor", "depth", "bound", "next", "nodes",
              "status")

    def calls(phase, **kw):
        a = {**(good1 if phase == 1 else good2), **kw}
        args = [a[k] for k in (order1 if phase == 1 else order2)]
        init, search = (L.tp_phase1_init, L.tp_phase1_search) if phase == 1 else (L.tp_phase2_init, L.tp_phase2_search)
        rc = [init(*args, sp)]
        msg = [L.rc_last_error().decode()]
        rc.append(search(*args, a["steps"], a["running"], sp))
        msg.append(L.rc_last_error().decode())
        return rc, msg
    off = lambda k, by: ctypes.c_void_p(bufs[k].view.data_ptr() + by)
    shared = [("cubies", dict(cubies=None)), ("cubies", dict(cubies=p(rows.view, 4))), ("n is", dict(n=-1)), ("cubie_pitch", dict(pitch=rows.pitch - 8)),
              ("cubie_pitch", dict(pitch=256)), ("table_a", dict(ta=None)), ("table_a", dict(ta=p(tabs[0], 4))), ("bytes_a", dict(ba=1000)),
              ("table_b", dict(tb=None)), ("table_b", dict(tb=p(tabs[1], 8))), ("bytes_b", dict(bb=-1)), ("limit", dict(limit=None)),
              ("limit", dict(limit=off("limit", 4))), ("path is", dict(path=None)), ("path is", dict(path=off("path", 8))), ("max_depth", dict(md=0)),
              ("max_depth", dict(md=49)), ("path_pitch", dict(pp=512)), ("path_pitch", dict(pp=1064)), ("trail", dict(trail=None)),
              ("trail", dict(trail=off("trail", 8))), ("cursor", dict(cursor=None)), ("cursor", dict(cursor=off("cursor", 1))),
              ("depth", dict(depth=None)), ("depth", dict(depth=off("depth", 4))), ("bound", dict(bound=None)), ("bound", dict(bound=off("bound", 4))),
              ("next", dict(next=None)), ("next", dict(next=off("next", 8))), ("nodes", dict(nodes=None)), ("nodes", dict(nodes=off("nodes", 8))),
              ("status", dict(status=None)), ("status", dict(status=off("status", 2)))]
    only1 = [("candidates", dict(K=0)), ("candidates", dict(K=4097)), ("stride", dict(stride=512)), ("stride", dict(stride=520)),
             ("stride", dict(stride=1 << 31)), ("cand_length", dict(cand_length=None)), ("cand_length", dict(cand_length=off("cand_length", 4))),
             ("cand_cubies", dict(cand=None)), ("cand_cubies", dict(cand=off("cand", 8))), ("cand_pitch", dict(cp=1040)), ("cand_pitch", dict(cp=256)),
             ("found", dict(found=None)), ("found", dict(found=off("found", 4)))]
    only2 = [("floor", dict(floor=off("floor", 4)))]
    for phase, cases in ((1, shared + only1), (2, shared + only2)):
        for word, kw in cases:
            rc, msg = calls(phase, **kw)
            assert rc == [EINVAL, EINVAL], (phase, word, kw, rc)
            assert all(word in m and m.startswith(f"tp_phase{phase}_") for m in msg), (phase, word, msg)
        for word, kw in [("max_steps", dict(steps=0)), ("max_steps", dict(steps=T.max_steps() + 1)), ("running", dict(running=None)),
                         ("running", dict(running=off("running", 4)))]:
            rc, msg = calls(phase, **kw)
            assert rc == [0, EINVAL] and word in msg[1], (phase, word, rc, msg)
        assert calls(phase, n=0)[0] == [0, 0]                                # n == 0 succeeds without a launch
    assert call(n=0) == 0
    torch.cuda.synchronize()
    # the accepted inits above wrote their frames: refill, refuse once more, and look at every byte
    for a in bufs.values():
        a.upload()
    for phase in (1, 2):
        assert calls(phase, md=0)[0] == [EINVAL, EINVAL] and calls(phase, cubies=None)[0] == [EINVAL, EINVAL]
    torch.cuda.synchronize()
    for k, a in bufs.items():
        a.check(f"{k} after the refused calls")
    rows.check("rows after the refused calls")
    out.check("index after the refused calls")
    assert all(torch.equal(a, b) for a, b in zip(tabs, tp.tables)) and not bool(cnt.any())


# -------------------------------------------------------------------------------------------------------- 7. stream order
def _host_tabs(ctx):
    if "tp" not in ctx.cache:
        host = [R.bfs(w)[0] for w in range(4)]
        ctx.cache["tp"] = (host, [ctx.torch.as_tensor(t.copy()).to(ctx.dev) for t in host])
    return ctx.cache["tp"]


def _s_build_begin(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _lib, _twophase_lib as T
    which = int(variant)
    nb = R.SIZE[which]
    table = arena.output((nb,))

    def check(w):
        got = table.cpu().numpy()
        assert np.flatnonzero(got == 0).tolist() == [R.GOAL[which]] and (np.delete(got, R.GOAL[which]) == 0xFF).all()
    return C.built(lambda: _lib.check(T.twophase_lib().tp_build_begin(C.P(table), nb, which, ctx.sp())), [], check)


def _s_build_level(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _lib, _twophase_lib as T
    t = ctx.torch
    which, depth = (int(x) for x in variant.split("@"))
    nb, dist = R.SIZE[which], _host_tabs(ctx)[0][which]
    start = t.as_tensor(np.where(dist <= depth, dist, 0xFF).astype(np.uint8))
    want = np.where(dist <= depth + 1, dist, 0xFF).astype(np.uint8)
    want_count = R.LEVELS[which][depth + 1] if depth + 1 < len(R.LEVELS[which]) else 0
    table, count = arena.state((nb,)), arena.output((4,), t.int32)

    def check(w):
        C.vec_same(table, want, "table")
        assert int(count[0]) == want_count, ("count", int(count[0]), want_count)
    return C.built(lambda: _lib.check(T.twophase_lib().tp_build_level(C.P(table), nb, which, depth, C.P(count), ctx.sp())),
                   [lambda w: table.copy_(start)], check)


def _s_rows(which, w):
    n = C.N
    if which < 2:
        rows = chain_ref.unrank(1, np.random.default_rng(C._SEED[w] + which).integers(0, chain_ref.SIZE[1], n))[0]
        rows[:, 8:] ^= np.random.default_rng(C._SEED[w]).integers(0, 2, (n, 12)).astype(np.uint8)
    else:
        rows = np.concatenate([g1_walks(49, [30] * 49, seed=C._SEED[w] + which)] * 21)
    rows[-6:] = outside_rows()
    return rows


def _s_index(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _lib, _twophase_lib as T
    n, which = C.N, int(variant)
    rows = {w: _s_rows(which, w) for w in C.SETS}
    host = {w: C.tiled(ctx, rows[w], n) for w in C.SETS}
    src, out = arena.input((C.tiles_of(n), 20, C.pitch_of(n))), arena.output((n,), ctx.torch.int32)

    def check(w):
        want = R.index_rows(which, rows[w])
        assert (want == 0xFFFFFFFF).any() and (want != 0xFFFFFFFF).sum() > n // 2
        C.vec_same(out, want.view(np.int32), "index")
    return C.built(lambda: _lib.check(T.twophase_lib().tp_index(C.P(src), n, C.pitch_of(n), which, C.P(out), ctx.sp())),
                   [lambda w: src.copy_(host[w])], check, float_payload=True)        # an index may hold the poison byte


def _s_phase(ctx, cs, variant, arena):
    """One init or one search launch of a phase over 40 lanes; sets A and B are different cubes.  fill() rewrites every byte of every
    buffer; for a search row it then runs the init and 300 passes eagerly, and the captured call makes the next 500."""
    from rubiks_cube_solver_amd import _lib, _twophase_lib as T
    t = ctx.torch
    phase, what = int(variant[0]), variant[1:]
    host, dev = _host_tabs(ctx)
    n, K, pitch, md, before, steps = 40, 2, 48, 24, 300, 500
    cols = K * pitch if phase == 1 else pitch
    h = R.Heuristic(phase, host)
    M = {}
    for w in C.SETS:
        seed = C._SEED[w] + phase
        if phase == 1:
            rows = np.concatenate([rows_of(env_of(3, scrambles(3, [1 + i % 6 for i in range(n - 8)], seed=seed)))[1], g1_walks(2, [0, 4], seed), outside_rows()])
            prefixes, limit = [()] * n, [9] * n
        else:
            rows = np.concatenate([g1_walks(n - 6, [(i % 9) + 1 for i in range(n - 6)], seed), outside_rows()])
            prefixes = [((), (0,), (2, 2), (7, 4))[i % 4] for i in range(n)]
            limit = [20 if i % 5 else 3 for i in range(n)]
        M[w] = dict(rows=rows, prefixes=prefixes, limit=limit)
    cub = arena.input((20, pitch))
    limit, floor = arena.input((pitch,), t.int32), arena.input((pitch,), t.int32)
    path = arena.state((md, cols))
    trail, cursor, status = arena.state((pitch, 2), t.int64), arena.state((pitch,)), arena.state((pitch,))
    depth, bound, nxt, nodes = arena.state((pitch,), t.int32), arena.state((pitch,), t.int32), arena.state((pitch,), t.int32), arena.state((pitch,), t.int64)
    found = cand_length = cand = None
    if phase == 1:
        found, cand_length, cand = arena.state((pitch,), t.int32), arena.state((cols,), t.int32), arena.state((20, cols))
    running = arena.output((4,), t.int32) if what == "search" else None
    scratch = t.zeros(4, dtype=t.int32, device=ctx.dev)
    L = T.twophase_lib()
    frame = [C.P(trail), C.P(cursor), C.P(depth), C.P(bound), C.P(nxt), C.P(nodes)]
    if phase == 1:
        args = [C.P(cub), n, pitch, C.P(dev[0]), R.SIZE[0], C.P(dev[1]), R.SIZE[1], C.P(limit), K, pitch, C.P(path), md, cols, C.P(cand_length), C.P(cand),
                cols] + frame + [C.P(found), C.P(status)]
        init, search = L.tp_phase1_init, L.tp_phase1_search
    else:
        args = [C.P(cub), n, pitch, C.P(dev[2]), R.SIZE[2], C.P(dev[3]), R.SIZE[3], C.P(path), md, cols, C.P(floor), C.P(limit)] + frame + [C.P(status)]
        init, search = L.tp_phase2_init, L.tp_phase2_search

    def fill(w):
        m = M[w]
        cub.fill_(FILL)
        cub[:, :n] = t.as_tensor(np.ascontiguousarray(m["rows"].T)).to(ctx.dev)
        limit.fill_(-1), floor.zero_()
        limit[:n] = t.as_tensor(np.array(m["limit"], np.int32)).to(ctx.dev)
        grid = np.full((md, cols), R.NOOP, np.uint8)
        for c, pre in enumerate(m["prefixes"]):
            grid[:len(pre), c] = pre
        floor[:n] = t.as_tensor(np.array([len(pre) for pre in m["prefixes"]], np.int32)).to(ctx.dev)
        path.copy_(t.as_tensor(grid))
        for buf in (trail, cursor, status, depth, bound, nxt, nodes):
            buf.zero_()
        if phase == 1:
            found.zero_(), cand_length.zero_()
            cand.copy_(t.as_tensor(R.HOME_ROWS)[:, None].expand(20, cols))
        if what == "search":
            _lib.check(init(*args, ctx.sp()))
            _lib.check(search(*args, before, C.P(scratch), ctx.sp()))

    def check(w):
        m = M[w]
        passes = before + steps if what == "search" else 0
        if phase == 1:
            want = [R.Phase1(r.tolist(), h, K, lim, max_depth=md).run(max_passes=passes) for r, lim in zip(m["rows"], m["limit"])]
        else:
            want = [R.Phase2(r.tolist(), h, lim, prefix=pre, max_depth=md).run(max_passes=passes) for r, lim, pre in zip(m["rows"], m["limit"], m["prefixes"])]
        state = dict(trail=trail, cursor=cursor, depth=depth, bound=bound, next=nxt, nodes=nodes, status=status, path=path)
        if phase == 1:
            state.update(found=found, cand_length=cand_length, cand_cubies=cand)
        state = {k: v.cpu().numpy() for k, v in state.items()}
        if phase == 1:
            _check_phase1_md(state, want, K, pitch, md, w)
        else:
            check_phase2(state, want, m["prefixes"], w)
        assert any(f.status for f in want) and (what == "init" or any(f.passes > before for f in want))
        if what == "search":
            assert int(running[0]) == sum(1 for f in want if not f.status), "running"
    if what == "init":
        return C.built(lambda: _lib.check(init(*args, ctx.sp())), [fill], check)
    return C.built(lambda: _lib.check(search(*args, steps, C.P(running), ctx.sp())), [fill], check)


def _check_phase1_md(state, frames, K, stride, md, what):
    """check_phase1 for a path of md rows"""
    full = dict(state)
    full["path"] = np.concatenate([state["path"], np.full((R.MAX_DEPTH - md, state["path"].shape[1]), R.NOOP, np.uint8)])
    check_phase1(full, frames, K, stride, what)


TP_ROWS = [C.Row("tp_build_begin", _s_build_begin, (3,), (0, 1, 2, 3)), C.Row("tp_build_level", _s_build_level, (3,), ("0@0", "1@9", "2@0", "2@21", "3@18", "3@19")),
           C.Row("tp_index", _s_index, (3,), (0, 1, 2, 3)), C.Row("tp_phase1_init", _s_phase, (3,), ("1init",)),
           C.Row("tp_phase1_search", _s_phase, (3,), ("1search",)), C.Row("tp_phase2_init", _s_phase, (3,), ("2init",)),
           C.Row("tp_phase2_search", _s_phase, (3,), ("2search",))]
TP_CASES = [(f"{r.label}-{v}", r, v) for r in TP_ROWS for v in r.variants]


def test_every_launching_export_has_a_stream_row():
    from rubiks_cube_solver_amd import _twophase_lib as T
    host_only = {"tp_table_bytes", "tp_generators", "tp_max_steps"}          # launch nothing
    assert {r.export for r in TP_ROWS} == set(T.TWOPHASE_SIGNATURES) - host_only
    assert not {r.export for r in TP_ROWS} & {r.export for r in C.ROWS}


@pytest.fixture(scope="module")
def ctx(oracle):
    return C.Ctx(oracle, "cuda")


@pytest.mark.parametrize("row,variant", [c[1:] for c in TP_CASES], ids=[c[0] for c in TP_CASES])
def test_one_call_under_capture_and_replay(ctx, row, variant):
    from tests.test_gpu_stream_order import GraphBackend
    try:
        with torch.no_grad():
            D.run(GraphBackend(ctx.ops, ctx.L), lambda arena: row.build(ctx, 3, variant, arena))
    except Exception as e:  # noqa: BLE001
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")) and "capture" not in str(e).lower():
            pytest.exit(f"a GPU fault in this case: nothing more is started on the device -- {e}", returncode=3)
        raise
