"""The subgroup chain on the GPU (pattern.ChainTables, search.chain_solve, the rct_* entry points of librubikhip.so): the built tables
against the committed level counts and the restatement (tests/chain_ref.py; tests/golden/chain_tables.npz holds its tables of stages
0, 1 and 3, which tests/test_chain_host.py reproduces), every table proved to be a distance through the device's own sticker moves,
index / unrank / descent against the restatement bit for bit in every layout with carved operands, chain_solve by mathematics, every
argument error, each launching export under capture and replay.  All comparisons are exact.  GPU only."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from tests import chain_ref as R
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
LAYOUTS = ("tight", "padded", "t512")        # one tight tile, one tile padded to a pitch that is no power of two, 512-cube tiles
CHUNK = 1 << 20
ML = R.MAX_LENGTH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mods():
    from rubiks_cube_solver_amd import _chain_lib, _lib, ops, pattern, search
    return _lib, _chain_lib, ops, pattern, search


def stream():
    from rubiks_cube_solver_amd import _lib
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def ceil16(n):
    return -(-n // 16) * 16


@pytest.fixture(scope="module")
def chain():
    _, _, _, pattern, _ = mods()
    return pattern.ChainTables.build(DEV)


@pytest.fixture(scope="module")
def host(chain):
    return [t.cpu().numpy() for t in chain.tables]


@pytest.fixture(scope="module")
def walked(host):
    """2565 cubes scrambled by 100 device moves, and the restatement's four descents of them through the DEVICE's tables (equal to
    the restatement's own by the table tests): per stage the rows, actions, lengths at entry and everything the descent returns."""
    _, _, ops, _, _ = mods()
    n = max(COUNTS)
    env = env_of(3, scrambles(3, [100] * n, seed=5))
    states = ops.to_aos(env.stickers, n).cpu().numpy()
    from rubiks_cube_solver_amd.tables import get_cubies
    rows = get_cubies(3).cubies(states)[0]
    actions, length = np.full((ML, n), R.NOOP, np.uint8), np.zeros(n, np.int32)
    stages = []
    for s in range(4):
        out = R.descend(s, host[s], rows, actions, length, ML)
        stages.append(dict(rows=rows, actions=actions, length=length, out=out))
        rows, actions, length = out[:3]
        assert not out[4].any()
    return dict(env=env, states=states, stages=stages, length=length, actions=actions, moves=np.stack([s["out"][3] for s in stages]))


# ---------------------------------------------------------------------------------------------------------------- 1. tables
def test_tables_have_the_levels_and_equal_the_restatement(chain, host):
    _, _, _, pattern, _ = mods()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "chain_tables.npz"))
    assert chain.levels == R.LEVELS and chain.depth == R.DEPTH
    for s in range(4):
        t = host[s]
        assert t.dtype == np.uint8 and len(t) == R.SIZE[s]
        assert tuple(np.bincount(t[t != R.NONE])) == R.LEVELS[s] and (t == R.NONE).sum() == R.SIZE[s] - sum(R.LEVELS[s])
        assert (np.flatnonzero(t == 0) == R.goal_indices(s)).all()
        if s != 2:
            assert (t == gold[f"stage{s}"]).all(), s
    again = pattern.ChainTables.build(DEV)                                   # building twice gives identical bytes
    assert again.levels == chain.levels and all(torch.equal(a, b) for a, b in zip(again.tables, chain.tables))
    wrapped = pattern.ChainTables([t.clone() for t in chain.tables])         # tables loaded from disk
    assert wrapped.levels is None and wrapped.depth is None
    with pytest.raises(ValueError):
        pattern.ChainTables([t[1:] for t in chain.tables])


@pytest.mark.parametrize("stage", range(4))
def test_table_is_the_distance_through_the_device_moves(chain, host, stage):
    """Every index that is not 0xFF: rct_unrank -> rcc_from_cubies (status 0 from rcc_cubies) -> rc_apply_moves per generator ->
    rcc_cubies -> rct_index -> the table.  The unranked cube reads back as its index; every child stays in the domain and differs by
    at most 1; some child is one closer exactly where the entry is not 0; 0 occurs exactly at the restated goals.  A byte array
    with these properties IS the least number of generators to a goal."""
    _, _, ops, _, _ = mods()
    t = chain.tables[stage]
    idx_all = np.flatnonzero(host[stage] != R.NONE)
    assert len(idx_all) == sum(R.LEVELS[stage])
    goal = torch.zeros(R.SIZE[stage], dtype=torch.bool, device=DEV)
    goal[torch.from_numpy(R.goal_indices(stage)).to(DEV)] = True
    for at in range(0, len(idx_all), CHUNK):
        part = torch.from_numpy(idx_all[at:at + CHUNK]).to(DEV)
        n = len(part)
        cub = chain.cubies(part, stage)                                      # raises if an index were flagged
        st = ops.from_cubies(cub, n, 3)
        assert not bool(ops.cubies(st, n, 3, cubies=False, status=True)["status"].any())
        assert torch.equal(chain.index(cub, stage, n), part)
        h = t[part].int()
        assert torch.equal(chain.distance(cub, stage, n).int(), h)
        down = torch.zeros(n, dtype=torch.bool, device=DEV)
        child = torch.empty_like(st)
        for gen in R.GENERATORS[stage]:
            acts = torch.full((n,), gen[0], dtype=torch.uint8, device=DEV)
            ops.apply_moves(st, child, acts, n, 3)
            if len(gen) == 2:
                ops.apply_moves(child, child, acts, n, 3)
            ci = chain.index(ops.cubies(child, n, 3, status=False)["cubies"], stage, n)
            assert bool((ci >= 0).all()), gen
            hc = t[ci].int()
            assert bool(((hc - h).abs() <= 1).all()), gen
            down |= hc == h - 1
        assert bool((down == (h > 0)).all())
        assert bool(((h == 0) == goal[part]).all())


# ------------------------------------------------------------------------------------------------------ 2. index and unrank
def outside_rows():
    """Rows outside the domains: one flipped edge pair, one twisted pair, a slice edge out of its slice, a corner permutation outside H
    (a quarter turn of U), a byte >= 24, a piece twice, 0xFF."""
    from rubiks_cube_solver_amd.tables import get_cubies, get_tables
    out = np.tile(R.HOME_ROWS, (8, 1))
    out[0, [8, 9]] = 1, 3
    out[1, [0, 1]] = 1, 5
    out[2, [8, 16]] = 16, 0
    out[3] = get_cubies(3).cubies(R.move(get_tables(3).solved[None, :], (R.U,)))[0][0]
    out[4, 12] = 24
    out[5, 9] = 0
    out[6, 3] = 0xFF
    out[7, 2] = 3                                                            # corner piece 1 twice
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_unrank_and_index_in_every_layout_carved(chain, walked, n):
    """rct_unrank into layout X and rct_index from it, every operand 16 bytes past a 32-byte boundary: the rows are the restatement's,
    an index >= N and a stage-3 index of the wrong parity are written solved and flagged, the indices read back, guards and pad
    columns keep their bytes.  Then rct_index on walked cubes of each domain (the restated descents' rows) with rows outside it."""
    _, CL, _, _, _ = mods()
    L = CL.chain_lib()
    rng = np.random.default_rng(n)
    for stage in range(4):
        N = R.SIZE[stage]
        idx = rng.integers(0, N, n).astype(np.uint32)
        idx[0] = N - 1
        for flagged in (False, True):
            if flagged:
                idx[n - 1] = N
                if n > 600:
                    idx[[7, 600]] = 0xFFFFFFFF, N + 12345
            want, bad = R.unrank(stage, np.where(idx >= N, -1, idx.astype(np.int64)))
            if stage == 3 and not flagged:                                   # make the plain run parity-right
                idx = np.where(bad, idx ^ 1, idx).astype(np.uint32)
                want, bad = R.unrank(stage, idx.astype(np.int64))
            assert bad.any() == flagged
            back = R.index_rows(stage, want)
            for lay in LAYOUTS:
                offs = LC.carve_offsets(4)
                ind = Arena(4 * n, offs[0])
                ind.expect(idx)
                ind.upload()
                cub = rows_arena(None, n, 20, lay, offs[1]).upload()
                flag = Arena(16, offs[2])
                flag.host[flag.start] = 0
                flag.upload()
                out = Arena(4 * n, offs[3]).upload()
                assert L.rct_unrank(ind.ptr(), n, stage, cub.ptr(), cub.pitch, flag.ptr(), stream()) == 0, L.rc_last_error()
                assert L.rct_index(cub.ptr(), n, cub.pitch, stage, out.ptr(), stream()) == 0, L.rc_last_error()
                cub.expect_rows(want, cub.pitch)
                flag.host[flag.start] = int(flagged)
                out.expect(back)
                for a, what in ((ind, "indices"), (cub, "cubies"), (flag, "bad"), (out, "index")):
                    a.check(f"stage {stage} n={n} {lay} flagged={flagged}: {what}")
        rows = walked["stages"][stage]["rows"][:n].copy()
        if n >= 8:
            rows[-8:] = outside_rows()
        want = R.index_rows(stage, rows)
        assert (want[:max(1, n - 8)] != 0xFFFFFFFF).all()
        if n >= 8:
            assert (want[-4:] == 0xFFFFFFFF).all() and (want[-8:-4] == 0xFFFFFFFF).sum() == (0, 1, 3, 4)[stage]
        for lay in LAYOUTS:
            offs = LC.carve_offsets(2)
            cub = rows_arena(rows, n, 20, lay, offs[0]).upload()
            out = Arena(4 * n, offs[1]).upload()
            assert L.rct_index(cub.ptr(), n, cub.pitch, stage, out.ptr(), stream()) == 0, L.rc_last_error()
            out.expect(want)
            cub.check(f"stage {stage} n={n} {lay}: cubies")
            out.check(f"stage {stage} n={n} {lay}: index of walked and outside rows")


# ---------------------------------------------------------------------------------------------------------------- 3. descent
def run_descend(L, table, stage, rows, actions, length, max_length, lay, want, what, act_extra=0):
    """One rct_descend call with every operand carved 16 bytes past a 32-byte boundary; every byte of every allocation is checked
    against `want` = the restatement's (rows, actions, length, moves, status)."""
    n = len(rows)
    offs = LC.carve_offsets(5)
    ap = ceil16(n) + act_extra
    cub = rows_arena(rows, n, 20, lay, offs[0]).upload()
    act = Arena(max_length * ap, offs[1])
    grid = np.full((max_length, ap), FILL, np.uint8)
    grid[:, :n] = actions[:max_length, :n]
    act.expect(grid)
    act.upload()
    ln = Arena(4 * n, offs[2])
    ln.expect(length.astype(np.int32))
    ln.upload()
    mv, st = Arena(n, offs[3]).upload(), Arena(n, offs[4]).upload()
    rc = L.rct_descend(cub.ptr(), n, cub.pitch, stage, p(table), table.numel(), act.ptr(), max_length, ap, ln.ptr(), mv.ptr(), st.ptr(), stream())
    assert rc == 0, L.rc_last_error()
    cub.expect_rows(want[0], cub.pitch)
    grid[:, :n] = want[1][:max_length, :n]
    act.expect(grid)
    ln.expect(want[2].astype(np.int32))
    mv.expect(want[3])
    st.expect(want[4])
    for a, name in ((cub, "cubies"), (act, "actions"), (ln, "length"), (mv, "moves"), (st, "status")):
        a.check(f"{what}: {name}")


@pytest.mark.parametrize("n", COUNTS)
def test_descend_equals_the_restatement_bit_for_bit(chain, walked, n):
    """Stage by stage on the walked cubes (the entry lengths of stages 1..3 are what the earlier stages left): cubie rows, actions,
    length, moves and status, in every layout, with guards and pad columns untouched."""
    _, CL, _, _, _ = mods()
    L = CL.chain_lib()
    for stage in range(4):
        s = walked["stages"][stage]
        want = tuple(x[:n] if x.ndim == 1 or x.shape[1] == 20 else x[:, :n] for x in s["out"])
        assert stage == 0 or s["length"][:n].any()
        for i, lay in enumerate(LAYOUTS):
            run_descend(L, chain.tables[stage], stage, s["rows"][:n], s["actions"][:, :n], s["length"][:n], ML, lay, want,
                        f"stage {stage} n={n} {lay}", act_extra=32 * i)


def test_descend_without_room_illegal_rows_and_foreign_tables(chain, host, walked):
    """513 cubes.  A max_length that leaves no room for some cubes; rows that are illegal or outside the domain among the walked ones;
    another stage's table, under which the walk is RCT_STUCK or RCT_OUTSIDE for some cubes and ends for all.  Each case equals the
    restatement bit for bit."""
    _, CL, _, _, _ = mods()
    L, n = CL.chain_lib(), 513
    for stage in range(4):
        s = walked["stages"][stage]
        rows, acts, ln = s["rows"][:n].copy(), s["actions"][:, :n], s["length"][:n].copy()
        # no room: the median of what the cubes need
        need = ln + 2 * s["out"][3][:n].astype(np.int32)
        short = int(np.median(need[s["out"][3][:n] > 0])) if stage else 10
        want = R.descend(stage, host[stage], rows, acts[:short], np.minimum(ln, short), short)
        assert (want[4] == R.NO_ROOM).any() and (want[4] == 0).any()
        run_descend(L, chain.tables[stage], stage, rows, acts[:short], np.minimum(ln, short), short, "padded", want, f"stage {stage} no room")
        ln2 = ln.copy()
        ln2[5] = -1                                                          # a negative entry length is refused the same way
        rows[-8:] = outside_rows()
        want = R.descend(stage, host[stage], rows, acts, ln2, ML)
        assert want[4][5] == R.NO_ROOM and (want[4][-4:] == R.ILLEGAL).all() and (want[3][-4:] == R.NONE).all()
        assert (want[4][-8:-4] == R.OUTSIDE).sum() == (0, 1, 3, 4)[stage]
        run_descend(L, chain.tables[stage], stage, rows, acts, ln2, ML, "t512", want, f"stage {stage} illegal rows")
    for stage, other in ((0, 2), (0, 3), (3, 2), (1, 2)):                     # tables at least as large as the stage's N
        s = walked["stages"][stage]
        rows, acts, ln = s["rows"][:n], s["actions"][:, :n], np.zeros(n, np.int32)
        want = R.descend(stage, host[other], rows, acts, ln, ML)
        assert ((want[4] & (R.STUCK | R.OUTSIDE)) != 0).any() and np.isin(want[4], (0, R.STUCK, R.OUTSIDE)).all()
        run_descend(L, chain.tables[other], stage, rows, acts, ln, ML, "tight", want, f"stage {stage} under the table of stage {other}")


# ------------------------------------------------------------------------------------------------------------ 4. chain_solve
def check_solution(states, res, n):
    """The actions replayed on the oracle solve every cube at exactly `length`; beyond it only the no-op."""
    from rubiks_cube_solver_amd.tables import get_tables
    solved = get_tables(3).solved
    length, actions = res["length"].cpu().numpy(), res["actions"].cpu().numpy()
    assert res["solved"].cpu().numpy().all() and (length >= 0).all() and (length <= R.MAX_LENGTH).all()
    assert actions.shape == (max(1, int(length.max())), n) and actions.dtype == np.uint8
    rows = np.arange(actions.shape[0])[:, None]
    assert (actions[rows >= length[None, :]] == R.NOOP).all() and (actions[rows < length[None, :]] < 12).all()
    assert (R.replay(states, actions) == solved).all()
    early = actions.copy()
    early[np.maximum(length - 1, 0), np.arange(n)] = R.NOOP                  # without its last move no cube is solved yet
    assert ((R.replay(states, early) != solved).any(1) == (length > 0)).all()
    return length, actions


def test_chain_solve_by_mathematics(chain, host, walked):
    _, CL, ops, _, S = mods()
    n, env, states = max(COUNTS), walked["env"], walked["states"]
    before = env.stickers.clone()
    res = S.chain_solve(chain, env)
    assert torch.equal(env.stickers, before)                                 # the env is left as it is
    length, actions = check_solution(states, res, n)
    moves = res["stage_moves"].cpu().numpy()
    assert not res["status"].cpu().numpy().any() and moves.shape == (4, n)
    # stage_moves = the table value at entry; each stage's output has the next stage's index defined (else that row were 0xFF)
    assert (moves == walked["moves"]).all() and (moves != R.NONE).all() and (moves <= np.array(R.DEPTH)[:, None]).all()
    assert (moves[0] == host[0][R.index(0, states)]).all() and (moves[0] == env.chain_solve(chain)["stage_moves"][0].cpu().numpy()).all()
    assert (length == walked["length"]).all() and (actions == walked["actions"][:actions.shape[0]]).all()
    assert (length >= moves.astype(int).sum(0)).all() and (length <= moves[0] + 2 * moves[1:].astype(int).sum(0)).all()
    print(f"chain_solve of {n} cubes after 100 moves: length mean {length.mean():.1f} max {length.max()} min {length.min()}; generators max {moves.astype(int).sum(0).max()}")
    assert (chain.distance(env, 0).cpu().numpy() == moves[0]).all()
    g = S.chain_solve(chain, env, graph=True)                                # the same launches as one hipGraph
    for k in ("solved", "length", "actions", "stage_moves", "status"):
        assert torch.equal(g[k], res[k]), k
    assert torch.equal(env.stickers, before)


def test_chain_solve_near_solved_and_solved_cubes(chain):
    """The 1 + 12 + 114 cubes at distance <= 2 from solved, and a batch of solved cubes."""
    _, _, ops, _, S = mods()
    seqs = [()] + [(a,) for a in range(12)] + list(itertools.product(range(12), repeat=2))
    scr = np.full((len(seqs), 2), 12, np.uint8)
    for i, q in enumerate(seqs):
        scr[i, :len(q)] = q
    env = env_of(3, scr)
    states = ops.to_aos(env.stickers, len(seqs)).cpu().numpy()
    assert len(np.unique(states, axis=0)) == 1 + 12 + 114
    res = S.chain_solve(chain, env)
    length, _ = check_solution(states, res, len(seqs))
    assert length[0] == 0 and (length[1:13] >= 1).all()
    env = env_of(3, np.full((5, 1), 12, np.uint8))
    res = S.chain_solve(chain, env)
    assert res["length"].cpu().numpy().tolist() == [0] * 5 and res["actions"].cpu().numpy().tolist() == [[12] * 5]
    assert res["solved"].all() and not res["stage_moves"].any()


def test_illegal_cubes_are_not_walked(chain, walked):
    """A batch that holds cubes no move sequence reaches -- a twisted corner, a flipped edge, two edges traded, a wrong centre --
    solves the legal ones exactly as without them and returns -1, no-ops and RCT_ILLEGAL for the rest."""
    _, CL, ops, _, S = mods()
    from rubiks_cube_solver_amd import VecCubeEnv
    from rubiks_cube_solver_amd.tables import get_cubies
    cb, n = get_cubies(3), 40
    states = walked["states"][:n].copy()
    rows = cb.cubies(states)[0]
    rows[3, 0] = rows[3, 0] // 3 * 3 + (rows[3, 0] + 1) % 3
    rows[7, 8] ^= 1
    rows[11, [8, 9]] = rows[11, [9, 8]]
    states[[3, 7, 11]] = cb.from_cubies(rows[[3, 7, 11]])[0]
    states[20, cb.fixed[0]] = (states[20, cb.fixed[0]] + 1) % 6              # a centre
    env = VecCubeEnv(n, DEV, 3, obs=None)
    env.set_sim_cube(states, check=False)
    bad = np.zeros(n, bool)
    bad[[3, 7, 11, 20]] = True
    assert ((env.legality().cpu().numpy() != 0) == bad).all()
    for graph in (False, True):
        res = S.chain_solve(chain, env, graph=graph)
        length, actions = res["length"].cpu().numpy(), res["actions"].cpu().numpy()
        assert (res["solved"].cpu().numpy() == ~bad).all() and (length[bad] == -1).all() and (actions[:, bad] == R.NOOP).all()
        assert (res["status"].cpu().numpy()[bad] == R.ILLEGAL).all() and not res["status"].cpu().numpy()[~bad].any()
        assert (length[~bad] == walked["length"][:n][~bad]).all()
        assert (actions[:, ~bad] == walked["actions"][:actions.shape[0], :n][:, ~bad]).all()


def test_the_222_raises(chain):
    _, _, _, pattern, S = mods()
    env2 = env_of(2, scrambles(2, [3, 3], seed=1))
    before = env2.stickers.clone()
    for call in (lambda: S.chain_solve(chain, env2), lambda: env2.chain_solve(chain), lambda: chain.index(env2, 0), lambda: chain.distance(env2, 1),
                 lambda: pattern.ChainTables.build(DEV, cube_size=2), lambda: pattern.ChainTables(chain.tables, cube_size=2),
                 lambda: chain.index(env_of(3, scrambles(3, [3], seed=1)), 4), lambda: chain.cubies([0], -1)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(env2.stickers, before)
    with pytest.raises(IndexError):
        chain.cubies([0, R.SIZE[1]], 1)
    with pytest.raises(IndexError):
        chain.cubies([1], 3)                                                 # e = 1 alone: an odd edge permutation under even corners


# ------------------------------------------------------------------------------------------------------- 5. argument errors
def test_argument_errors_write_nothing(chain):
    _, CL, _, _, _ = mods()
    L, n, sp = CL.chain_lib(), 513, stream()
    tb = chain.tables[0]
    N = tb.numel()
    before = tb.clone()
    rows = rows_arena(np.tile(R.HOME_ROWS, (n, 1)), n, 20, "tight", 0).upload()
    out = Arena(4 * n + 16, 0).upload()
    act = Arena(ML * 528, 0).upload()
    ln, mv, st = Arena(4 * n + 16, 0).upload(), Arena(n + 16, 0).upload(), Arena(n + 16, 0).upload()
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    flag = torch.zeros(16, dtype=torch.uint8, device=DEV)
    ind = torch.zeros(16, dtype=torch.int32, device=DEV)
    cub = torch.full((20, 16), FILL, dtype=torch.uint8, device=DEV)
    refused = []
    for s in (-1, 4, 255):
        refused += [L.rct_build_begin(p(tb), 1 << 22, s, sp), L.rct_build_level(p(tb), 1 << 22, s, 0, p(cnt), sp),
                    L.rct_index(rows.ptr(), n, rows.pitch, s, out.ptr(), sp), L.rct_unrank(p(ind), 3, s, p(cub), 16, p(flag), sp),
                    L.rct_descend(rows.ptr(), n, rows.pitch, s, p(tb), 1 << 22, act.ptr(), ML, 528, ln.ptr(), mv.ptr(), st.ptr(), sp),
                    L.rct_generators(s, None, None)]
    refused += [L.rct_build_begin(None, N, 0, sp), L.rct_build_begin(p(tb, 8), N, 0, sp), L.rct_build_begin(p(tb), N - 1, 0, sp),
                L.rct_build_begin(p(tb), -1, 0, sp), L.rct_build_begin(p(tb), N, 1, sp),
                L.rct_build_level(p(tb), N - 1, 0, 0, p(cnt), sp), L.rct_build_level(p(tb), N, 0, -1, p(cnt), sp),
                L.rct_build_level(p(tb), N, 0, 254, p(cnt), sp), L.rct_build_level(p(tb), N, 0, 0, None, sp),
                L.rct_build_level(p(tb), N, 0, 0, p(cnt, 4), sp), L.rct_build_level(None, N, 0, 0, p(cnt), sp),
                L.rct_unrank(None, 3, 0, p(cub), 16, p(flag), sp), L.rct_unrank(p(ind, 4), 3, 0, p(cub), 16, p(flag), sp),
                L.rct_unrank(p(ind), 3, 0, None, 16, p(flag), sp), L.rct_unrank(p(ind), 3, 0, p(cub, 8), 16, p(flag), sp),
                L.rct_unrank(p(ind), 3, 0, p(cub), 8, p(flag), sp), L.rct_unrank(p(ind), 17, 0, p(cub), 16, p(flag), sp),
                L.rct_unrank(p(ind), 3, 0, p(cub), 16, None, sp), L.rct_unrank(p(ind), -1, 0, p(cub), 16, p(flag), sp)]
    assert all(rc == EINVAL for rc in refused), refused
    good = dict(cubies=rows.ptr(), n=n, pitch=rows.pitch, stage=0, index=out.ptr())
    call = lambda **kw: (lambda a: L.rct_index(a["cubies"], a["n"], a["pitch"], a["stage"], a["index"], sp))({**good, **kw})
    for word, kw in [("cubies", dict(cubies=None)), ("cubies", dict(cubies=p(rows.view, 8))), ("n is", dict(n=-1)), ("pitch", dict(pitch=rows.pitch - 8)),
                     ("pitch", dict(pitch=256)), ("index", dict(index=None)), ("index", dict(index=p(out.view, 4))), ("stage", dict(stage=4))]:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in L.rc_last_error().decode(), (word, L.rc_last_error())
    good2 = dict(cubies=rows.ptr(), n=n, pitch=rows.pitch, stage=0, table=p(tb), bytes=N, actions=act.ptr(), ml=ML, ap=528, length=ln.ptr(),
                 moves=mv.ptr(), status=st.ptr())
    call2 = lambda **kw: (lambda a: L.rct_descend(a["cubies"], a["n"], a["pitch"], a["stage"], a["table"], a["bytes"], a["actions"], a["ml"], a["ap"],
                                                  a["length"], a["moves"], a["status"], sp))({**good2, **kw})
    for word, kw in [("cubies", dict(cubies=None)), ("cubies", dict(cubies=p(rows.view, 4))), ("n is", dict(n=-1)), ("pitch", dict(pitch=rows.pitch - 8)),
                     ("pitch", dict(pitch=256)), ("table", dict(table=None)), ("table", dict(table=p(tb, 4))), ("bytes", dict(bytes=N - 1)),
                     ("bytes", dict(bytes=0)), ("bytes", dict(stage=1)), ("actions", dict(actions=None)), ("actions", dict(actions=p(act.view, 8))),
                     ("max_length", dict(ml=0)), ("max_length", dict(ml=-3)), ("act_pitch", dict(ap=512)), ("act_pitch", dict(ap=520)),
                     ("length", dict(length=None)), ("length", dict(length=p(ln.view, 4))), ("moves", dict(moves=None)),
                     ("moves", dict(moves=p(mv.view, 1))), ("status", dict(status=None)), ("status", dict(status=p(st.view, 2)))]:
        assert call2(**kw) == EINVAL, (word, kw)
        assert word in L.rc_last_error().decode(), (word, L.rc_last_error())
    assert call(n=0) == 0 and call2(n=0) == 0 and L.rct_unrank(p(ind), 0, 0, p(cub), 16, p(flag), sp) == 0   # n == 0 succeeds without a launch
    torch.cuda.synchronize()
    for a, what in ((rows, "rows"), (out, "index"), (act, "actions"), (ln, "length"), (mv, "moves"), (st, "status")):
        a.check(f"{what} after the refused calls")
    assert torch.equal(tb, before) and not bool(flag.any()) and not bool(cnt.any()) and bool((cub == FILL).all())


# -------------------------------------------------------------------------------------------------------- 6. stream order
def _gold(ctx, stage):
    key = ("chain", stage)
    if key not in ctx.cache:
        host = np.load(os.path.join(ROOT, "tests", "golden", "chain_tables.npz"))[f"stage{stage}"]
        ctx.cache[key] = (host, ctx.torch.as_tensor(host).to(ctx.dev))
    return ctx.cache[key]


def _s_build_begin(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _chain_lib, _lib
    stage = int(variant)
    nb = R.SIZE[stage]
    table = arena.output((nb,))
    goals = R.goal_indices(stage)

    def check(w):
        got = table.cpu().numpy()
        assert (np.flatnonzero(got == 0) == goals).all() and (np.delete(got, goals) == 0xFF).all()
    return C.built(lambda: _lib.check(_chain_lib.chain_lib().rct_build_begin(C.P(table), nb, stage, ctx.sp())), [], check)


def _s_build_level(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _chain_lib, _lib
    t = ctx.torch
    stage, depth = (int(x) for x in variant.split("@"))
    nb, dist = R.SIZE[stage], _gold(ctx, stage)[0]
    start = t.as_tensor(np.where(dist <= depth, dist, 0xFF).astype(np.uint8))
    want = np.where(dist <= depth + 1, dist, 0xFF).astype(np.uint8)
    want_count = R.LEVELS[stage][depth + 1] if depth + 1 < len(R.LEVELS[stage]) else 0
    table, count = arena.state((nb,)), arena.output((4,), t.int32)

    def check(w):
        C.vec_same(table, want, "table")
        assert int(count[0]) == want_count, ("count", int(count[0]), want_count)
    return C.built(lambda: _lib.check(_chain_lib.chain_lib().rct_build_level(C.P(table), nb, stage, depth, C.P(count), ctx.sp())),
                   [lambda w: table.copy_(start)], check)


def _s_indices(stage, w):
    i = np.random.default_rng(C._SEED[w] + stage).integers(0, R.SIZE[stage], C.N).astype(np.int64)
    if stage == 3:
        i = np.where(R.unrank(3, i)[1], i ^ 1, i)
    i[11 if w == "A" else 1000] = R.SIZE[stage] + 5
    return i


def _s_unrank(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _chain_lib, _lib
    n, stage = C.N, int(variant)
    idxs = {w: _s_indices(stage, w) for w in C.SETS}
    index, f1 = C.vec_input(ctx, arena, {w: idxs[w].astype(np.uint32).view(np.int32) for w in C.SETS})
    cub, bad = arena.output((C.tiles_of(n), 20, C.pitch_of(n))), arena.state((16,))

    def check(w):
        e_cub, e_bad = R.unrank(stage, np.where(idxs[w] >= R.SIZE[stage], -1, idxs[w]))
        assert e_bad.sum() == 1
        C.same(ctx, cub, n, e_cub, "cubies")
        assert bad.cpu().numpy().tolist() == [1] + [0] * 15, "bad"
    return C.built(lambda: _lib.check(_chain_lib.chain_lib().rct_unrank(C.P(index), n, stage, C.P(cub), C.pitch_of(n), C.P(bad), ctx.sp())),
                   [f1, lambda w: bad.zero_()], check)


def _s_rows(stage, w):
    rows = R.unrank(stage, np.minimum(_s_indices(stage, w), R.SIZE[stage] - 1))[0]
    rows[-8:] = outside_rows()
    return rows


def _s_index(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _chain_lib, _lib
    n, stage = C.N, int(variant)
    host = {w: C.tiled(ctx, _s_rows(stage, w), n) for w in C.SETS}
    src, out = arena.input((C.tiles_of(n), 20, C.pitch_of(n))), arena.output((n,), ctx.torch.int32)

    def check(w):
        want = R.index_rows(stage, _s_rows(stage, w))
        assert (want == 0xFFFFFFFF).any() and (want != 0xFFFFFFFF).sum() > n // 2
        C.vec_same(out, want.view(np.int32), "index")
    return C.built(lambda: _lib.check(_chain_lib.chain_lib().rct_index(C.P(src), n, C.pitch_of(n), stage, C.P(out), ctx.sp())),
                   [lambda w: src.copy_(host[w])], check, float_payload=True)        # an index may hold the poison byte


def _s_descend(ctx, cs, variant, arena):
    """Cubes of the stage's domain by rct_unrank's rule (the restatement's), eight rows outside it, entry lengths 0..3."""
    from rubiks_cube_solver_amd import _chain_lib, _lib
    t = ctx.torch
    n, stage = C.N, int(variant)
    dist, table = _gold(ctx, stage)
    ap = C.pitch_of(n) * C.tiles_of(n)
    M = {}
    for w in C.SETS:
        rows = _s_rows(stage, w)
        ln = (np.arange(n) % 4).astype(np.int32)
        acts = np.full((40, ap), R.NOOP, np.uint8)
        M[w] = dict(rows=C.tiled(ctx, rows, n), ln=t.as_tensor(ln), want=R.descend(stage, dist, rows, acts, ln, 40))
        assert (M[w]["want"][4] == 0).sum() > n // 2 and (M[w]["want"][4] != 0).any()
    cub, act = arena.state((C.tiles_of(n), 20, C.pitch_of(n))), arena.state((40, ap))
    length, moves, status = arena.state((n,), t.int32), arena.output((n,)), arena.output((n,))

    def check(w):
        rows, acts, ln, mv, st = M[w]["want"]
        C.same(ctx, cub, n, rows, "cubies")
        C.vec_same(act, acts, "actions")
        C.vec_same(length, ln, "length")
        C.vec_same(moves, mv, "moves")
        C.vec_same(status, st, "status")
    return C.built(lambda: _lib.check(_chain_lib.chain_lib().rct_descend(C.P(cub), n, C.pitch_of(n), stage, C.P(table), table.numel(), C.P(act), 40, ap,
                                                                         C.P(length), C.P(moves), C.P(status), ctx.sp())),
                   [lambda w: cub.copy_(M[w]["rows"]), lambda w: act.fill_(R.NOOP), lambda w: length.copy_(M[w]["ln"])], check)


# the form of tests/stream_cases.py ROWS, kept here: that table is pinned to the eight signature tables it lists
CHAIN_ROWS = [C.Row("rct_build_begin", _s_build_begin, (3,), (0, 1, 3)), C.Row("rct_build_level", _s_build_level, (3,), ("0@0", "0@6", "1@4", "3@14", "3@15")),
              C.Row("rct_unrank", _s_unrank, (3,), (0, 1, 3)), C.Row("rct_index", _s_index, (3,), (0, 1, 3)),
              C.Row("rct_descend", _s_descend, (3,), (0, 1, 3))]
CHAIN_CASES = [(f"{r.label}-{v}", r, v) for r in CHAIN_ROWS for v in r.variants]


def test_every_launching_export_has_a_stream_row():
    from rubiks_cube_solver_amd import _chain_lib
    host_only = {"rct_table_bytes", "rct_generators", "rct_corner_cosets"}   # launch nothing
    assert {r.export for r in CHAIN_ROWS} == set(_chain_lib.CHAIN_SIGNATURES) - host_only
    assert not {r.export for r in CHAIN_ROWS} & {r.export for r in C.ROWS}


@pytest.fixture(scope="module")
def ctx(oracle):
    return C.Ctx(oracle, "cuda")


@pytest.mark.parametrize("row,variant", [c[1:] for c in CHAIN_CASES], ids=[c[0] for c in CHAIN_CASES])
def test_one_call_under_capture_and_replay(ctx, row, variant):
    """Stage 2 has no committed table: its rows would have to build one by the 90-second search, and its kernels are the template the
    other stages instantiate; the table, index, unrank and descent tests above cover it at every index."""
    from tests.test_gpu_stream_order import GraphBackend
    try:
        with torch.no_grad():
            D.run(GraphBackend(ctx.ops, ctx.L), lambda arena: row.build(ctx, 3, variant, arena))
    except Exception as e:  # noqa: BLE001
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")) and "capture" not in str(e).lower():
            pytest.exit(f"a GPU fault in this case: nothing more is started on the device -- {e}", returncode=3)
        raise
